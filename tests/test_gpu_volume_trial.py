"""Volume-change trial moves (mpmc_trial_volume_begin; System::volume_change / volume_change_Gibbs with revert_volume_change as the
rejection, reference src/System.MonteCarlo.cpp:1235-1340, 1690-1727).

What is held, and to what:
  - the move itself bit for bit: the device's positions (mpmc_debug_device_positions) and the host's (mpmc_trial_volume_get) against a
    restatement with sequential Python-float sums; basis = b * s elementwise; reciprocal, volume, cutoff = mpmc_pbc_compute of the product;
  - the trial's energies against the oracle on the host-scaled configuration at 1e-9 and against a fresh context at 1e-11 (two of the
    library's own paths over the same doubles), counts exactly;
  - a rejected trial leaves nothing behind: the bits of a displacement trial, an insertion trial, a batch of insertion candidates and of
    energy() are those of before, the following trials are deltas, and no evaluation ran inside the reject;
  - an accepted trial is the new accepted configuration without a further evaluation.
Scale factors 0.97, 1.04 and nextafter(1, 2).  None of the scaled boxes has a pair the reference turns non-finite (every oracle energy
below is asserted finite)."""
import ctypes

import numpy as np
import pytest

import util
from mpmcxx_amd import energy
from volume_trial_cases import TERM_FIXTURES, host_scale  # (the one restatement of the move; shared with the follow-up tests)

pytestmark = pytest.mark.gpu

SCALES = [0.97, 1.04, float(np.nextafter(1.0, 2.0))]
ERR_ARG, ERR_INVALID_DATUM = -3, 6001


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def long_molecules():
    """two molecules of 65 and 300 atoms with unequal masses: sequential sums longer than a wave, a last chunk of one atom and one of 44"""
    _, _, opts = util.load_fixture("ion64_es")
    rng = np.random.default_rng(5)
    n, side, a = 365, 8, 3.9
    grid = np.array([(i, j, k) for i in range(side) for j in range(side) for k in range(side)], dtype=np.float64)[:n]
    pos = (grid - (side - 1) / 2.0) * a + rng.uniform(-0.2, 0.2, size=(n, 3))
    atoms = {"pos": pos, "charge": np.where(np.arange(n) % 2 == 0, 0.1, -0.1) * (np.arange(n) < 364),
             "polarizability": np.zeros(n), "epsilon": np.full(n, 50.0), "sigma": np.full(n, 3.0),
             "mol_id": np.where(np.arange(n) < 65, 0, 1).astype(np.int32), "frozen": np.zeros(n, dtype=np.int32),
             "mass": 1.0 + (np.arange(n) % 7) * 3.3}
    return atoms, np.eye(3) * side * a, opts


def slab_nonpolar(tmp_path_factory):
    atoms, basis, opts = util.load_generated("slab1025_planted", tmp_path_factory.mktemp("slab"))
    return atoms, basis, dict(opts, polarization=0, polar_iterative=0, polar_ewald=0, polar_gs=0)


@pytest.fixture(scope="module")
def boxes(tmp_path_factory):
    out = {name: util.load_fixture(name) for name in ("ion64_es", "water64_polar", "ion216_triclinic")}
    out["long_molecules"] = long_molecules()
    out["slab1025"] = slab_nonpolar(tmp_path_factory)
    return out


MOVE_BOXES = ["ion64_es", "water64_polar", "ion216_triclinic", "long_molecules"]


# ---- 1. bits of the move ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MOVE_BOXES)
def test_bits_of_the_move(boxes, name):
    atoms, basis, opts = boxes[name]
    S = energy.System(atoms, basis, opts)
    try:
        S.energy()
        cur_atoms, cur_basis = {k: np.array(v) for k, v in atoms.items()}, np.array(basis, dtype=np.float64)
        for s in SCALES:
            S.trial_volume_energy(s)
            st = S.trial_volume_state()
            pos, b = host_scale(cur_atoms, cur_basis, s)
            R, vol, cut = energy.pbc_compute(b)
            assert np.array_equal(bits(st["basis"]), bits(b)), (name, s)
            assert np.array_equal(bits(st["reciprocal"]), bits(R)), (name, s)
            assert bits(st["volume"]) == bits(vol) and bits(st["cutoff"]) == bits(cut), (name, s)
            assert np.array_equal(bits(st["pos"]), bits(pos)), (name, s, "host positions")
            assert np.array_equal(bits(S.device_positions()), bits(pos)), (name, s, "device positions")
            S.accept()  # the next scale compounds on this one
            assert np.array_equal(bits(S.device_positions()), bits(pos)) and np.array_equal(bits(S.atoms["pos"]), bits(pos)), (name, s)
            assert np.array_equal(bits(S.basis), bits(b))
            cur_atoms["pos"], cur_basis = pos, b
            # the centres of mass of the new positions, by the library's own restatement of update_COM
            com = S.update_com()[0]
            for m, (i0, i1) in enumerate(util.molecules(cur_atoms)):
                mm, cm = 0.0, [0.0, 0.0, 0.0]
                for i in range(i0, i1):
                    mm += float(cur_atoms["mass"][i])
                    for p in range(3):
                        cm[p] += float(cur_atoms["mass"][i]) * float(pos[i, p])
                assert np.array_equal(bits(com[m]), bits(np.array([c / mm for c in cm]))), (name, s, m)
        assert S.volume_trial_counts() == {"evaluated": 3, "accepted": 3, "rejected": 0, "reject_evaluations": 0}
    finally:
        S.close()


# ---- 2. energy parity -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("name", MOVE_BOXES)
def test_energy_against_oracle_and_fresh_context(boxes, name, s):
    atoms, basis, opts = boxes[name]
    S = energy.System(atoms, basis, opts)
    try:
        S.energy()
        S.trial_volume_energy(s)
        assert S.last_trial_was_full()
        pos, b = host_scale(atoms, basis, s)
        ref = util.check_trial_against_oracle(S.trial_observables, atoms, b, opts, pos, label=f"{name} s={s}")
        assert np.isfinite(ref["energy"])
        util.check_trial_against_fresh(S, atoms, b, opts, pos, label=f"{name} s={s}")
        S.reject()
    finally:
        S.close()


@pytest.mark.parametrize("name", TERM_FIXTURES + ["ion64_es+autoreject"])
def test_energy_with_each_further_term(tmp_path, name):
    """every term a full evaluation carries follows the trial cell: against a fresh context on the host-scaled configuration"""
    if name == "ion64_es+autoreject":
        atoms, basis, opts = util.load_fixture("ion64_es")
        opts = dict(opts, cavity_autoreject_absolute=1, cavity_autoreject_scale=0.9)
    elif name in util.SMALL:
        atoms, basis, opts = util.load_fixture(name)
    else:
        atoms, basis, opts = util.load_generated(name, tmp_path)
    S = energy.System(atoms, basis, opts)
    try:
        S.energy()
        for s in SCALES[:2]:
            S.trial_volume_energy(s)
            pos, b = host_scale(atoms, basis, s)
            F = energy.System(util.with_positions(atoms, pos), b, opts)
            try:
                F.energy()
                keys = util.TRIAL_KEYS + ["three_body_energy", "lrc_pair", "lrc_self", "es_self"]
                bad = util.component_errors(S.trial_observables, F.observables, keys, 1e-11)
                assert not bad, f"{name} s={s}: " + "; ".join(bad)
                for k in util.COUNT_KEYS + ["n_es_in_cutoff", "polar_iterations"]:
                    assert S.trial_observables[k] == F.observables[k], (name, s, k)
                if name == "ion64_es+autoreject":
                    assert S.cavity_autoreject_info()["n_absolute"] == F.cavity_autoreject_info()["n_absolute"]
            finally:
                F.close()
            S.reject()
    finally:
        S.close()


# ---- 3. reject leaves nothing behind ------------------------------------------------------------------------------------------------------------
def far_point(atoms, basis, rng):
    while True:
        frac = 0.5 - rng.random(3)
        d = (atoms["pos"] - frac @ basis) @ np.linalg.inv(basis)
        if np.linalg.norm((d - np.rint(d)) @ basis, axis=1).min() > 2.5:
            return frac @ basis


@pytest.mark.parametrize("name", ["ion64_es", "slab1025", "ion216_triclinic"])
def test_reject_leaves_nothing_behind(boxes, name):
    atoms, basis, opts = boxes[name]
    opts = util.nonpolar(opts)
    basis = np.asarray(basis, dtype=np.float64)
    rng = np.random.default_rng(3)
    i0, i1 = util.molecules(atoms)[len(util.molecules(atoms)) // 2]
    new = util.moved(atoms, i0, i1 - i0, seed=7)
    a0, a1 = util.molecules(atoms)[0]
    mol = {k: np.array(v[a0:a1]) for k, v in atoms.items()}
    mol["pos"] = mol["pos"] - mol["pos"].mean(0) + far_point(atoms, basis, rng)
    cands = np.stack([mol["pos"] - mol["pos"].mean(0) + far_point(atoms, basis, rng) for _ in range(3)])
    S = energy.System(atoms, basis, opts)
    try:
        S.energy()
        first = dict(S.observables)

        def probes():
            out = []
            S.trial_energy(i0, new)
            out.append((dict(S.trial_observables), S.last_trial_was_full()))
            S.reject()
            S.trial_insert_energy(S.n, mol)
            out.append((dict(S.trial_observables), S.last_trial_was_full()))
            S.reject()
            out.append(S.insert_candidates(mol, cands))
            return out

        before = probes()
        S.trial_volume_energy(1.04)
        assert S.trial_observables["energy"] != first["energy"]
        S.reject()
        after = probes()
        assert after == before, name  # every field of every result, bit for bit (no NaN in them: == is then bit equality up to signed zeros)
        assert before[0][1] is False and before[1][1] is False
        assert S.volume_trial_counts() == {"evaluated": 1, "accepted": 0, "rejected": 1, "reject_evaluations": 0}
        S.energy()
        assert dict(S.observables) == first, name
        assert np.array_equal(bits(S.device_positions()), bits(atoms["pos"]))
    finally:
        S.close()


def test_reject_on_a_polarizable_box(boxes):
    atoms, basis, opts = boxes["water64_polar"]
    S = energy.System(atoms, basis, opts)
    try:
        S.energy()
        first = dict(S.observables)
        S.trial_volume_energy(1.04)
        S.reject()
        i0, i1 = util.molecules(atoms)[5]
        new = util.moved(atoms, i0, i1 - i0, seed=9, sigma=0.1)
        S.trial_energy(i0, new)  # (the existing rule of a rejected full trial: this one evaluates in full)
        pos = np.array(atoms["pos"])
        pos[i0:i1] = new
        util.check_trial_against_fresh(S, atoms, basis, opts, pos, label="water64_polar after a rejected volume trial")
        S.reject()
        S.energy()
        bad = util.component_errors(S.observables, first, util.TRIAL_KEYS, 1e-11)
        assert not bad, bad
        assert S.volume_trial_counts()["reject_evaluations"] == 0
    finally:
        S.close()


# ---- 4. accept carries on -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ion64_es", "ion216_triclinic"])
def test_accept_carries_on(boxes, name):
    atoms, basis, opts = boxes[name]
    opts = dict(util.nonpolar(opts), cavity_bias=1, cavity_grid_size=4, cavity_radius=2.0)
    basis = np.asarray(basis, dtype=np.float64)
    S = energy.System(atoms, basis, opts)
    try:
        S.energy()
        S.cavity_update()
        S.cavity_point(0)
        S.trial_volume_energy(0.97)
        accepted = dict(S.trial_observables)
        S.accept()
        with pytest.raises(energy.MpmcError) as e:  # a stale grid, exactly as after mpmc_set_box
            S.cavity_point(0)
        assert e.value.code == ERR_ARG
        S.cavity_update()
        S.cavity_point(0)
        pos, b = host_scale(atoms, basis, 0.97)
        cur = util.with_positions(atoms, pos)
        # a displacement and an insertion are deltas on the new cell
        i0, i1 = util.molecules(atoms)[3]
        new = util.moved(cur, i0, i1 - i0, seed=11)
        S.trial_energy(i0, new)
        assert not S.last_trial_was_full()
        moved_pos = pos.copy()
        moved_pos[i0:i1] = new
        util.check_trial_against_fresh(S, cur, b, opts, moved_pos, label=f"{name}: displacement after an accepted volume trial")
        S.reject()
        a0, a1 = util.molecules(atoms)[0]
        mol = {k: np.array(v[a0:a1]) for k, v in cur.items()}
        mol["pos"] = mol["pos"] - mol["pos"].mean(0) + far_point(cur, b, np.random.default_rng(4))
        S.trial_insert_energy(S.n, mol)
        assert not S.last_trial_was_full()
        grown = {k: np.concatenate([cur[k], mol[k]]) for k in cur}
        grown["mol_id"][-(a1 - a0):] = int(cur["mol_id"].max()) + 1
        F = energy.System(grown, b, opts)
        F.energy()
        bad = util.component_errors(S.trial_observables, F.observables, util.TRIAL_KEYS + ["lrc_pair", "lrc_self", "es_self"], 1e-11)
        F.close()
        assert not bad, bad
        S.reject()
        S.energy()
        bad = util.component_errors(S.observables, accepted, util.TRIAL_KEYS, 1e-11)
        assert not bad, bad
        S.set_box(b)  # the scaled basis is the context's own: a no-op that keeps the accepted totals
        S.trial_energy(i0, new)
        assert not S.last_trial_was_full()
        S.reject()
    finally:
        S.close()


# ---- 5. no-op and refusals ----------------------------------------------------------------------------------------------------------------------
def test_noop_and_refusals(boxes):
    atoms, basis, opts = boxes["ion64_es"]
    L = energy.lib()
    S = energy.System(atoms, basis, opts)
    try:
        def refused(code, scale=1.04):
            rc = L.mpmc_trial_volume_begin(S.handle, float(scale))
            assert rc == code and len(L.mpmc_last_error(S.handle)) > 0, (rc, code, L.mpmc_last_error(S.handle))

        refused(ERR_ARG)  # no accepted configuration
        e0 = S.energy()
        waits = util.debug_counts(S, "mpmc_debug_wait_counters", 4)
        assert S.trial_volume_energy(1.0) == e0 and not S.last_trial_was_full()  # launches nothing
        st = S.trial_volume_state()
        assert np.array_equal(bits(st["pos"]), bits(atoms["pos"])) and np.array_equal(bits(st["basis"]), bits(basis))
        S.accept()
        assert util.debug_counts(S, "mpmc_debug_wait_counters", 4) == waits
        assert S.volume_trial_counts()["evaluated"] == 0
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            refused(ERR_INVALID_DATUM, bad)
        i0, i1 = util.molecules(atoms)[0]
        S.trial_energy(i0, util.moved(atoms, i0, i1 - i0, seed=1))
        refused(ERR_ARG)  # a trial already open
        S.reject()
        assert S.trial_volume_energy(1.04) != e0  # the context is still usable
        S.reject()
        # a caller-supplied cutoff: no rule for scaling an override
        b = np.ascontiguousarray(basis, dtype=np.float64).reshape(9)
        assert L.mpmc_set_box(S.handle, b.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), None, 0.0, 5.0) == 0
        S.energy()
        refused(ERR_ARG)
        S.set_box(basis)
        S.energy()
        S.trial_volume_energy(0.97)
        S.reject()
    finally:
        S.close()
    no_mass = {k: v for k, v in atoms.items() if k != "mass"}
    S = energy.System(no_mass, basis, opts)
    try:
        S.energy()
        rc = L.mpmc_trial_volume_begin(S.handle, 1.04)
        assert rc == ERR_ARG and b"without masses" in L.mpmc_last_error(S.handle)
        S.energy()
    finally:
        S.close()


# ---- 6. asynchronous pairs ----------------------------------------------------------------------------------------------------------------------
def test_async_pair_returns_the_blocking_bits(boxes):
    L = energy.lib()
    L.mpmc_trial_energy_async.argtypes = [ctypes.c_void_p]
    L.mpmc_trial_energy_wait.argtypes = [ctypes.c_void_p, ctypes.POINTER(energy.Result)]
    made = [energy.System(*boxes[name]) for name in ("ion64_es", "ion216_triclinic")]
    try:
        blocking = []
        for S, s in zip(made, (1.04, 0.97)):
            S.energy()
            S.trial_volume_energy(s)
            blocking.append(dict(S.trial_observables))
            S.reject()
        for S, s in zip(made, (1.04, 0.97)):
            assert L.mpmc_trial_volume_begin(S.handle, s) == 0
            assert L.mpmc_trial_energy_async(S.handle) == 0
        for S, want in zip(made, blocking):
            r = energy.Result()
            assert L.mpmc_trial_energy_wait(S.handle, ctypes.byref(r)) == 0
            assert r.as_dict() == want
            assert L.mpmc_trial_reject(S.handle) == 0
    finally:
        for S in made:
            S.close()
