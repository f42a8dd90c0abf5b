"""GPU (MI355X): what a volume trial (mpmc_trial_volume_begin, csrc/trial.cpp) leaves for the calls behind it.  tests/test_gpu_volume_trial.py
holds the move itself; this file holds the states the move passes through to what follows them.  Inputs: tests/volume_trial_cases.py; what
makes them mean something is asserted on the CPU by tests/test_volume_trial_preconditions.py.

  1 reject, per term     every term fixture, every polarizable configuration and the solves without a delta path: probes (a displacement
                         trial, an insertion trial and insert_candidates where the context allows them, dipoles()) before and after a
                         rejected trial at 1.04.  Non-polarizable: every field of every probe and energy() bit for bit, the trials still
                         deltas, the device's positions the original bits.  Polarizable: the first displacement behind the reject is full
                         (the documented rule) and agrees with a fresh context, a second one accepted, the next a delta again, the
                         molecule moved back, energy() the first one's to 1e-11 and the dipoles at the ragged ladder's bounds
  2 accept, polarizable  0.97 accepted with no energy() behind it: dipoles() against a fresh context of the host-scaled configuration, a
                         displacement delta against a fresh context and the oracle, 1.04 on top against a fresh context
  3 class flip           the slab at FLIP_SCALE, non-polarizable and jac_compact, in list order (where the scale changes the class counts:
                         the tile stats of the accepted and of the trial cell are the restated ones) and under the spatial order
  4 list edits           edge190 and sorted129: insertion accepted, volume trial accepted, removal accepted, volume trial rejected,
                         insertion delta, energy(), every step against a fresh context, the move's bits on the grown list, exchange trials
                         on the delta path, uploads as a context without the volume trials makes them
  5 drift                DRIFT_SCALE accepted, then every atom handed over again with 0.01 A of noise: no re-sort
  6 frozen               ion216_frozen and ion216_framework: frozen molecules are scaled too
  7 the closing calls    mpmc_set_box, mpmc_set_options, mpmc_set_atoms and mpmc_update_positions behind an evaluated volume trial and
                         behind one enqueued and never waited for
  8 energy() inside      an evaluation asked for while an evaluated volume trial is open is refused and leaves the trial open

Same-context comparisons are bit for bit, fresh-context ones use util.check_trial_against_fresh at 1e-11, oracle ones
util.check_trial_against_oracle at util.REL_TOL, counts are exact.
"""
import contextlib
import ctypes

import numpy as np
import pytest

import util
import polar_ragged_boxes as B
import polar_trial_cases as C
import test_gpu_polar_ragged_ladder as L
import volume_trial_cases as V
from mpmcxx_amd import energy
from volume_trial_cases import bits

pytestmark = pytest.mark.gpu

ERR_ARG = -3
FRESH_REL = 1e-11
TOTAL_KEYS = util.TRIAL_KEYS + ["lrc_pair", "lrc_self", "es_self"]


@pytest.fixture(scope="module", autouse=True)
def _need_device():
    if energy.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests need an MI355X")


@contextlib.contextmanager
def system(atoms, basis, opts, sort=1, pairs=(), max_atoms=None):
    """a context of its own, closed on the way out; sort == 0: in list order (spatial_sort is read when the atoms are uploaded)"""
    energy.configure("spatial_sort", sort)
    try:
        S = energy.System(atoms, basis, opts, max_atoms=max_atoms)
    finally:
        energy.configure("spatial_sort", 1)
    try:
        for key, value in pairs:
            S.configure(key, value)
        yield S
    finally:
        S.close()


def fresh_totals(atoms, basis, opts, sort=1):
    with system(atoms, basis, opts, sort) as F:
        F.energy()
        return dict(F.observables), (F.dipoles() if V.is_polarizable(opts) else None)


def agree(got, ref, label, keys=TOTAL_KEYS, rel=FRESH_REL):
    bad = util.component_errors(got, ref, keys, rel)
    assert not bad, f"{label} (rel {rel}): " + "; ".join(bad)
    for k in util.COUNT_KEYS + ["n_es_in_cutoff", "polar_iterations"]:
        assert got[k] == ref[k], (label, k, got[k], ref[k])


def dipoles_agree(got, want, opts, label):
    """(mu, ef_static, ef_induced) against another context's: the largest difference within the ragged ladder's bound of the solve's family
    times the largest component"""
    fam = "wolf" if opts.get("polar_wolf") else ("pef" if opts.get("polar_ewald_full") else "relax")
    rel = L.BOUNDS[fam][1]
    for k, g, w in zip(("mu", "ef_static", "ef_induced"), got, want):
        top, d = float(np.abs(w).max()), float(np.abs(np.asarray(g) - np.asarray(w)).max())
        assert d <= rel[k] * top, (label, k, d, top)


def trial_displacement(S, first, new):
    S.trial_energy(first, new)
    return dict(S.trial_observables), S.last_trial_was_full()


def reject_counts(S, **want):
    got = S.volume_trial_counts()
    assert got == dict({"evaluated": 0, "accepted": 0, "rejected": 0, "reject_evaluations": 0}, **want), got


# ---- 1. reject, per term ------------------------------------------------------------------------------------------------------------------------
def reject_case(case):
    """(atoms, basis, options, configure pairs) of a case of test 1"""
    if isinstance(case, tuple):
        return V.polar_box(*case) + (C.CONFIGS[case[1]][1],)
    if case in V.EXTRA_SOLVES:
        return V.extra_solve(case) + ((),)
    return V.fixture(case) + ((),)


REJECT_CASES = V.TERM_FIXTURES + ["gs_ranked"] + V.POLAR_CASES


@pytest.mark.parametrize("case", REJECT_CASES, ids=[c if isinstance(c, str) else f"{c[0]}-{c[1]}" for c in REJECT_CASES])
def test_reject_per_term(case):
    atoms, basis, opts, pairs = reject_case(case)
    pos0 = np.array(atoms["pos"], dtype=np.float64)
    first, new = V.displacement(atoms, basis)
    with system(atoms, basis, opts, pairs=pairs) as S:
        S.energy()
        start = dict(S.observables)
        if not V.is_polarizable(opts):
            mol = cands = None
            if V.insertion_allowed(opts):
                a0, a1 = util.molecules(atoms)[0]
                mol = {k: np.array(v[a0:a1]) for k, v in atoms.items()}
                shape = mol["pos"] - mol["pos"].mean(0)
                points = [V.far_point(atoms, basis, V.REJECT_SCALE, seed=100 + k) for k in range(4)]
                mol["pos"] = shape + points[0]
                cands = np.stack([shape + p for p in points[1:]])

            def probes():
                out = [trial_displacement(S, first, new)]
                S.reject()
                if mol is not None:
                    S.trial_insert_energy(S.n, mol)
                    out.append((dict(S.trial_observables), S.last_trial_was_full()))
                    S.reject()
                if V.candidates_allowed(opts):
                    out.append(S.insert_candidates(mol, cands))
                return out

            before = probes()
            assert len(before) == 1 + int(V.insertion_allowed(opts)) + int(V.candidates_allowed(opts)), (case, len(before))
            S.trial_volume_energy(V.REJECT_SCALE)
            assert S.trial_observables["energy"] != start["energy"]
            S.reject()
            after = probes()
            assert after == before, case  # every field of every result, bit for bit
            assert before[0][1] is False, case  # the displacement is a delta before and behind the rejected trial
            reject_counts(S, evaluated=1, rejected=1)
            S.energy()
            assert dict(S.observables) == start, case
            assert np.array_equal(bits(S.device_positions()), bits(pos0)), case
            return
        # polarizable
        delta = V.has_delta(opts)
        mu0 = S.dipoles()
        before, full = trial_displacement(S, first, new)
        assert full == (not delta), (case, full)
        S.reject()
        S.trial_volume_energy(V.REJECT_SCALE)
        S.reject()
        moved = C.applied(pos0, first, new)
        got, full = trial_displacement(S, first, new)
        assert full, f"{case}: the first displacement behind a rejected volume trial is a delta on the rejected cell's field"
        util.check_trial_against_fresh(S, atoms, basis, opts, moved, label=f"{case}: displacement behind the rejected volume trial")
        agree(got, before, f"{case}: the displacement behind the reject against the one before the trial", keys=util.TRIAL_KEYS)
        S.reject()
        # a second molecule, accepted (still in full); the next displacement is a delta on it
        second, new2 = V.displacement(atoms, basis, where=0.25, seed=17)
        assert second != first
        got, full = trial_displacement(S, second, new2)
        assert full, case
        there = C.applied(pos0, second, new2)
        util.check_trial_against_fresh(S, atoms, basis, opts, there, label=f"{case}: second displacement")
        S.accept()
        got, full = trial_displacement(S, first, new)
        assert full == (not delta), (case, full)
        util.check_trial_against_fresh(S, atoms, basis, opts, C.applied(there, first, new), label=f"{case}: displacement behind an accepted one")
        S.reject()
        # the second molecule back where it stood: the first configuration again
        got, full = trial_displacement(S, second, pos0[second:second + len(new2)])
        assert full == (not delta), (case, full)
        S.accept()
        S.energy()
        agree(S.observables, start, f"{case}: energy() against the first one", keys=util.TRIAL_KEYS)
        dipoles_agree(S.dipoles(), mu0, opts, f"{case}: dipoles against the first ones")
        reject_counts(S, evaluated=1, rejected=1)


# ---- 2. accept on polarizable boxes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,cfg", V.POLAR_CASES)
def test_accept_on_a_polarizable_box(key, cfg):
    atoms, basis, opts = V.polar_box(key, cfg)
    with system(atoms, basis, opts, pairs=C.CONFIGS[cfg][1]) as S:
        S.energy()
        S.trial_volume_energy(V.SHRINK)
        small, sb = V.scaled(atoms, basis, V.SHRINK)
        want = util.check_trial_against_fresh(S, atoms, sb, opts, small["pos"], label=f"{key} {cfg}: volume trial {V.SHRINK}")
        S.accept()  # (no energy() from here on)
        dipoles_agree(S.dipoles(), want, opts, f"{key} {cfg}: dipoles behind the accepted volume trial")
        first, new = V.displacement(small, sb)
        got, full = trial_displacement(S, first, new)
        assert not full, f"{key} {cfg}: the displacement behind an accepted volume trial was evaluated in full"
        moved = C.applied(small["pos"], first, new)
        util.check_trial_against_fresh(S, atoms, sb, opts, moved, label=f"{key} {cfg}: displacement behind the accepted volume trial")
        if cfg in C.ORACLE_KNOWS:
            util.check_trial_against_oracle(got, atoms, sb, V.reference_options(key, cfg), moved, label=f"{key} {cfg}: displacement behind the accepted volume trial")
        S.reject()
        S.trial_volume_energy(V.GROW)
        big, bb = V.scaled(small, sb, V.GROW)
        util.check_trial_against_fresh(S, atoms, bb, opts, big["pos"], label=f"{key} {cfg}: volume trial {V.GROW} on top")
        S.reject()
        reject_counts(S, evaluated=2, accepted=1, rejected=1)


# ---- 3. class flip ------------------------------------------------------------------------------------------------------------------------------
_slab_oracle = {}


def far_beyond(st):
    return st["thole_far"], st["beyond_cutoff"]


@pytest.mark.parametrize("sort", [0, 1])
@pytest.mark.parametrize("cfg", ["nonpolar", "jac_compact"])
def test_class_flip(cfg, sort):
    """in list order FLIP_SCALE takes tile pairs out of the far class (restated counts, asserted where the context classifies for a solve);
    under the spatial order no scale can, and the same steps run beside it"""
    atoms, basis, _ = B.box(V.SLAB)
    polar = cfg != "nonpolar"
    opts = C.options(V.SLAB, cfg) if polar else util.nonpolar(B.box(V.SLAB)[2])
    s, start, flipped = V.flip_search()
    small, sb = V.scaled(atoms, basis, s)
    first, new = C.JUMPER, C.jitter(atoms["pos"], C.JUMPER, 47)
    label = f"{V.SLAB} {cfg} sort {sort}"
    with system(atoms, basis, opts, sort) as S:
        S.energy()
        st0 = S.tile_stats()
        before, full0 = trial_displacement(S, first, new)
        assert not full0, label
        S.reject()
        S.trial_volume_energy(s)
        st1 = S.tile_stats()
        print(f"\n{label}: tile stats {st0} -> under the volume trial {st1}")
        # the restated counts of this order, of the accepted and of the trial cell.  A context that solves no dipoles classifies no pair as
        # far (k_classify takes the far range from the solve's damping): its far count is 0 and only the beyond-cutoff count is held, which
        # no scale changes
        want0, want1 = start[0 if sort == 0 else 1], flipped[0 if sort == 0 else 1]
        if polar:
            assert far_beyond(st0) == want0 and far_beyond(st1) == want1, (st0, st1, want0, want1)
            assert (want0 != want1) == (sort == 0)
        else:
            assert far_beyond(st0) == (0, want0[1]) and far_beyond(st1) == (0, want1[1]), (st0, st1, want0, want1)
        if cfg not in _slab_oracle:
            _slab_oracle[cfg] = util.oracle_energy(small, sb, {k: v for k, v in opts.items() if k != "solver"})
        ref = _slab_oracle[cfg]
        bad = util.component_errors(S.trial_observables, ref, util.TRIAL_KEYS, util.REL_TOL)
        assert not bad, f"{label}: volume trial against the oracle: " + "; ".join(bad)
        for k in ("n_lj_in_cutoff", "n_es_in_cutoff", "polar_iterations"):
            assert S.trial_observables[k] == ref[k], (label, k)
        util.check_trial_against_fresh(S, atoms, sb, opts, small["pos"], label=f"{label}: volume trial")
        S.reject()
        after, full = trial_displacement(S, first, new)
        if polar:
            assert full, label
            agree(after, before, f"{label}: the jumper's displacement behind the reject against the one before", keys=util.TRIAL_KEYS)
            util.check_trial_against_fresh(S, atoms, basis, opts, C.applied(atoms["pos"], first, new), label=f"{label}: displacement behind the reject")
        else:
            assert (after, full) == (before, False), label  # a delta with the bits of before the trial
        S.reject()
        reject_counts(S, evaluated=1, rejected=1)
    with system(atoms, basis, opts, sort) as S:
        S.energy()
        S.trial_volume_energy(s)
        S.accept()
        moved = C.jitter(small["pos"], C.JUMPER, 47)
        got, full = trial_displacement(S, first, moved)
        assert not full, label
        util.check_trial_against_fresh(S, atoms, sb, opts, C.applied(small["pos"], first, moved), label=f"{label}: displacement behind the accept")
        S.reject()


# ---- 4. list edits ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(V.LATTICE))
def test_list_edits_between_volume_trials(name):
    atoms, basis, opts, vacant = V.lattice_box(name)
    hist = {label: (a, b) for label, a, b in V.list_edit_history(name)}
    n = len(atoms["pos"])

    def against_fresh(obs, label):
        a, b = hist[label]
        agree(obs, fresh_totals(a, b, opts)[0], f"{name}: {label} against a fresh context")

    room = n + util.ladder_constants()["kTile"]  # (capacity for the grown list: no growth rebuild in the chain)
    with system(atoms, basis, opts, max_atoms=room) as S, system(atoms, basis, opts, max_atoms=room) as P:
        S.energy()
        # 1. an insertion, accepted
        S.trial_insert_energy(S.n, V.new_molecule(atoms, vacant[0]))
        assert not S.last_trial_was_full()
        against_fresh(S.trial_observables, "grown")
        S.accept()
        assert S.n == n + 3
        # 2. a volume trial of the grown list: the move's bits, then accepted
        S.trial_volume_energy(V.GROW)
        big, bb = hist["scaled"]
        assert np.array_equal(bits(S.trial_volume_state()["pos"]), bits(big["pos"])), (name, "host positions of the grown list")
        assert np.array_equal(bits(S.device_positions()), bits(big["pos"])), (name, "device positions of the grown list")
        assert np.array_equal(bits(S.trial_volume_state()["basis"]), bits(bb))
        against_fresh(S.trial_observables, "scaled")
        S.accept()
        assert np.array_equal(bits(S.atoms["pos"]), bits(big["pos"])) and np.array_equal(bits(S.device_positions()), bits(big["pos"]))
        # 3. the removal of another molecule, accepted
        r0, r1 = util.molecules(big)[V.REMOVED]
        S.trial_remove_energy(r0, r1 - r0)
        assert not S.last_trial_was_full()
        against_fresh(S.trial_observables, "fewer")
        S.accept()
        assert S.n == n
        # 4. a volume trial, rejected
        S.trial_volume_energy(V.SHRINK)
        shrunk, sb = hist["shrunk"]
        assert np.array_equal(bits(S.device_positions()), bits(shrunk["pos"])), (name, "device positions behind the removal")
        against_fresh(S.trial_observables, "shrunk")
        S.reject()
        assert np.array_equal(bits(S.device_positions()), bits(hist["fewer"][0]["pos"]))
        # 5. an insertion delta
        S.trial_insert_energy(S.n, V.new_molecule(hist["fewer"][0], vacant[1] * V.GROW))
        assert not S.last_trial_was_full()
        against_fresh(S.trial_observables, "again")
        S.reject()
        # 6. energy()
        S.energy()
        against_fresh(S.observables, "fewer")
        assert util.exchange_counts(S)[:2] == (3, 0), util.exchange_counts(S)
        reject_counts(S, evaluated=2, accepted=1, rejected=1)
        # the uploads of the same list edits without the volume trials
        P.energy()
        P.trial_insert_energy(P.n, V.new_molecule(atoms, vacant[0]))
        P.accept()
        r0, r1 = util.molecules(hist["grown"][0])[V.REMOVED]
        P.trial_remove_energy(r0, r1 - r0)
        P.accept()
        P.trial_insert_energy(P.n, V.new_molecule(V.without(hist["grown"][0], r0, r1), vacant[1]))
        P.reject()
        P.energy()
        assert util.exchange_counts(P)[:2] == (3, 0)
        print(f"\n{name}: uploads (carried, sorted) {util.upload_counts(S)} with the volume trials, {util.upload_counts(P)} without")
        assert util.upload_counts(S) == util.upload_counts(P), (util.upload_counts(S), util.upload_counts(P))


# ---- 5. drift -----------------------------------------------------------------------------------------------------------------------------------
def test_accepted_scale_moves_the_drift_reference():
    atoms, basis, opts = V.nonpolar_rung(V.DRIFT_RUNG)
    big, bb = V.scaled(atoms, basis, V.DRIFT_SCALE)
    jitter = np.random.default_rng(8).uniform(-0.01, 0.01, size=big["pos"].shape)
    with system(atoms, basis, opts) as S:
        S.energy()
        assert util.upload_counts(S)[1] == 1  # sorted once
        S.trial_volume_energy(V.DRIFT_SCALE)
        S.accept()
        S.update_positions(0, big["pos"] + jitter)  # every atom, 0.01 A from where the accepted move left it
        S.energy()
        assert util.upload_counts(S)[1] == 1, f"a bulk update behind an accepted volume move sorted again: {util.upload_counts(S)}"
        agree(S.observables, fresh_totals(util.with_positions(atoms, big["pos"] + jitter), bb, opts)[0], "jittered positions in the scaled cell")
        # control: one molecule 2.5 A further is past kResortDrift, and the count moves
        a, b = util.molecules(atoms)[len(util.molecules(atoms)) // 2]
        far = big["pos"] + jitter
        far[a:b] += np.array([2.5, 0.0, 0.0])
        S.update_positions(0, far)
        S.energy()
        assert util.upload_counts(S)[1] == 2, util.upload_counts(S)


# ---- 6. frozen ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", V.FROZEN)
def test_frozen_molecules_are_scaled_too(name):
    atoms, basis, opts = V.fixture(name)
    assert np.any(atoms["frozen"])
    with system(atoms, basis, opts) as S:
        S.energy()
        n_frozen = S.observables["n_frozen"]
        assert n_frozen > 0
        for s in (V.SHRINK, V.GROW):
            S.trial_volume_energy(s)
            sa, sb = V.scaled(atoms, basis, s)
            st = S.trial_volume_state()
            assert np.array_equal(bits(st["pos"]), bits(sa["pos"])) and np.array_equal(bits(S.device_positions()), bits(sa["pos"])), (name, s)
            assert np.any(sa["pos"][np.asarray(atoms["frozen"]) != 0] != atoms["pos"][np.asarray(atoms["frozen"]) != 0])
            ref = util.check_trial_against_oracle(S.trial_observables, atoms, sb, opts, sa["pos"], label=f"{name} s={s}")
            for k in util.COUNT_KEYS:
                assert S.trial_observables[k] == ref[k], (name, s, k, S.trial_observables[k], ref[k])
            assert S.trial_observables["n_frozen"] == n_frozen
            util.check_trial_against_fresh(S, atoms, sb, opts, sa["pos"], label=f"{name} s={s}")
            if s == V.SHRINK:
                S.reject()
        S.accept()
        first, new = V.displacement(sa, sb)
        got, full = trial_displacement(S, first, new)
        assert not full, name
        util.check_trial_against_fresh(S, atoms, sb, opts, C.applied(sa["pos"], first, new), label=f"{name}: displacement behind the accept")
        assert got["n_frozen"] == n_frozen
        for k in util.COUNT_KEYS:
            if k != "n_lj_in_cutoff":
                assert got[k] == S.observables[k], (name, k)
        S.reject()
        reject_counts(S, evaluated=2, accepted=1, rejected=1)


# ---- 7. the four closing calls ------------------------------------------------------------------------------------------------------------------
def _async_api():
    lib = energy.lib()
    lib.mpmc_trial_energy_async.argtypes = [ctypes.c_void_p]
    return lib


@pytest.mark.parametrize("state", ["evaluated", "enqueued"])
@pytest.mark.parametrize("call", ["set_box", "set_options", "set_atoms", "update_positions", "set_box_same", "set_options_same"])
@pytest.mark.parametrize("name", ["ion64_es", "water64_polar"])
def test_closing_calls(name, call, state):
    lib = _async_api()
    atoms, basis, opts = V.fixture(name)
    atoms = {k: np.array(v) for k, v in atoms.items()}
    first, new = V.displacement(atoms, basis, sigma=0.1)
    with system(atoms, basis, opts) as S:
        S.energy()
        if state == "evaluated":
            S.trial_volume_energy(V.REJECT_SCALE)
        else:
            assert lib.mpmc_trial_volume_begin(S.handle, V.REJECT_SCALE) == 0
            assert lib.mpmc_trial_energy_async(S.handle) == 0  # ... and never waited for
        held = (atoms, basis, opts)  # what the caller holds behind the call
        if call == "set_box":
            other = basis * np.array([1.01, 1.02, 1.03])[:, None]
            S.set_box(other)  # (raises unless the call returns 0)
            held = (atoms, other, opts)
        elif call == "set_options":
            changed = dict(opts, ewald_kmax=5 if int(opts["ewald_kmax"]) != 5 else 6)
            S.set_options(changed)
            held = (atoms, basis, changed)
        elif call == "set_atoms":
            S.set_atoms(atoms)
        elif call == "set_box_same":  # the accepted cell again: a no-op without a trial, the end of the trial with one
            S.set_box(basis)
        elif call == "set_options_same":
            S.set_options(opts)
        else:
            S.update_positions(first, new)
            want = C.applied(atoms["pos"], first, new)
            assert np.array_equal(bits(S.device_positions()), bits(want)), "the accepted positions with the one molecule changed"
            held = (util.with_positions(atoms, want), basis, opts)
        assert S.volume_trial_counts()["accepted"] == 0
        with pytest.raises(energy.MpmcError, match="no trial move is open") as e:
            S.reject()
        assert e.value.code == ERR_ARG
        if call.endswith("_same"):
            assert np.array_equal(bits(S.device_positions()), bits(atoms["pos"])), "the accepted positions are resident again"
        S.energy()  # (raises unless it returns 0)
        agree(S.observables, fresh_totals(*held)[0], f"{name} {call} behind an {state} volume trial: energy()")
        a, b, o = held
        f2, n2 = V.displacement(a, b, where=0.25, seed=23, sigma=0.1)
        S.trial_energy(f2, n2)
        util.check_trial_against_fresh(S, a, b, o, C.applied(a["pos"], f2, n2), label=f"{name} {call} behind an {state} volume trial: displacement")
        S.reject()
        assert S.volume_trial_counts()["accepted"] == 0


def test_a_closing_call_that_fails_still_closes_the_trial():
    """mpmc_update_positions closes the trial and then refuses a non-finite position: the accepted configuration and its totals are back,
    and the polarizable field and store on the device are the abandoned cell's, so the next displacement evaluates in full, as behind a reject"""
    atoms, basis, opts = V.fixture("water64_polar")
    first, new = V.displacement(atoms, basis, sigma=0.1)
    with system(atoms, basis, opts) as S:
        S.energy()
        before, full = trial_displacement(S, first, new)
        assert not full
        S.reject()
        S.trial_volume_energy(V.REJECT_SCALE)
        with pytest.raises(energy.MpmcError, match="non-finite position"):
            S.update_positions(first, np.full_like(new, np.nan))
        with pytest.raises(energy.MpmcError, match="no trial move is open"):
            S.reject()
        assert np.array_equal(bits(S.device_positions()), bits(atoms["pos"]))
        got, full = trial_displacement(S, first, new)
        assert full, "a delta on the abandoned cell's field"
        util.check_trial_against_fresh(S, atoms, basis, opts, C.applied(atoms["pos"], first, new), label="displacement behind a failed closing call")
        agree(got, before, "the displacement behind the failed call against the one before the trial", keys=util.TRIAL_KEYS)
        S.reject()


# ---- 8. an evaluation asked for inside an open volume trial ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["energy", "lj", "coulombic"])
def test_evaluation_inside_an_open_volume_trial(which):
    """The rule (include/mpmc_energy.h): the evaluation entry points are refused with MPMC_ERR_ARG while a volume trial is open, and the
    trial stays open.  Whatever the call answers, the accepted totals behind the trial are the first evaluation's: a delta behind the
    reject has the bits of before the trial, with and without an energy() in between."""
    atoms, basis, opts = V.fixture("ion64_es")
    first, new = V.displacement(atoms, basis)
    with system(atoms, basis, opts) as S:
        S.energy()
        start = dict(S.observables)
        before = trial_displacement(S, first, new)
        assert before[1] is False
        S.reject()
        S.trial_volume_energy(V.REJECT_SCALE)
        refused = False
        try:
            getattr(S, which)()
        except energy.MpmcError as e:
            refused = True
            assert e.code == ERR_ARG and "volume trial" in str(e), e
        try:
            S.reject()
        except energy.MpmcError as e:  # (a library that evaluated may have closed the trial; one that refused may not)
            assert not refused and "no trial move is open" in str(e), "a refused evaluation closed the trial"
        after = trial_displacement(S, first, new)  # (in front of any energy(): on the accepted totals as the trial left them)
        S.reject()
        assert after == before, f"{which}() inside an open volume trial changed the base of the next delta"
        S.energy()
        assert dict(S.observables) == start, which
        after = trial_displacement(S, first, new)
        S.reject()
        assert after == before, which
        assert np.array_equal(bits(S.device_positions()), bits(atoms["pos"]))
