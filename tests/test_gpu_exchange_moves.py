"""GPU (MI355X): exchange trials -- insertion and removal of one molecule (mpmc_trial_insert_begin / mpmc_trial_remove_begin).

Every trial is held to a stateless evaluation of the trial composition in a fresh context (1e-11 relative per component) and to the
oracle on the same atom list (1e-9 relative per component), all counts bit-exact (util.check_trial_against_fresh,
util.check_trial_against_oracle); the position-independent terms and counts of the result are compared with the oracle's as well."""
import numpy as np
import pytest

import util
from mpmcxx_amd import energy

pytestmark = pytest.mark.gpu

molecules = util.molecules
nonpolar = util.nonpolar
ERR_ARG, ERR_INVALID_DATUM = -3, 6001  # MPMC_ERR_ARG, MPMC_ERR_INVALID_DATUM
STATIC_COUNTS = ["n_pairs", "n_intra", "n_rd_excluded", "n_es_excluded", "n_frozen"]


def molecule(atoms, a, b, pos=None):
    """atoms [a, b) as an atoms dict of their own (optionally at other positions)"""
    mol = {k: np.array(v[a:b]) for k, v in atoms.items()}
    if pos is not None:
        mol["pos"] = np.array(pos, dtype=np.float64)
    return mol


def inserted(atoms, at, mol):
    new_id = int(np.max(atoms["mol_id"])) + 1
    out = {}
    for k, v in atoms.items():
        piece = np.full(len(mol["pos"]), new_id, dtype=v.dtype) if k == "mol_id" else np.asarray(mol[k], dtype=v.dtype)
        out[k] = np.insert(v, at, piece, axis=0)
    return out


def removed(atoms, a, b):
    return {k: np.delete(v, np.s_[a:b], axis=0) for k, v in atoms.items()}


def count_N(atoms):
    """countN: molecules whose last atom is not frozen"""
    return float(sum(1 for _, b in molecules(atoms) if not atoms["frozen"][b - 1]))


def check_exchange(S, trial_atoms, basis, opts, label, full=False):
    """the open trial of S against a fresh context and the oracle on `trial_atoms`, every field of the result"""
    assert S.last_trial_was_full() == full, label
    obs = S.trial_observables
    util.check_trial_against_fresh(S, trial_atoms, basis, opts, trial_atoms["pos"], rel=1e-11, label=label)
    ref = util.check_trial_against_oracle(obs, trial_atoms, basis, opts, trial_atoms["pos"], label=label)
    for k in STATIC_COUNTS:
        assert obs[k] == ref[k], (label, k, obs[k], ref[k])
    keys = ["lrc_pair", "lrc_self"] + ([] if opts.get("wolf") or opts.get("rd_only") else ["es_self"])
    bad = util.component_errors(obs, ref, keys, util.REL_TOL)
    assert not bad, f"{label}: position-independent terms vs oracle: " + "; ".join(bad)
    assert obs["N"] == count_N(trial_atoms), (label, obs["N"])
    assert obs["NU"] == obs["N"] * obs["energy"], label
    return ref


def random_rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def random_insertion(rng, atoms, basis):
    """a copy of a random molecule, rotated, its centre uniform over fractional coordinates in [-1, 2): wrapped images are exercised"""
    mols = molecules(atoms)
    a, b = mols[rng.integers(len(mols))]
    p = atoms["pos"][a:b]
    centre = p.mean(axis=0)
    rel = (p - centre) @ random_rotation(rng).T if b - a > 1 else p - centre
    new_centre = rng.uniform(-1.0, 2.0, size=3) @ np.asarray(basis).reshape(3, 3)
    bounds = [m[0] for m in mols] + [len(atoms["pos"])]
    return int(bounds[rng.integers(len(bounds))]), molecule(atoms, a, b, rel + new_centre)


@pytest.mark.parametrize("name", ["lj64", "ion64_es", "water64_polar", "ion216_triclinic", "ion216_frozen", "ion216_wolf", "water64_fh2"])
def test_sequence_of_exchange_moves(name):
    from oracle import OracleSystem

    atoms, basis, opts = util.load_fixture(name)
    opts = nonpolar(opts)
    atoms = {k: np.array(v) for k, v in atoms.items()}
    rng = np.random.default_rng(2024)
    S = energy.System(atoms, basis, opts)
    e_acc = S.energy()
    seen = set()
    kinds = ["insert", "remove", "move"]
    # the first six moves walk through every (kind, verdict); the rest are drawn
    plan = [(k, v) for k in kinds for v in (True, False)]
    for step in range(30):
        kind, accept = plan[step] if step < len(plan) else (kinds[rng.integers(3)], rng.random() < 0.5)
        label = f"{name} step {step} {kind}"
        mols = molecules(atoms)
        if kind == "insert":
            at, mol = random_insertion(rng, atoms, basis)
            trial = inserted(atoms, at, mol)
            e_trial = S.trial_insert_energy(at, mol)
        elif kind == "remove":
            a, b = mols[rng.integers(len(mols))]
            trial = removed(atoms, a, b)
            e_trial = S.trial_remove_energy(a, b - a)
        else:
            a, b = mols[rng.integers(len(mols))]
            trial = dict(atoms, pos=atoms["pos"].copy())
            trial["pos"][a:b] += rng.normal(scale=0.4, size=(b - a, 3))
            e_trial = S.trial_energy(a, trial["pos"][a:b])
        if kind == "move":
            assert not S.last_trial_was_full(), label
            util.check_trial_against_fresh(S, trial, basis, opts, trial["pos"], rel=1e-11, label=label)
            ref = util.check_trial_against_oracle(S.trial_observables, trial, basis, opts, trial["pos"], label=label)
        else:
            ref = check_exchange(S, trial, basis, opts, label)
        assert util.close(e_trial, ref["energy"]), label
        seen.add((kind, accept))
        if accept:
            S.accept()
            atoms, e_acc = trial, e_trial
            assert S.n == len(atoms["pos"])
            for k in atoms:  # the object's own arrays follow (the inserted molecule's id is the library's choice: one no other atom has)
                if k != "mol_id":
                    assert np.array_equal(S.atoms[k], atoms[k]), (label, k)
            assert molecules(S.atoms) == molecules(atoms), label
        else:
            S.reject()
    assert seen == {(k, v) for k in kinds for v in (True, False)}
    e_final = S.energy()
    ref = OracleSystem(atoms, basis, opts).energy()
    assert util.close(e_final, ref["energy"]) and util.close(e_acc, ref["energy"], 1e-10)
    # (under Wolf the oracle reports no electrostatic in-cutoff count: util.check_trial_against_oracle)
    util.assert_counts(S.observables, ref, bool(opts.get("rd_only")) or bool(opts.get("wolf")), label=name)
    S.close()


def lj_atom_at(atoms, basis, frac):
    return molecule(atoms, 0, 1, (np.asarray(frac) @ np.asarray(basis).reshape(3, 3))[None, :])


def test_tile_edges_one_tile():
    """lj64 is exactly one tile: 64 -> 65 (a tile is born) -> 66 -> 65 -> 64 (it dies again)"""
    atoms, basis, opts = util.load_fixture("lj64")
    atoms = {k: np.array(v) for k, v in atoms.items()}
    assert len(atoms["pos"]) == 64
    S = energy.System(atoms, basis, nonpolar(opts), max_atoms=256)
    opts = nonpolar(opts)
    S.energy()
    steps = [("insert", 64, (0.13, 0.57, 0.91)), ("insert", 0, (1.31, -0.42, 0.25)), ("remove", 65, None), ("remove", 0, None)]
    for i, (kind, at, frac) in enumerate(steps):
        if kind == "insert":
            mol = lj_atom_at(atoms, basis, frac)
            trial = inserted(atoms, at, mol)
            S.trial_insert_energy(at, mol)
        else:
            trial = removed(atoms, at, at + 1)
            S.trial_remove_energy(at, 1)
        check_exchange(S, trial, basis, opts, f"one tile step {i}")
        S.accept()
        atoms = trial
        # a displacement on the new composition, without any re-basing evaluation in between
        moved = dict(atoms, pos=atoms["pos"].copy())
        moved["pos"][3] += 0.2
        S.trial_energy(3, moved["pos"][3:4])
        assert not S.last_trial_was_full()
        util.check_trial_against_fresh(S, moved, basis, opts, moved["pos"], label=f"one tile step {i} displacement")
        S.reject()
    assert len(atoms["pos"]) == 64
    ref = util.oracle_energy(atoms, basis, opts)
    assert util.close(S.energy(), ref["energy"])
    util.assert_counts(S.observables, ref, False, label="one tile")
    S.close()


def test_tile_edges_three_full_tiles():
    """The 64 waters of water64_polar are 192 atoms = three full tiles (the fixture carries one more single-atom molecule at its end, which
    goes first: 193 -> 192, the fourth tile dies): 189 (padding appears), then 195 (a fourth tile again)"""
    atoms, basis, opts = util.load_fixture("water64_polar")
    opts = nonpolar(opts)
    atoms = {k: np.array(v) for k, v in atoms.items()}
    assert len(atoms["pos"]) == 193 and molecules(atoms)[-1] == (192, 193)
    rng = np.random.default_rng(5)
    S = energy.System(atoms, basis, opts, max_atoms=256)
    S.energy()
    trial = removed(atoms, 192, 193)
    S.trial_remove_energy(192, 1)
    check_exchange(S, trial, basis, opts, "193 -> 192")
    S.accept()
    atoms = trial
    assert len(atoms["pos"]) == 192
    a, b = molecules(atoms)[17]
    trial = removed(atoms, a, b)
    S.trial_remove_energy(a, b - a)
    check_exchange(S, trial, basis, opts, "192 -> 189")
    S.accept()
    atoms = trial
    for i in range(2):
        at, mol = random_insertion(rng, atoms, basis)
        trial = inserted(atoms, at, mol)
        S.trial_insert_energy(at, mol)
        check_exchange(S, trial, basis, opts, f"insertion {i} after 189")
        S.accept()
        atoms = trial
    assert len(atoms["pos"]) == 195
    ref = util.oracle_energy(atoms, basis, opts)
    assert util.close(S.energy(), ref["energy"])
    util.assert_counts(S.observables, ref, False, label="195")
    S.close()


def test_accepted_insertion_grows_the_context():
    atoms, basis, opts = util.load_fixture("ion64_es")
    opts = nonpolar(opts)
    atoms = {k: np.array(v) for k, v in atoms.items()}
    S = energy.System(atoms, basis, opts, max_atoms=len(atoms["pos"]))
    S.energy()
    at, mol = random_insertion(np.random.default_rng(9), atoms, basis)
    trial = inserted(atoms, at, mol)
    e_trial = S.trial_insert_energy(at, mol)
    check_exchange(S, trial, basis, opts, "growth")
    S.accept()
    assert S.observables["energy"] == e_trial
    # the totals are kept: a trial that moves nothing returns the accepted totals
    a, b = molecules(trial)[0]
    assert S.trial_energy(a, trial["pos"][a:b]) == e_trial
    S.reject()
    a, b = molecules(trial)[5]
    S.trial_remove_energy(a, b - a)
    check_exchange(S, removed(trial, a, b), basis, opts, "removal after growth")
    S.reject()
    assert util.close(S.energy(), util.oracle_energy(trial, basis, opts)["energy"])
    S.close()


def test_long_molecule():
    """a rigid molecule of 12 charged LJ sites (more than the 8 atoms a displacement carries in its kernel arguments), inserted and removed"""
    atoms, basis, opts = util.load_fixture("ion64_es")
    opts = nonpolar(opts)
    atoms = {k: np.array(v) for k, v in atoms.items()}
    rng = np.random.default_rng(12)
    m = 12
    B = np.asarray(basis).reshape(3, 3)
    mol = molecule(atoms, 0, 1)
    mol = {k: np.repeat(v, m, axis=0) for k, v in mol.items()}
    mol["pos"] = np.array([0.4, 0.6, 0.2]) @ B + rng.normal(scale=1.2, size=(m, 3))
    mol["charge"] = np.where(np.arange(m) % 2 == 0, 0.35, -0.35)
    mol["sigma"] = np.linspace(2.5, 3.5, m)
    mol["epsilon"] = np.linspace(20.0, 60.0, m)
    S = energy.System(atoms, basis, opts, max_atoms=128)
    S.energy()
    at = molecules(atoms)[20][0]
    trial = inserted(atoms, at, mol)
    S.trial_insert_energy(at, mol)
    check_exchange(S, trial, basis, opts, "long molecule in")
    S.accept()
    atoms = trial
    other = molecules(atoms)[3]
    S.trial_remove_energy(other[0], other[1] - other[0])
    check_exchange(S, removed(atoms, *other), basis, opts, "a neighbour out")
    S.reject()
    S.trial_remove_energy(at, m)
    trial = removed(atoms, at, at + m)
    check_exchange(S, trial, basis, opts, "long molecule out")
    S.accept()
    ref = util.oracle_energy(trial, basis, opts)
    assert util.close(S.energy(), ref["energy"])
    S.close()


@pytest.mark.parametrize("kind", ["insert", "remove"])
@pytest.mark.parametrize("name", ["ion64_es", "water64_fh2"])
def test_rejection_leaves_no_trace(name, kind):
    atoms, basis, opts = util.load_fixture(name)
    opts = nonpolar(opts)
    atoms = {k: np.array(v) for k, v in atoms.items()}
    rng = np.random.default_rng(3)
    a, b = molecules(atoms)[7]
    fixed = atoms["pos"][a:b] + 0.25

    def probe(S):
        e_t = S.trial_energy(a, fixed)
        obs_t = dict(S.trial_observables)
        S.reject()
        return e_t, obs_t, S.energy(), dict(S.observables)

    untouched = energy.System(atoms, basis, opts)
    untouched.energy()
    want = probe(untouched)
    S = energy.System(atoms, basis, opts)
    S.energy()
    if kind == "insert":
        at, mol = random_insertion(rng, atoms, basis)
        S.trial_insert_energy(at, mol)
    else:
        c, d = molecules(atoms)[11]
        S.trial_remove_energy(c, d - c)
    assert not S.last_trial_was_full()
    S.reject()
    assert S.n == len(atoms["pos"]) and np.array_equal(S.atoms["pos"], atoms["pos"])
    assert probe(S) == want  # the same bits as a context that never saw the trial
    S.close()
    untouched.close()


@pytest.mark.parametrize("verdict", ["accept", "reject"])
def test_polarizable_box_takes_the_full_evaluation(verdict):
    atoms, basis, opts = util.load_fixture("water64_polar")
    atoms = {k: np.array(v) for k, v in atoms.items()}
    rng = np.random.default_rng(21)
    S = energy.System(atoms, basis, opts)
    S.energy()
    at, mol = random_insertion(rng, atoms, basis)
    trial = inserted(atoms, at, mol)
    S.trial_insert_energy(at, mol)
    check_exchange(S, trial, basis, opts, "polarizable insertion", full=True)
    if verdict == "accept":
        S.accept()
        atoms = trial
    else:
        S.reject()
    assert util.close(S.energy(), util.oracle_energy(atoms, basis, opts)["energy"])
    a, b = molecules(atoms)[9]
    trial = removed(atoms, a, b)
    S.trial_remove_energy(a, b - a)
    check_exchange(S, trial, basis, opts, "polarizable removal", full=True)
    if verdict == "accept":
        S.accept()
        atoms = trial
    else:
        S.reject()
    assert S.n == len(atoms["pos"])
    assert util.close(S.energy(), util.oracle_energy(atoms, basis, opts)["energy"])
    S.close()


def test_protocol_errors():
    atoms, basis, opts = util.load_fixture("water64_polar")
    opts = nonpolar(opts)
    atoms = {k: np.array(v) for k, v in atoms.items()}
    a, b = molecules(atoms)[4]
    mol = molecule(atoms, a, b, atoms["pos"][a:b] + 1.0)
    S = energy.System(atoms, basis, opts)

    def fails(code, fn, *args):
        with pytest.raises(energy.MpmcError) as e:
            fn(*args)
        assert e.value.code == code, (e.value.code, str(e.value))
        assert str(e.value)

    fails(ERR_ARG, S.trial_remove_energy, a, b - a)  # no accepted configuration yet
    fails(ERR_ARG, S.trial_insert_energy, a, mol)
    e0 = S.energy()
    fails(ERR_ARG, S.trial_remove_energy, a, b - a - 1)  # not a whole molecule
    fails(ERR_ARG, S.trial_remove_energy, a + 1, b - a)  # straddles two
    fails(ERR_ARG, S.trial_remove_energy, a, 2 * (b - a))  # two molecules
    fails(ERR_ARG, S.trial_insert_energy, a + 1, mol)  # inside a molecule
    fails(ERR_ARG, S.trial_insert_energy, len(atoms["pos"]) + 1, mol)
    bad = dict(mol, pos=mol["pos"].copy())
    bad["pos"][1, 2] = np.nan
    fails(ERR_INVALID_DATUM, S.trial_insert_energy, a, bad)
    S.trial_remove_energy(a, b - a)
    fails(ERR_ARG, S.trial_remove_energy, a, b - a)  # a trial is already open
    fails(ERR_ARG, S.trial_insert_energy, a, mol)
    fails(ERR_ARG, S.trial_energy, a, atoms["pos"][a:b] + 0.1)
    S.reject()
    assert S.energy() == e0  # usable, and unchanged
    # the only molecule of a box cannot be removed
    one = molecule(atoms, a, b)
    T = energy.System(one, basis, opts)
    T.energy()
    fails(ERR_ARG, T.trial_remove_energy, 0, b - a)
    T.trial_insert_energy(b - a, mol)
    check_exchange(T, inserted(one, b - a, mol), basis, opts, "second molecule")
    T.accept()
    T.close()
    S.trial_insert_energy(a, mol)
    check_exchange(S, inserted(atoms, a, mol), basis, opts, "after the errors")
    S.reject()
    S.close()


def test_cpp_facade_exchange_trials(tmp_path):
    """include/mpmc_system.hpp: accept_trial() edits the facade's list as the library edited its own"""
    import json
    import subprocess

    import test_exchange_moves

    exe = test_exchange_moves.build(tmp_path)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert (r["n_in"], r["n_final"], r["N_trial"]) == (130, 128, 65.0) and r["refused"] != 0
    # 1e-11: a trial total against an evaluation of the same list (the bound of util.check_trial_against_fresh)
    assert util.close(r["e_in"], r["e_in_fresh"], 1e-11) and util.close(r["e_in"], r["e_in_again"], 1e-11)
    assert r["e_back"] == r["e_in_again"] and r["e_out"] != r["e_in"]  # a rejected removal leaves the same bits
    assert util.close(r["e_gone"], r["e_final"], 1e-11) and util.close(r["e_final"], r["e0"], 1e-11)  # the inserted dimer is out again
