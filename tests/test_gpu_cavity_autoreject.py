"""cavity_autoreject on the GPU: the contact counts of mpmc_set_cavity_autoreject / mpmc_cavity_autoreject_info (kernels_contact.hip).

The goldens (tests/golden/autoreject_cases.json, tools/make_autoreject_golden.py) are the reference's own results with the keywords
`cavity_autoreject`, `cavity_autoreject_absolute` and `cavity_autoreject_scale` appended to committed fixtures; tests/cavity_autoreject_ref.py
restates the contract in numpy (brute-force counts with the minimum image).  Counts are integers and compared exactly; the sum
lj_pairs = S + n_replaced * 1e40 is compared exactly against the setting-off run of the same context.
"""
import ctypes as C

import numpy as np
import pytest

import cavity_autoreject_ref as R
import util
from mpmcxx_amd import energy, gen_box, pqr

pytestmark = pytest.mark.gpu

RESULT_FIELDS = [f for f, _ in energy.Result._fields_]
CASES = sorted(R.cases())
MAXVALUE = 1.0e40
BOTH = R.SIGMA | R.ABSOLUTE
COUNT_KEYS = ("n_replaced", "n_absolute", "n_unmeasured_frozen")
ERR_ARG, ERR_INVALID_SETTING, ERR_UNSUPPORTED = -3, 4000, 4004


@pytest.fixture(scope="module", autouse=True)
def _need_device():
    if energy.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests need an MI355X")


def bits(r):
    return {k: r[k] for k in RESULT_FIELDS}


def info_counts(S):
    i = S.cavity_autoreject_info()
    return {k: i[k] for k in COUNT_KEYS}


def ref_counts(atoms, basis, opts, rules, scale, pos=None):
    c = R.counts(atoms, basis, opts, rules, scale, pos)
    return {k: c[k] for k in COUNT_KEYS}


def fresh(atoms, basis, opts, rules, scale, pos=None):
    """a new context's evaluation of a configuration under the setting: (returned energy, observables, info)"""
    F = energy.System(atoms if pos is None else util.with_positions(atoms, pos), basis, R.without_keys(opts))
    F.set_cavity_autoreject(rules, scale, float(opts.get("cavity_autoreject_repulsion") or 0.0))
    e = F.energy()
    out = (e, dict(F.observables), F.cavity_autoreject_info())
    F.close()
    return out


_SLABS = {}


def slab(n, tmp_path_factory):
    """slab<n>_planted without polarization: 17 / 33 tiles in a 25 x 25 x 83+ A cell (tile pairs beyond every contact distance exist), planted
    pairs at 2.0 A, three-site molecules of which every sixth is frozen"""
    if n not in _SLABS:
        inp, _ = gen_box.materialize(f"slab{n}_planted", str(tmp_path_factory.mktemp(f"slab{n}")))
        atoms, basis, opts = pqr.load_case(inp)
        _SLABS[n] = (atoms, basis, util.nonpolar(opts))
    atoms, basis, opts = _SLABS[n]
    return {k: np.array(v) for k, v in atoms.items()}, np.array(basis), dict(opts)


# ---- the reference's own results ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_parity_with_reference_golden(name):
    atoms, basis, opts, case = R.load(name)
    g, plain = case["result"], case["plain"]
    rules, scale = R.rules_of(opts)
    S = energy.System(atoms, basis, opts)  # (the options carry the keywords: set_options switches the setting on)
    returned = S.energy()
    obs, info = dict(S.observables), S.cavity_autoreject_info()
    print(name, returned, obs["rd_energy"], obs["lj_pairs"], info)
    assert (info["rules"], info["scale"]) == (rules, scale)
    # energies: the observables against the harness's parts, the returned value against its total (the absolute rule's MAXVALUE included)
    for ours, ref in (("rd_energy", "rd"), ("lj_pairs", "lj_pairs"), ("coulombic_energy", "es"), ("polarization_energy", "polar")):
        assert util.close(obs[ours], g[ref]), (name, ours, obs[ours], g[ref])
    assert util.close(returned, g["total"]) and returned == info["returned_energy"], (name, returned, g["total"])
    assert util.close(obs["energy"], (g["rd"] + g["es"]) + g["polar"]), (name, obs["energy"])
    # counts: exact
    assert info["n_replaced"] == round(g["lj_pairs"] / MAXVALUE) == R.restated(name)["n_replaced"], (name, info)
    assert info_counts(S) == {k: R.restated(name)[k] for k in COUNT_KEYS}, (name, info)
    hit = info["n_absolute"] + info["n_unmeasured_frozen"] > 0
    assert info["absolute_penalty"] == (MAXVALUE if hit else 0.0) and hit == (g["total"] - g["rd"] > 0.5 * MAXVALUE and bool(rules & R.ABSOLUTE))
    # against the setting off, same context: electrostatics and polarization to the bit, the sum exact, a case without contact to the bit
    S.set_cavity_autoreject(0)
    off_returned = S.energy()
    off = dict(S.observables)
    for k in RESULT_FIELDS:
        if k not in ("energy", "NU", "rd_energy", "lj_pairs"):
            assert obs[k] == off[k], (name, k, obs[k], off[k])
    assert obs["lj_pairs"] == off["lj_pairs"] + float(info["n_replaced"]) * MAXVALUE
    if info["n_replaced"] == 0:
        assert bits(obs) == bits(off)
        if not hit:
            assert returned == off_returned
    assert util.close(off["energy"], plain["total"]) and off_returned == off["energy"]
    S.close()


# ---- exactness of the sum and of the counts, on boxes with partial tiles, many tiles and a skewed cell ---------------------------------------
@pytest.mark.parametrize("name,scale", [("ion216_polar", 1.0), ("water64_polar", 1.0), ("ion1000_polar", 1.0), ("ion216_triclinic", 1.0),
                                        ("slab1025", 1.0), ("slab2049", 0.9)])
def test_sum_is_exact_and_counts_equal_the_restatement(name, scale, tmp_path_factory):
    if name.startswith("slab"):
        atoms, basis, opts = slab(int(name[4:]), tmp_path_factory)
    else:
        atoms, basis, opts = util.load_fixture(name)
        opts = util.nonpolar(opts) if name == "ion1000_polar" else opts  # (the dipole solve of 1000 atoms is other tests')
    S = energy.System(atoms, basis, opts)
    S.energy()
    off = dict(S.observables)
    want = ref_counts(atoms, basis, opts, BOTH, scale)
    S.set_cavity_autoreject(BOTH, scale)
    e = S.energy()
    on, info = dict(S.observables), S.cavity_autoreject_info()
    print(name, scale, info)
    assert info_counts(S) == want, (name, info, want)
    assert want["n_replaced"] > 0
    assert on["lj_pairs"] == off["lj_pairs"] + float(want["n_replaced"]) * MAXVALUE
    assert on["rd_energy"] == (on["lj_pairs"] + off["lrc_pair"]) + off["lrc_self"]
    assert on["energy"] == on["rd_energy"] + off["coulombic_energy"] + off["polarization_energy"] and on["NU"] == on["N"] * on["energy"]
    assert e == on["energy"] + info["absolute_penalty"]
    assert info["tile_pairs_walked"] + info["tile_pairs_skipped"] == (S.n + 63) // 64 * ((S.n + 63) // 64 + 1) // 2
    if name == "ion216_triclinic":
        assert info["tile_pairs_skipped"] == 0
    if name.startswith("slab"):
        assert want["n_unmeasured_frozen"] > 0 and info["absolute_penalty"] == MAXVALUE  # (frozen molecules, polarization off: the quirk pairs)
    # each rule alone shares the walk's counts; mpmc_lj returns the penalised rd_energy
    S.set_cavity_autoreject(R.SIGMA, scale)
    assert S.lj() == on["rd_energy"] and S.cavity_autoreject_info()["n_replaced"] == want["n_replaced"]
    S.energy()
    i = S.cavity_autoreject_info()
    assert (i["n_replaced"], i["n_absolute"], i["n_unmeasured_frozen"], i["absolute_penalty"]) == (want["n_replaced"], 0, 0, 0.0)
    assert bits(S.observables) == bits(on)
    S.set_cavity_autoreject(R.ABSOLUTE, scale)
    S.energy()
    i = S.cavity_autoreject_info()
    assert (i["n_replaced"], i["n_absolute"], i["n_unmeasured_frozen"]) == (0, want["n_absolute"], want["n_unmeasured_frozen"])
    assert bits(S.observables) == bits(off)  # (the absolute rule never touches the observables)
    S.close()


# ---- tile-pair skipping ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rules", [R.SIGMA, R.ABSOLUTE])
def test_tile_pair_skipping_on_the_slab(rules, tmp_path_factory):
    """Tiles in list order (spatial_sort = 0: 64 consecutive atoms, about 1.3 layers of the slab), one atom pulled next to an atom 11 tiles
    further up the list at dmax (1 -+ 1e-9): the pair below dmax is found across the two tiles, the pair above is not, and the walk that
    skips tile pairs counts what the walk of every tile pair counts."""
    atoms, basis, opts = slab(1025, tmp_path_factory)
    scale = 0.93
    a, b = 12, 710  # (single-atom molecules, movable, tiles 0 and 11)
    assert atoms["mol_id"][a] != atoms["mol_id"][b] and not atoms["frozen"][a] and not atoms["frozen"][b]
    dmax = scale * 0.5 * (atoms["sigma"][a] + atoms["sigma"][b]) if rules == R.SIGMA else scale
    key = "n_replaced" if rules == R.SIGMA else "n_absolute"
    seen = {}
    for label, factor in (("below", 1.0 - 1e-9), ("above", 1.0 + 1e-9)):
        pos = atoms["pos"].copy()
        pos[b] = pos[a] + np.array([0.0, 0.0, -dmax * factor])  # (below the first layer: through the periodic face of the long axis)
        moved = util.with_positions(atoms, pos)
        want = R.counts(moved, basis, opts, rules, scale)
        pair_in = (a, b) in (want["replaced_pairs"] if rules == R.SIGMA else want["absolute_pairs"])
        assert pair_in == (label == "below")
        got = {}
        for skip in (1, 0):
            S = energy.System(moved, basis, opts)
            S.configure("spatial_sort", 0)
            S.configure("contact_skip", skip)
            S.set_cavity_autoreject(rules, scale)
            S.energy()
            got[skip] = S.cavity_autoreject_info()
            S.close()
        print(rules, label, got[1])
        assert got[1]["tile_pairs_skipped"] > 0 and got[0]["tile_pairs_skipped"] == 0
        assert got[1]["tile_pairs_walked"] < got[0]["tile_pairs_walked"] == 17 * 18 // 2
        for k in COUNT_KEYS:
            assert got[1][k] == got[0][k] == want[k], (label, k, got[1][k], got[0][k], want[k])
        seen[label] = got[1][key]
    assert seen["below"] == seen["above"] + 1


# ---- trial moves --------------------------------------------------------------------------------------------------------------------------
def _contact_pose(atoms, mover, target_o, dist=0.8, site=1):
    """positions of molecule `mover` (first, end) translated so that its atom `site` (1: the first H) sits `dist` from atom target_o, along +x"""
    a, b = mover
    shift = atoms["pos"][target_o] + np.array([dist, 0.0, 0.0]) - atoms["pos"][a + site]
    return atoms["pos"][a:b] + shift


def _check_trial(S, atoms, basis, opts, rules, scale, pos, label, keys=util.TRIAL_KEYS):
    """the open trial of S against a new context's evaluation of the trial configuration and against the restatement: counts exactly, the
    energy components `keys` at the 1e-11 the suite holds a trial to against a fresh context (util.check_trial_against_fresh)"""
    e_ref, ref, iref = fresh(atoms, basis, opts, rules, scale, pos)
    got, info = dict(S.trial_observables), S.cavity_autoreject_info()
    want = ref_counts(atoms, basis, opts, rules, scale, pos)
    assert {k: info[k] for k in COUNT_KEYS} == {k: iref[k] for k in COUNT_KEYS} == want, (label, info, iref, want)
    bad = util.component_errors(got, ref, [k for k in keys if ref[k] != 0.0 or got[k] != 0.0], 1e-11)
    assert not bad, (label, bad)
    assert info["absolute_penalty"] == iref["absolute_penalty"] and info["returned_energy"] == got["energy"] + info["absolute_penalty"]
    return want


@pytest.mark.parametrize("polar", [0, 1])
def test_displacement_trials_follow_the_contacts(polar):
    atoms, basis, opts = util.load_fixture("water64_polar")
    opts = opts if polar else util.nonpolar(opts)
    rules, scale = BOTH, 1.0
    # the planted contact: without polarization an H at 0.8 A from another molecule's O (an absolute contact); in the polarizable box an O at
    # 0.95 sigma = 2.99 A from another O (a sigma contact at a distance where the ten Jacobi iterations stay well-conditioned), so that
    # every energy component is compared in both
    dist, site = (0.95 * 3.15, 0) if polar else (0.8, 1)
    keys = util.TRIAL_KEYS
    mols = util.molecules(atoms)
    S = energy.System(atoms, basis, opts)
    S.set_cavity_autoreject(rules, scale)
    S.energy()
    base = info_counts(S)
    assert base == ref_counts(atoms, basis, opts, rules, scale) and base["n_absolute"] == 0
    pos = atoms["pos"].copy()
    # a move that creates an absolute contact (and changes the sigma contacts of the molecule): H of molecule 5 at 0.8 A from the O of molecule 20
    a, b = mols[5]
    new = _contact_pose(atoms, mols[5], mols[20][0], dist, site)
    e = S.trial_energy(a, new)
    assert not S.last_trial_was_full()
    p1 = pos.copy()
    p1[a:b] = new
    made = _check_trial(S, atoms, basis, opts, rules, scale, p1, "create", keys)
    assert made != base and e == S.cavity_autoreject_info()["returned_energy"] and e >= MAXVALUE
    assert made["n_absolute"] >= 1 or polar
    planted = (a + site, mols[20][0]) if a + site < mols[20][0] else (mols[20][0], a + site)
    found = R.counts(atoms, basis, opts, rules, scale, p1)
    assert planted in (found["replaced_pairs"] if polar else found["absolute_pairs"])
    # reject: the accepted counts are back (a second trial starts from them)
    S.reject()
    S.trial_energy(a, new)
    _check_trial(S, atoms, basis, opts, rules, scale, p1, "again", keys)
    S.accept()
    S.energy()
    assert info_counts(S) == made
    # a move that removes the contact again
    moved = util.with_positions(atoms, p1)
    S.trial_energy(a, pos[a:b])
    gone = _check_trial(S, moved, basis, opts, rules, scale, pos, "remove", keys)
    assert gone == base
    S.reject()
    # a contact between two moved atoms: molecules 30 and 31 move together, the planted site of 31 lands next to the O of 30
    a0, b1 = mols[30][0], mols[31][1]
    both = p1[a0:b1].copy() + np.array([0.05, -0.03, 0.02])
    both[3:6] += (both[0] + np.array([dist, 0.0, 0.0])) - both[3 + site]
    S.trial_energy(a0, both)
    p2 = p1.copy()
    p2[a0:b1] = both
    pair = _check_trial(S, moved, basis, opts, rules, scale, p2, "two moved atoms", keys)
    found = R.counts(moved, basis, opts, rules, scale, p2)
    assert (a0, a0 + 3 + site) in (found["replaced_pairs"] if polar else found["absolute_pairs"])  # (both atoms of the pair moved)
    S.accept()
    S.energy()
    assert info_counts(S) == pair
    S.close()


def test_full_evaluation_fallback_of_a_long_move():
    atoms, basis, opts = util.load_fixture("ion1000_polar")
    opts = dict(opts, polar_max_iter=2)
    rules, scale = BOTH, 0.97
    S = energy.System(atoms, basis, opts)
    S.set_cavity_autoreject(rules, scale)
    S.energy()
    base = info_counts(S)
    m = 257  # (> MPMC_TRIAL_MAX_ATOMS)
    new = util.moved(atoms, 100, m, seed=3, sigma=0.4)
    S.trial_energy(100, new)
    assert S.last_trial_was_full()
    pos = atoms["pos"].copy()
    pos[100:100 + m] = new
    t = _check_trial(S, atoms, basis, opts, rules, scale, pos, "long move")
    assert t != base
    S.reject()
    S.energy()
    assert info_counts(S) == base
    S.trial_energy(100, new)
    S.accept()
    S.energy()
    assert info_counts(S) == t
    S.close()


def test_insertion_and_removal_trials_stay_on_the_delta_path():
    """an insertion adds the molecule's contacts with the residents, a removal subtracts them: O(m N), no full evaluation"""
    atoms, basis, opts = util.load_fixture("water64_polar")
    opts = util.nonpolar(opts)
    rules, scale = BOTH, 1.0
    mols = util.molecules(atoms)
    S = energy.System(atoms, basis, opts)
    S.set_cavity_autoreject(rules, scale)
    S.energy()
    base = info_counts(S)
    full0 = util.exchange_counts(S)[1]
    # insertion of a copy of molecule 5 whose H sits 0.8 A from the O of molecule 20
    a, b = mols[5]
    mol = {k: np.array(v[a:b]) for k, v in atoms.items()}
    mol["pos"] = _contact_pose(atoms, mols[5], mols[20][0])
    grown = {k: np.concatenate([v, mol[k]]) for k, v in atoms.items()}
    grown["mol_id"][-(b - a):] = int(atoms["mol_id"].max()) + 1
    e = S.trial_insert_energy(S.n, mol)
    assert not S.last_trial_was_full()
    ins = _check_trial(S, grown, basis, opts, rules, scale, grown["pos"], "insert")
    assert ins["n_absolute"] >= 1 and ins["n_replaced"] > base["n_replaced"] and e >= MAXVALUE
    S.reject()
    S.trial_insert_energy(S.n, mol)  # (after a reject the accepted counts are back: the same trial again)
    _check_trial(S, grown, basis, opts, rules, scale, grown["pos"], "insert again")
    S.accept()
    assert S.n == len(grown["pos"])
    # a displacement and a removal start from the accepted trial counts without a re-basing evaluation
    S.trial_remove_energy(mols[7][0], 3)
    assert not S.last_trial_was_full()
    less = {k: np.delete(v, np.s_[mols[7][0]:mols[7][1]], axis=0) for k, v in grown.items()}
    _check_trial(S, less, basis, opts, rules, scale, less["pos"], "remove another")
    S.reject()
    S.energy()
    assert info_counts(S) == ins
    # removal of the inserted molecule: its contacts go
    S.trial_remove_energy(len(atoms["pos"]), b - a)
    assert not S.last_trial_was_full()
    out = _check_trial(S, atoms, basis, opts, rules, scale, atoms["pos"], "remove")
    assert out == base
    S.accept()
    S.energy()
    assert info_counts(S) == base and util.exchange_counts(S)[1] == full0  # (no exchange trial of this test was evaluated in full)
    S.close()


def test_exchange_trials_count_the_unmeasured_frozen_pairs_of_the_trial_composition():
    atoms, basis, opts = util.load_fixture("ion216_frozen")
    opts = util.nonpolar(opts)
    rules, scale = BOTH, 1.0
    S = energy.System(atoms, basis, opts)
    S.set_cavity_autoreject(rules, scale)
    S.energy()
    base = info_counts(S)
    frozen = np.nonzero(atoms["frozen"])[0]
    first = int(frozen[3])  # (single-atom molecules: a frozen one leaves, and comes back at another place)
    S.trial_remove_energy(first, 1)
    assert not S.last_trial_was_full()
    less = {k: np.delete(v, first, axis=0) for k, v in atoms.items()}
    t = _check_trial(S, less, basis, opts, rules, scale, less["pos"], "remove frozen")
    assert t["n_unmeasured_frozen"] == base["n_unmeasured_frozen"] - (len(frozen) - 1)
    S.accept()
    mol = {k: np.array(v[first:first + 1]) for k, v in atoms.items()}
    mol["pos"] = atoms["pos"][first:first + 1] + np.array([0.4, -0.3, 0.2])
    grown = {k: np.concatenate([less[k], mol[k]]) for k in less}
    grown["mol_id"][-1] = int(less["mol_id"].max()) + 1
    S.trial_insert_energy(S.n, mol)
    assert not S.last_trial_was_full()
    t = _check_trial(S, grown, basis, opts, rules, scale, grown["pos"], "insert frozen")
    assert t["n_unmeasured_frozen"] == base["n_unmeasured_frozen"]
    S.accept()
    S.energy()
    assert info_counts(S) == t
    S.close()


# ---- batched insertion candidates ---------------------------------------------------------------------------------------------------------
def _species():
    """a rigid bent three-site molecule: X, a small Lennard-Jones site (sigma 0.5 A: the mixed sigma with the box's 3.405 A is 1.95 A), and two
    charged sites without dispersion 0.9572 A from it"""
    z = np.zeros(3)
    return {"charge": np.array([-0.8, 0.4, 0.4]) * 408.7816, "polarizability": z.copy(), "epsilon": np.array([50.0, 0.0, 0.0]),
            "sigma": np.array([0.5, 0.0, 0.0]), "mass": np.array([15.999, 1.008, 1.008]), "frozen": np.zeros(3, np.int32), "has_disp": np.zeros(3, np.int32)}


def _pose(A, dist, toward):
    """X at `dist` along +x from the point A, its first H pointing at A (toward) or away, the second 104.52 degrees from the first"""
    th = np.radians(104.52)
    d, e = np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0])
    u = -d if toward else d
    v = np.cos(th) * u + np.sin(th) * e
    p = A + dist * d
    return np.stack([p, p + 0.9572 * u, p + 0.9572 * v])


def _batch_box():
    """ion216_polar without polarization, scale 0.8 (no contact among the residents), and 600 poses of _species: the four kinds next to atom
    100 -- in a void (no contact), X at 1.4 A (sigma contact: 1.4 < 0.8 * 1.95), H at 0.8 A with X at 1.757 A (absolute contact only),
    X at 1.2 A with its H at 0.24 A (both) -- then seeded translations of them through the cell"""
    atoms, basis, opts = util.load_fixture("ion216_polar")
    opts = util.nonpolar(opts)
    A = atoms["pos"][100]
    kinds = [_pose(A + np.array([2.0, 2.0, 2.0]), 0.0, False), _pose(A, 1.4, False), _pose(A, 1.757, True), _pose(A, 1.2, True)]
    rng = np.random.default_rng(23)
    poses = kinds + [kinds[k % 4] + rng.uniform(-12.0, 12.0, size=3) for k in range(596)]
    return atoms, basis, opts, np.stack(poses)


def test_candidate_kinds_are_what_they_were_built_for():
    atoms, basis, opts, poses = _batch_box()
    sp = _species()
    got = []
    for c in range(4):
        g = {k: np.concatenate([atoms[k], sp[k]]) for k in sp}
        g["pos"] = np.concatenate([atoms["pos"], poses[c]])
        g["mol_id"] = np.concatenate([atoms["mol_id"], [int(atoms["mol_id"].max()) + 1] * 3]).astype(np.int32)
        r = R.counts(g, basis, opts, BOTH, 0.8)
        got.append((r["n_replaced"], r["n_absolute"]))
    assert got == [(0, 0), (1, 0), (0, 1), (1, 1)]


@pytest.mark.parametrize("n_cand", [1, 256, 257, 600])
def test_insert_candidates_equal_the_loop_of_single_insertion_trials(n_cand):
    """out[c] and the per-candidate counts, bit for bit, across the internal chunks of 256 candidates"""
    atoms, basis, opts, poses = _batch_box()
    poses = poses[3:4] if n_cand == 1 else poses[:n_cand]
    sp = _species()
    S = energy.System(atoms, basis, opts, max_atoms=len(atoms["pos"]) + 64)
    L = S._L
    none = (C.c_int64 * 1)()
    assert L.mpmc_insert_candidates_contacts(S.handle, n_cand, none, none) == ERR_ARG and b"no batch" in L.mpmc_last_error(S.handle)
    S.set_cavity_autoreject(BOTH, 0.8)
    S.energy()
    accepted, base = bits(S.observables), info_counts(S)
    out = S.insert_candidates(sp, poses)
    nr, na = S.insert_candidates_contacts(n_cand)
    assert L.mpmc_insert_candidates_contacts(S.handle, n_cand + 1, none, none) == ERR_ARG and b"differs" in L.mpmc_last_error(S.handle)
    kinds = set()
    for c in range(n_cand):
        S.trial_insert_energy(S.n, dict(sp, pos=poses[c]))
        assert not S.last_trial_was_full()
        t, i = bits(S.trial_observables), S.cavity_autoreject_info()
        S.reject()
        assert bits(out[c]) == t, c
        assert (int(nr[c]), int(na[c])) == (i["n_replaced"], i["n_absolute"]), c
        kinds.add((nr[c] > base["n_replaced"], na[c] > 0))
    assert (int(nr[0]), int(na[0])) == ((0, 0) if n_cand > 1 else (1, 1))  # (the lone candidate is the one with both contacts)
    if n_cand >= 256:
        assert kinds == {(False, False), (True, False), (False, True), (True, True)}
        assert [(int(nr[c]), int(na[c])) for c in range(4)] == [(0, 0), (1, 0), (0, 1), (1, 1)]
    # nothing of the accepted state moved; with the setting off the batch has the bits of a context that never made the call, and no counts
    S.energy()
    assert bits(S.observables) == accepted and info_counts(S) == base
    S.set_cavity_autoreject(0)
    S.energy()
    off = S.insert_candidates(sp, poses)
    P = energy.System(atoms, basis, opts, max_atoms=len(atoms["pos"]) + 64)
    P.energy()
    never = P.insert_candidates(sp, poses)
    P.close()
    assert [bits(r) for r in off] == [bits(r) for r in never]
    nr, na = S.insert_candidates_contacts(n_cand)
    assert not nr.any() and not na.any()
    for c in range(min(n_cand, 4)):  # (the sigma rule's penalty is the only difference of the batch under the setting)
        replaced = (c in (1, 3)) if n_cand > 1 else True
        assert out[c]["lj_pairs"] == off[c]["lj_pairs"] + (MAXVALUE if replaced else 0.0)
    S.close()


def test_disp_expansion_sigma_and_repulsion_tests():
    """under the disp-expansion term the rule is disp_expansion()'s: no cutoff, sigma_ij = r0_ij, and the repulsion test beside it"""
    atoms, basis, opts, case = R.load("ion216_disp_s09_rep100")
    rules, scale = R.rules_of(opts)
    S = energy.System(atoms, basis, opts)
    S.energy()
    base, obs = info_counts(S), dict(S.observables)
    i = S.cavity_autoreject_info()
    assert base == ref_counts(atoms, basis, opts, rules, scale) and i["repulsion"] == 100.0
    assert i["tile_pairs_skipped"] == 0  # (the repulsion test has no distance bound: every tile pair is walked)
    assert base["n_replaced"] > ref_counts(atoms, basis, dict(opts, cavity_autoreject_repulsion=0.0), rules, scale)["n_replaced"]
    assert S.disp_expansion() == obs["rd_energy"]  # (the component entry returns the penalised rd_energy, like mpmc_lj)
    pos = atoms["pos"].copy()
    for step, first in enumerate((7, 100, 101)):
        new = util.moved(util.with_positions(atoms, pos), first, 1, seed=40 + step, sigma=0.5)
        S.trial_energy(first, new)
        assert not S.last_trial_was_full()
        p2 = pos.copy()
        p2[first:first + 1] = new
        _check_trial(S, atoms, basis, opts, rules, scale, p2, f"disp {step}", ["rd_energy", "lj_pairs", "es_real", "es_recip"])
        if step != 1:
            S.accept()
            pos = p2
        else:
            S.reject()
    S.energy()
    assert info_counts(S) == ref_counts(atoms, basis, opts, rules, scale, pos)
    # without a threshold the sigma test alone, with the tile-pair skip
    S.set_cavity_autoreject(rules, 1.0, 0.0)
    S.energy()
    assert info_counts(S) == ref_counts(atoms, basis, dict(opts, cavity_autoreject_repulsion=0.0), rules, 1.0, pos)
    S.close()


# ---- refusals, lifetime, off --------------------------------------------------------------------------------------------------------------
def test_refusals():
    atoms, basis, opts = util.load_fixture("water64_polar")
    S = energy.System(atoms, basis, opts)
    L = S._L
    for scale in (0.0, 1.5, -0.1, float("nan")):
        assert L.mpmc_set_cavity_autoreject(S.handle, R.SIGMA, scale, 0.0) == ERR_INVALID_SETTING and b"scale" in L.mpmc_last_error(S.handle)
    assert L.mpmc_set_cavity_autoreject(S.handle, 4, 0.5, 0.0) == ERR_INVALID_SETTING
    assert L.mpmc_set_cavity_autoreject(S.handle, 0, 7.0, 0.0) == 0  # (off: the scale is not read)
    # the keyword's flag bit stays refused: the setter alone switches the behaviour on
    o = energy.make_options(opts)
    o.unsupported_flags = 1 << 16
    assert L.mpmc_set_options(S.handle, C.byref(o)) == ERR_UNSUPPORTED
    S.set_options(opts)
    # the sigma rule with rd_crystal: refused at the evaluation, with a text; the absolute rule runs beside it
    S.set_rd_crystal(True, 2)
    S.set_cavity_autoreject(R.SIGMA, 0.9)
    with pytest.raises(energy.MpmcError) as err:
        S.energy()
    assert err.value.code == ERR_UNSUPPORTED and "rd_crystal" in str(err.value)
    S.set_cavity_autoreject(R.ABSOLUTE, 0.9)
    S.energy()
    assert S.cavity_autoreject_info()["n_absolute"] == 0
    S.set_rd_crystal(False)
    # not while a trial move is open
    S.set_cavity_autoreject(R.SIGMA, 0.9)
    S.energy()
    S._check(L.mpmc_trial_begin(S.handle, 0, 1, energy._dp(np.ascontiguousarray(atoms["pos"][:1] + 0.2))))
    assert L.mpmc_set_cavity_autoreject(S.handle, BOTH, 0.9, 0.0) == ERR_ARG and b"trial" in L.mpmc_last_error(S.handle)
    S._check(L.mpmc_trial_energy(S.handle, C.byref(energy.Result())))
    S._check(L.mpmc_trial_reject(S.handle))
    S.close()


def test_setting_survives_set_atoms_set_box_set_options_and_growth():
    atoms, basis, opts = util.load_fixture("water64_polar")
    rules, scale = BOTH, 1.0
    S = energy.System(atoms, basis, opts, max_atoms=193)
    S.set_cavity_autoreject(rules, scale)
    S.energy()
    small = info_counts(S)
    assert small == ref_counts(atoms, basis, opts, rules, scale)
    big, bbasis, bopts = util.load_fixture("ion216_frozen")
    bopts = util.nonpolar(bopts)
    S.set_box(bbasis)
    S.set_atoms(big)  # (216 > 193: the context grows)
    S._check(S._L.mpmc_set_options(S.handle, C.byref(energy.make_options(bopts))))  # (through the C ABI, without the keywords)
    S.energy()
    want = ref_counts(big, bbasis, bopts, rules, scale)
    assert info_counts(S) == want and want["n_unmeasured_frozen"] > 0 and want["n_replaced"] > 0
    i = S.cavity_autoreject_info()
    assert (i["rules"], i["scale"]) == (rules, scale)
    S.update_positions(3, big["pos"][3:5] + 0.3)
    S.energy()
    p = big["pos"].copy()
    p[3:5] += 0.3
    assert info_counts(S) == ref_counts(big, bbasis, bopts, rules, scale, p)
    S.set_box(basis)
    S.set_atoms(atoms)
    S.set_options(opts)  # (options that never named the keywords leave the setting alone)
    S.energy()
    assert info_counts(S) == small
    S.close()


@pytest.mark.parametrize("name", ["lj64", "water64_polar", "ion1000_polar"])
def test_off_after_on_restores_bits_and_launch_counts(name):
    atoms, basis, opts = util.load_fixture(name)
    opts = util.nonpolar(opts) if name == "ion1000_polar" else opts
    mols = util.molecules(atoms)

    def run(S):
        S.set_profiling(True)
        S.timings(reset=True)
        S.energy()
        out = [bits(S.observables)]
        a, b = mols[3]
        S.trial_energy(a, atoms["pos"][a:b] + 0.21)
        out.append(bits(S.trial_observables))
        S.reject()
        S.energy()
        out.append(bits(S.observables))
        launches = {k: v["launches"] for k, v in S.timings().items()}
        S.set_profiling(False)
        return out, launches

    P = energy.System(atoms, basis, opts)
    never, never_launches = run(P)
    P.close()
    S = energy.System(atoms, basis, opts)
    S.set_cavity_autoreject(BOTH, 1.0)
    on, on_launches = run(S)
    assert on_launches["pair"] > never_launches["pair"]  # (the contact walk is timed with the pair kernels)
    S.set_cavity_autoreject(0)
    off, off_launches = run(S)
    assert off == never and off_launches == never_launches
    assert S.cavity_autoreject_info()["rules"] == 0
    S.close()
