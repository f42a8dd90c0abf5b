"""GPU (MI355X): displacement trials of polarizable boxes -- the `polar_delta` branch of mpmc_trial_energy_async (csrc/trial.cpp): O(m N)
deltas of the pair energies and of the real-space static field, the resident positions swapped, enqueue(RUN_STORE | RUN_SOLVE) with the
Thole store rewritten only for the tile pairs of touch[0 .. touch_n) (the moved atoms' tiles and the tiles a rejected trial left behind;
more than eight: every tile pair) -- under every solve configuration the path serves, at the eight-tile limit from both sides, and across
moves that flip tile-pair classes.

Boxes, configurations, moves and references: tests/polar_trial_cases.py; what makes the comparisons mean something (conditioning, distances,
which tiles the large moves cover, which classes the long jump flips, what the lattice hop does to the raw ranges) is asserted on the
CPU by tests/test_polar_trial_preconditions.py.

Every trial is held to
  a fresh context on the trial configuration   util.check_trial_against_fresh: 1e-11 per component, in-cutoff counts and polar_iterations exact
  its restatement, and the oracle where it knows the configuration
                                               the polarization energy at the REF_REL* of the variant's own GPU file (through the ragged
                                               ladder's BOUNDS), iterations exact, the Palmo correction and polar_relax_info's counters
                                               where they apply; every component at util.REL_TOL against the oracle, or against the
                                               oracle without polarization for the configurations it does not know
  not S.last_trial_was_full()
and after an accept S.dipoles() to the restatement's ef_static, mu and ef_induced as the ragged ladder compares them; an energy() behind an
accepted trial gives the trial's components to 1e-11.  Run with -s for the measured deviations.

As measured on an MI355X (largest over the file: polarization energy relative / ef_static / mu / ef_induced as fractions of their largest
component, against the restatements):
  jac_mf         1.2e-13 / 3.7e-13 / 1.3e-12 / 1.3e-12        jac_compact    1.2e-13 / 3.8e-13 / 1.1e-12 / 1.9e-12
  jac_dense      1.9e-14 / 3.7e-13 / 5.3e-13 / 4.4e-13        jac_dense_sym  1.9e-14 / 3.7e-13 / 5.3e-13 / 4.4e-13
    (the whole-matrix and the upper-triangle dense solve: the same configurations give their largest deviations, equal to two digits; step
    by step they differ, 2.8e-15 against 3.3e-15 in the energy of the 257-atom start, 3.7e-15 against 3.3e-15 in ef_induced on the slab)
  jac_gamma      2.0e-14 / 1.9e-13 / 6.2e-13 / 2.0e-13        jac_rrms       1.8e-14 / 1.9e-13 / 6.1e-13 / 2.0e-13
  gs             1.3e-13 / 3.7e-13 / 4.2e-12 / 4.6e-12        gs_nopbc       5.9e-15 / 3.2e-15 / 2.0e-13 / 4.2e-13
  gs_sor         1.5e-14 / 1.9e-13 / 5.1e-13 / 7.9e-13        jac_sor        1.4e-13 / 3.7e-13 / 2.4e-12 / 2.3e-12
  wolf_jac       2.4e-13 / 2.0e-15 / 1.6e-12 / 1.7e-12        wolf_gsp       1.5e-14 / 1.9e-15 / 2.7e-13 / 4.5e-13, correction 1.4e-14 |U_pol|
  zodid          1.3e-15 / 1.9e-13 / 1.8e-13 / 0              jac_prec       2.4e-15 / 1.8e-15 / 2.1e-13 / 1.1e-12
  gs_prec        2.2e-16 / 1.8e-15 / 6.5e-14 / 3.6e-13        jac_esor_prec  2.4e-14 / 2.5e-15 / 4.5e-13 / 1.9e-12
Tile stats of the slabs under the long jump, of 171 tile pairs: thole_far and beyond_cutoff 76 -> 71 in list order, 5 -> 4 under the spatial
order, as tests/test_polar_trial_preconditions.py restates them; in list order back at 76 with the pass behind the rejected jump.
"""
import numpy as np
import pytest

import util
import polar_ragged_boxes as B
import polar_trial_cases as C
import test_gpu_polar_ragged_ladder as L
import test_gpu_polar_wolf as PW
from mpmcxx_amd import energy

pytestmark = pytest.mark.gpu

REL = util.REL_TOL
FRESH_REL = 1e-11
OTHER_KEYS = [k for k in util.TRIAL_KEYS if k not in ("energy", "polarization_energy")]
SEEN = {}  # configuration -> {quantity: largest deviation over this module's comparisons}


@pytest.fixture(scope="module", autouse=True)
def _need_device():
    if energy.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests need an MI355X")


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for cfg, devs in SEEN.items():  # (with -s: the record in CHANGELOG.md)
        print(f"\nlargest, {cfg}: " + " ".join(f"{k} {v:.1e}" for k, v in devs.items()))


def make(rung, cfg, sort=1, pos=None):
    """a context of the box under cfg, in list order when sort == 0 (spatial_sort is read when the atoms are uploaded)"""
    atoms, basis, _ = B.box(rung)
    if pos is not None:
        atoms = util.with_positions(atoms, pos)
    energy.configure("spatial_sort", sort)  # (for the contexts created from here on)
    try:
        S = energy.System(atoms, basis, C.options(rung, cfg))
    finally:
        energy.configure("spatial_sort", 1)
    for key, value in C.CONFIGS[cfg][1]:
        S.configure(key, value)
    return S


def note(cfg, devs):
    seen = SEEN.setdefault(cfg, {})
    for k, v in devs.items():
        seen[k] = max(seen.get(k, 0.0), v)


def against_references(S, obs, rung, cfg, pos, label, dipoles=False):
    """`obs` (the trial's or the evaluation's observables of the live context S) against the restatement of the configuration `pos`, and
    against the oracle; dipoles: S.dipoles() too (after an accept or an evaluation: the context's dipoles are this configuration's)"""
    atoms = B.box(rung)[0]
    o = C.options(rung, cfg)
    want = C.restated(rung, cfg, pos)
    rel_e, rel_f = L.BOUNDS[C.family(cfg)]
    fails, devs = [], {}
    u = want["polarization_energy"]
    devs["energy"] = abs(obs["polarization_energy"] - u) / abs(u)
    if not abs(obs["polarization_energy"] - u) <= rel_e * abs(u):
        fails.append(("polarization_energy", obs["polarization_energy"], u))
    assert obs["polar_iterations"] == want["polar_iterations"], (label, "polar_iterations", obs["polar_iterations"], want["polar_iterations"])
    assert obs["iterator_failed"] == want["iterator_failed"] == 0, (label, "iterator_failed", obs["iterator_failed"], want["iterator_failed"])
    if o.get("polar_palmo"):
        corr = S.palmo_info()[0]
        devs["palmo"] = abs(corr - want["correction"]) / abs(u)
        if not (abs(corr - want["correction"]) <= PW.REF_REL * abs(u) and corr != 0.0 and want["correction"] != 0.0):
            fails.append(("palmo", corr, want["correction"]))
    if cfg in C.RELAXED:
        info = S.polar_relax_info()
        assert info["acted"] == 1 and info["contractions"] == want["contractions"], (label, info, want["contractions"])
        if cfg == "zodid":
            assert info["contractions"] == 0 and info["store_filled"] == 0, (label, info)
    if cfg in C.ORACLE_KNOWS:  # (util.check_trial_against_oracle's comparison, on the oracle's result kept per configuration)
        ref = C.oracle(rung, cfg, pos)
        bad = util.component_errors(obs, ref, util.TRIAL_KEYS, REL)
        assert not bad, f"{label}: against the oracle (rel {REL}): " + "; ".join(bad)
        for k in ("n_lj_in_cutoff", "n_es_in_cutoff", "polar_iterations"):
            assert obs[k] == ref[k], (label, k, obs[k], ref[k])
    else:  # every other component against the oracle with polarization off; the total is their sum with the restated polarization energy
        ref = C.others(rung, cfg, pos)
        bad = util.component_errors(obs, ref, OTHER_KEYS, REL)
        assert not bad, f"{label}: against the oracle without polarization (rel {REL}): " + "; ".join(bad)
        for k in ("n_lj_in_cutoff", "n_es_in_cutoff"):
            assert obs[k] == ref[k], (label, k, obs[k], ref[k])
        assert abs(obs["energy"] - (ref["energy"] + u)) <= REL * (abs(ref["energy"]) + abs(u)), (label, obs["energy"], ref["energy"], u)
    if dipoles:
        mu, E0, F = S.dipoles()
        for k, got in zip(L.ARRAYS, (E0, mu, F)):
            top = float(np.abs(want[k]).max())
            d = float(np.abs(got - want[k]).max())
            devs[k] = d / top if top else d
            if not d <= rel_f[k] * top:
                fails.append((k, d, top))
        assert not np.any(np.asarray(mu)[np.asarray(atoms["polarizability"]) == 0.0]), f"{label}: a dipole on an atom with alpha == 0"
    print(f"\n{label}: iterations {obs['polar_iterations']} " + " ".join(f"{k} {v:.1e}" for k, v in devs.items()))
    assert not fails, (label, fails)
    note(cfg, devs)


def trial(S, rung, cfg, pos, first, new, label):
    """one trial of S, whose accepted configuration is `pos`, held to the four references; returns the trial configuration"""
    atoms, basis, _ = B.box(rung)
    S.trial_energy(first, new)
    assert not S.last_trial_was_full(), f"{label}: the trial was evaluated in full"
    full = C.applied(pos, first, new)
    util.check_trial_against_fresh(S, atoms, basis, C.options(rung, cfg), full, rel=FRESH_REL, label=label)
    against_references(S, S.trial_observables, rung, cfg, full, label)
    return full


def accept(S, rung, cfg, full, label):
    """... accepted: the context's dipoles are the trial configuration's"""
    got = dict(S.trial_observables)
    S.accept()
    against_references(S, got, rung, cfg, full, f"{label}, accepted", dipoles=True)
    return got


def evaluated(S, rung, cfg, pos, label, trial_obs=None, rel=FRESH_REL):
    """energy() of the live context against the references of `pos`, twice with the same bits; trial_obs: what the accepted trial that
    led here gave, which the evaluation reproduces to `rel` per component"""
    S.energy()
    first = L.snapshot(S)
    against_references(S, S.observables, rung, cfg, pos, label, dipoles=True)
    if trial_obs is not None:
        bad = util.component_errors(trial_obs, S.observables, util.TRIAL_KEYS, rel)
        assert not bad, f"{label}: the accepted trial against the evaluation behind it (rel {rel}): " + "; ".join(bad)
    S.energy()
    assert L.same_bits(first, L.snapshot(S)), f"{label}: a second evaluation gives other bits"


# ---- (a) configuration x box sequences ----------------------------------------------------------------------------------------------------------
SEQUENCE_CASES = [(rung, cfg) for rung in (257,) + C.SLABS for cfg in C.sequence_configs(rung)]


@pytest.mark.parametrize("rung,cfg", SEQUENCE_CASES)
def test_sequence(rung, cfg):
    """energy(); a one-molecule move rejected; one in another part of the list accepted, whose store pass also repairs the rejected tile;
    65 atoms accepted; one frozen atom rejected; energy(), held to the references of the accumulated positions"""
    pos = B.box(rung)[0]["pos"].copy()
    S = make(rung, cfg)
    try:
        S.energy()
        against_references(S, S.observables, rung, cfg, pos, f"{rung} {cfg} start", dipoles=True)
        last = None
        for label, first, new, take in C.sequence(rung):
            label = f"{rung} {cfg} {label}"
            full = trial(S, rung, cfg, pos, first, new, label)
            if take:
                last = accept(S, rung, cfg, full, label)
                pos = full
            else:
                S.reject()
        evaluated(S, rung, cfg, pos, f"{rung} {cfg} the evaluation behind the sequence", last)
    finally:
        S.close()


# ---- (b) eight tiles exactly, and nine ------------------------------------------------------------------------------------------------------------
LARGE_CASES = [(rung, cfg, 0) for rung in sorted(C.LARGE) for cfg in C.EIGHT_TILE_CONFIGS] + [(rung, cfg, 1) for rung in sorted(C.LARGE) for cfg in ("jac_compact", "gs")]


@pytest.mark.parametrize("rung,cfg,sort", LARGE_CASES)
def test_large_moves(rung, cfg, sort):
    """The first large move rejected (tiles 0 to 4 of the list order), the second accepted (4 to 7 at 512 atoms: with the tiles left
    behind exactly eight, the restricted pass at its limit; 5 to 8 at 513 atoms: nine, the unrestricted pass), then one atom of tile 0 and
    one of tile 7 accepted, whose passes rebuild one tile's pairs and rely on every other pair being the accepted geometry's.  In list order
    (sort 0) the tiles are the blocks the CPU file reasoned about; with the spatial order the references alone decide."""
    pos = B.box(rung)[0]["pos"].copy()
    S = make(rung, cfg, sort)
    try:
        S.energy()
        assert S.tile_stats()["tile_pairs"] == (36 if rung == 512 else 45)
        last = None
        for k, (first, new, take) in enumerate(C.large_moves(rung)):
            label = f"{rung} {cfg} sort {sort} move {k} ({len(new)} atoms)"
            full = trial(S, rung, cfg, pos, first, new, label)
            if take:
                last = accept(S, rung, cfg, full, label)
                pos = full
            else:
                S.reject()
        evaluated(S, rung, cfg, pos, f"{rung} {cfg} sort {sort} the evaluation behind the moves", last)
    finally:
        S.close()


# ---- (c) class flips on both slabs -------------------------------------------------------------------------------------------------------------------
FLIP_CASES = [(rung, cfg, sort) for rung in C.SLABS for cfg in C.FLIP_CONFIGS for sort in (0, 1) if sort == 0 or not C.keeps_list_order(cfg)]
# (Gauss-Seidel sweeps keep the list order whatever the switch says: one run)


def far_beyond(st):
    return st["thole_far"], st["beyond_cutoff"]


@pytest.mark.parametrize("rung,cfg,sort", FLIP_CASES)
def test_long_jump_flips_classes(rung, cfg, sort):
    """One atom of tile 4 of the list order jumps to the vacant site of the top layer and back: the tile pairs of its tile with the tiles
    of the top layers need stored tensors they never had, and lose them again; between a reject and the next pair pass the device holds
    the rejected geometry's classes, panel table and bounds, which the next pass must not read"""
    listed = sort == 0 or C.keeps_list_order(cfg)
    P, site, nudge = C.flip_positions(rung)
    S = make(rung, cfg, sort)
    try:
        S.energy()
        st0 = S.tile_stats()
        against_references(S, S.observables, rung, cfg, P["start"], f"{rung} {cfg} sort {sort} start", dipoles=True)
        assert st0["tile_pairs"] == 171
        # 2. the long jump
        trial(S, rung, cfg, P["start"], C.JUMPER, site, f"{rung} {cfg} sort {sort} long jump")
        st = S.tile_stats()
        print(f"{rung} {cfg} sort {sort}: tile stats {st0} -> under the long jump {st}")
        if listed:
            assert st0["thole_far"] - st["thole_far"] >= 3 and st0["beyond_cutoff"] - st["beyond_cutoff"] >= 3, (st0, st)
        else:
            assert far_beyond(st) != far_beyond(st0), ("the long jump flips no class under the spatial order: the test exercises nothing", st0, st)
        # 3. rejected; a bystander far from both ends, accepted
        S.reject()
        label = f"{rung} {cfg} sort {sort} bystander behind the rejected jump"
        full = trial(S, rung, cfg, P["start"], C.BYSTANDER, nudge, label)
        accept(S, rung, cfg, full, label)
        if listed:
            assert far_beyond(S.tile_stats()) == far_beyond(st0), (st0, S.tile_stats())
        # 4. the long jump again, accepted
        label = f"{rung} {cfg} sort {sort} long jump, accepted"
        full = trial(S, rung, cfg, P["nudged"], C.JUMPER, site, label)
        got = accept(S, rung, cfg, full, label)
        evaluated(S, rung, cfg, P["nudged_jumped"], f"{rung} {cfg} sort {sort} the evaluation behind the jump", got)
        if listed:
            F = make(rung, cfg, sort, pos=P["nudged_jumped"])
            try:
                F.energy()
                assert S.tile_stats() == F.tile_stats(), (S.tile_stats(), F.tile_stats())
            finally:
                F.close()
        # 5. back to the original site: rejected, then accepted
        home = P["nudged"][C.JUMPER:C.JUMPER + 1]
        totals = []
        for take in (False, True):
            label = f"{rung} {cfg} sort {sort} jump back, {'accepted' if take else 'rejected'}"
            full = trial(S, rung, cfg, P["nudged_jumped"], C.JUMPER, home, label)
            totals.append(dict(S.trial_observables))
            if take:
                accept(S, rung, cfg, full, label)
            else:
                S.reject()
        evaluated(S, rung, cfg, P["nudged"], f"{rung} {cfg} sort {sort} the evaluation behind the jump back", totals[1])
        for t in totals:
            bad = util.component_errors(t, S.observables, util.TRIAL_KEYS, 1e-10)
            assert not bad, f"{rung} {cfg} sort {sort}: the trials of the jump back against the evaluation (rel 1e-10): " + "; ".join(bad)
        if listed:
            assert far_beyond(S.tile_stats()) == far_beyond(st0), (st0, S.tile_stats())
    finally:
        S.close()


@pytest.mark.parametrize("rung,cfg,sort", FLIP_CASES)
def test_lattice_hop(rung, cfg, sort):
    """One atom of a middle tile displaced by exactly one cell vector: the wrapped coordinates and all physics are unchanged, the tile's raw
    coordinate range spans a cell, so its tile pairs lose the common periodic image along the hop"""
    axis = C.hop_axis(cfg, sort)
    i, new, ph, (a, nw) = C.hop_positions(rung, axis)
    p0 = B.box(rung)[0]["pos"]
    keys = ("nonuniform_dims_x_pairs_stored", "nonuniform_dims_x_pairs_far")
    S = make(rung, cfg, sort)
    try:
        S.energy()
        before = S.pair_stats()
        start = dict(S.observables)
        label = f"{rung} {cfg} sort {sort} hop along {axis}"
        full = trial(S, rung, cfg, p0, i, new, label)
        bad = util.component_errors(S.trial_observables, start, util.TRIAL_KEYS, FRESH_REL)
        assert not bad, f"{label}: against the configuration before the hop (rel {FRESH_REL}): " + "; ".join(bad)
        for k in ("n_lj_in_cutoff", "n_es_in_cutoff", "polar_iterations"):
            assert S.trial_observables[k] == start[k], (label, k)
        after = S.pair_stats()
        print(f"{label}: non-uniform dimensions x pairs {[before[k] for k in keys]} -> {[after[k] for k in keys]}")
        assert sum(after[k] for k in keys) > sum(before[k] for k in keys), (before, after)
        accept(S, rung, cfg, full, label)
        label = f"{rung} {cfg} sort {sort} one molecule behind the hop"
        full = trial(S, rung, cfg, ph, a, nw, label)
        got = accept(S, rung, cfg, full, label)
        evaluated(S, rung, cfg, full, f"{rung} {cfg} sort {sort} the evaluation behind the hop", got)
    finally:
        S.close()
