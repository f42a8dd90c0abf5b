"""GPU (MI355X): every kernel that forms a periodic image, on crystal lattices (thousands of pairs exactly on a half-cell tie) and in
strongly skewed cells (60 and 120 degree angles, the fcc primitive cell), held to the image the reference takes:
rint(((0 + R[0][p] d0) + R[1][p] d1) + R[2][p] d2), which at a tie is decided by the last bit of that unfused sum and in a skewed cell is
not the nearest image.  Boxes: tests/lattice_tie_boxes.py; what they hold, in numbers: tests/test_lattice_tie_preconditions.py.

Yardsticks and bounds are the suite's own, none is new: util.assert_matches_oracle (energies at util.REL_TOL with no floor, counts to
the bit, the per-atom fields) where the oracle has the solve; the restatements polar_direct_ref, polar_gs_ranked_ref,
polar_ewald_full_ref, polar_relax_ref and polar_wolf_ref with the bounds of their own GPU files elsewhere (all of them take the
reference's image: test_lattice_tie_preconditions.test_the_restatements_take_the_reference_image); util.check_trial_against_oracle for
the trial moves.  Run with -s for the largest deviation per test.

What failed before its fix, on the library of the commit before: `compact` in every non-orthorhombic cell from four tiles on -- the panel
contraction (kernels_panel.hip, pan_step) rounded a fused sum of the pre-shifted displacement, and contracted the pairs on a tie with a
displacement of another image than the one their stored tensor was made for.
"""
import ctypes

import numpy as np
import pytest

import util
import lattice_tie_boxes as B
import polar_direct_ref
import polar_gs_ranked_ref
import polar_ragged_boxes as PR
import test_gpu_polar_gs_ranked as GSR
import test_gpu_polar_ragged_ladder as RL
from mpmcxx_amd import energy

pytestmark = pytest.mark.gpu

CONST = util.ladder_constants()
TILE = CONST["kTile"]
SMALL, PANEL, LARGE = (B.SIZES[k] for k in ("small", "panel", "large"))
SEEN = {}


@pytest.fixture(scope="module", autouse=True)
def _need_device():
    if energy.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests need an MI355X")


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if SEEN:
        print("\nlargest deviation per test (energies: relative; fields: max_i |d_i| / allowed_i, 1 = the bound):")
        for label, d in SEEN.items():
            print(f"  {label}: " + ", ".join(f"{k} {v:.1e}" for k, v in d.items() if v))


def panel_table(S):
    """the work table of the panel kernel of the last evaluation, [entries, 4] = {tile pair A, tile pair B or -1, flags, J}; no rows
    unless the evaluation built one (mpmc_debug_panel_table)"""
    fn = energy.lib().mpmc_debug_panel_table
    fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    tab = np.zeros((20000, 4), dtype=np.int32)
    n = fn(S.handle, tab.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), len(tab))
    assert n >= 0
    return tab[:n][tab[:n, 0] >= 0]


# ---- 1. full evaluation ------------------------------------------------------------------------------------------------------------------
# the solves the oracle has: (options on top of B.OPTIONS, configure switches).  `sweep`: the pair sweep switched on below its size
# threshold (kSweepMinPairs tile pairs are 64 tiles; no box here may hold 2 000 atoms), as test_gpu_pair_sweep does
ORACLE_SOLVES = {"compact": dict(solver="compact"), "matrix_free": dict(solver="matrix_free"), "dense": dict(solver="dense"),
                 "polar_gs": dict(polar_gs=1), "nopbc_field": dict(polar_ewald=0)}
FULL = ([(c, PANEL, v, s) for c in B.CELLS for v in B.VARIANTS for s in ORACLE_SOLVES] +
        [(c, G, v, s) for c in B.CELLS for G in (SMALL, LARGE) for v in B.VARIANTS for s in ("compact", "matrix_free")] +
        [(c, PANEL, v, s) for c in B.SLABS for v in B.VARIANTS for s in ("compact", "matrix_free")])


def oracle_changes(solve):
    return {k: v for k, v in ORACLE_SOLVES[solve].items() if k != "solver"}


@pytest.mark.parametrize("cell,G,variant,solve", FULL)
def test_full_evaluation_against_the_oracle(cell, G, variant, solve):
    atoms, basis, opts, _ = B.box(cell, G, variant)
    o = dict(opts, **ORACLE_SOLVES[solve])
    ref = B.oracle(cell, G, variant, **oracle_changes(solve))
    label = f"{cell} G={G} {variant} {solve}"
    sweep = B.by_region(cell, G) and solve == "compact"  # (the boxes whose tiles have classes: lattice_tie_boxes.by_region)
    if sweep:
        energy.configure("pair_kernel", 2)
    if cell in B.SLABS:  # in list order: the tiles are slices of the slab (below kSortGridMinTiles tiles the spatial order cuts columns along c)
        energy.configure("spatial_sort", 0)
    try:
        S = energy.System(atoms, basis, o)
    finally:
        energy.configure("pair_kernel", 0)
        energy.configure("spatial_sort", 1)
    try:
        S.energy()
        util.assert_matches_oracle(S.observables, S.dipoles(), ref, atoms, o, label=label, deviations=SEEN.setdefault(label, {}))
        nt = B.n_tiles(atoms, TILE)
        assert S.tile_stats()["tile_pairs"] == nt * (nt + 1) // 2
        if solve == "compact":
            tab = panel_table(S)
            assert (len(tab) > 0) == (nt >= 3) and S.memory_usage()[1] > 0, (label, nt, len(tab))  # the panel kernel ran on the stored tensors
        if sweep:
            assert S.last_pair_kernel() == "sweep", label
            ps = S.pair_stats()
            masks = sorted(set((tab[:, 2] & 15).tolist()))
            print(f"\n{label}: {ps}, panel masks (common directions | 8 far) {masks}")
            # the classifier at work, or this box did not exercise it: tile pairs beyond the damping range; stored tile pairs with a common
            # image index in some directions (fewer than three indices to round per pair, on average) next to tile pairs without one.
            # In a cell of three tiles per edge two tiles beyond the damping range lie about half a cell apart in every direction, so
            # they have no common index; the slabs have far-field panels with a common index along c only, and tile pairs beyond the cutoff
            assert ps["tile_pairs_far"] > 0 and ps["pairs_far"] > 0, (label, ps)
            assert 0 < ps["nonuniform_dims_x_pairs_stored"] < 3 * ps["pairs_stored"], (label, ps)
            assert 0 < ps["nonuniform_dims_x_pairs_swept"] < 3 * ps["pairs_swept"], (label, ps)
            assert any(m & 8 for m in masks) and any(not m & 8 and (m & 7) not in (0, 7) for m in masks), (label, masks)
            if cell in B.SLABS:
                assert ps["tile_pairs_beyond_cutoff"] > 0, (label, ps)
                assert 0 < ps["nonuniform_dims_x_pairs_far"] < 3 * ps["pairs_far"], (label, ps)
                assert any(m & 8 and (m & 7) not in (0, 7) for m in masks), (label, masks)
    finally:
        S.close()


# the solves the oracle does not have, against their restatements: polar_ragged_boxes' variants (polar_ewald_full, polar_sor, polar_zodid,
# polar_wolf with polar_gs and polar_palmo) with test_gpu_polar_ragged_ladder's comparison, the ranked Gauss-Seidel sweeps and the direct solve
RESTATED = ("pef", "jac_sor", "zodid", "wolf_gsp", "gs_ranked", "direct")
_fields, _nonpolar = {}, {}


def restated_options(opts, solve):
    if solve == "gs_ranked":
        return dict(opts, polar_gs_ranked=1, polar_max_iter=3)
    if solve == "direct":
        return dict(opts, polar_iterative=0)
    return dict(opts, **PR.VARIANTS[solve])


def static_field_of(cell, G, variant, o):
    key = (cell, G, variant, "wolf" if o.get("polar_wolf") and not o["polar_ewald"] else "ewald")
    if key not in _fields:
        atoms, basis, _, _ = B.box(cell, G, variant)
        _fields[key] = PR.static_field(atoms, basis, o)
    return _fields[key]


def oracle_without_polarization(cell, G, variant):
    if (cell, G, variant) not in _nonpolar:
        atoms, basis, opts, _ = B.box(cell, G, variant)
        _nonpolar[cell, G, variant] = util.oracle_energy(atoms, basis, util.nonpolar(opts))
    return _nonpolar[cell, G, variant]


@pytest.mark.parametrize("solve", RESTATED)
@pytest.mark.parametrize("variant", B.VARIANTS)
@pytest.mark.parametrize("cell", B.CELLS)
def test_full_evaluation_against_the_restatements(cell, variant, solve):
    atoms, basis, opts, _ = B.box(cell, PANEL, variant)
    o = restated_options(opts, solve)
    label = f"{cell} G={PANEL} {variant} {solve}"
    S = energy.System(atoms, basis, o)
    try:
        S.energy()
        obs = S.observables
        mu, E0, F = S.dipoles()
        if solve == "gs_ranked":
            want = polar_gs_ranked_ref.solve(atoms, basis, o)
            assert obs["polar_iterations"] == want["polar_iterations"] and obs["iterator_failed"] == want["iterator_failed"] == 0
            dev = abs(obs["polarization_energy"] - want["polarization_energy"]) / abs(want["polarization_energy"])
            assert dev <= GSR.REF_REL_E, (label, obs["polarization_energy"], want["polarization_energy"])
            seen = {"energy": dev}
            for k, got in (("ef_static", E0), ("mu", mu), ("ef_induced", F)):
                bad, ratio, _ = util.field_errors(got, want[k], GSR.REF_REL_MU, 1e-12)
                seen[k] = ratio
                assert bad.size == 0, (label, k, ratio)
            GSR.against_rank_pass(S, atoms, basis, want["ranked_sweeps"], label)
            SEEN[label] = seen
            floor_e = 0.0
        elif solve == "direct":
            want = polar_direct_ref.solve(atoms, basis, o)
            info = S.direct_info()
            assert info["status"] == 0 and obs["iterator_failed"] == 0 and info["n_unknowns"] == 3 * int((atoms["polarizability"] != 0).sum())
            bad, ratio, _ = util.field_errors(E0, want["ef_static"])
            assert bad.size == 0, (label, "ef_static", ratio)
            top = np.abs(want["mu"]).max()
            dev_mu = np.abs(mu - want["mu"]).max() / top
            assert dev_mu <= util.REL_TOL, (label, dev_mu)
            assert util.close(obs["polarization_energy"], want["polarization_energy"]), (label, obs["polarization_energy"], want["polarization_energy"])
            SEEN[label] = {"ef_static": ratio, "mu": dev_mu,
                           "energy": abs(obs["polarization_energy"] - want["polarization_energy"]) / abs(want["polarization_energy"])}
            floor_e = 0.0
        else:
            E = static_field_of(cell, PANEL, variant, o)
            want = PR.solve(solve, atoms, basis, o, E)
            pef_box = {"n_real_pairs": want["n_real_pairs"], "n_k": want["n_k"]} if o.get("polar_ewald_full") else None
            floor_e = RL.against_the_restatement(S, atoms, o, solve, want, label, pef_box)
        RL.against_the_oracle_without_polarization(S, oracle_without_polarization(cell, PANEL, variant), want["polarization_energy"], floor_e, label)
    finally:
        S.close()


# ---- 2. energies-only evaluation: the one-stream in-flight plan, the energy from the moments ------------------------------------------------
def bead_atoms(atoms, basis, info, b):
    """bead b: a seeded quarter of the lattice atoms another whole cell away along each lattice vector (the ties stay ties, at other k)"""
    rng = np.random.default_rng(900 + b)
    nl = info["n_lattice"]
    away = np.where((rng.random(nl) < 0.25)[:, None], rng.integers(-1, 2, size=(nl, 3)), 0)
    pos = atoms["pos"].copy()
    pos[:nl] += away @ basis
    return util.with_positions(atoms, pos)


@pytest.mark.parametrize("cell", B.CELLS)
def test_bead_ensemble_against_the_oracle_and_lone_evaluations(cell):
    atoms, basis, opts, info = B.box(cell, PANEL)
    lists = [bead_atoms(atoms, basis, info, b) for b in range(4)]
    beads = [energy.System(a, basis, opts) for a in lists]
    try:
        sums, per, failed = energy.pi_potential_local(beads)
        assert not failed
        per = [dict(p) for p in per]
        for b, (a, p) in enumerate(zip(lists, per)):
            ref = util.oracle_energy(a, basis, opts)
            label = f"{cell} bead {b}"
            bad = util.component_errors(p, ref, [k for k, _ in util.ENERGY_KEYS], util.REL_TOL)
            assert not bad, f"{label}: in the ensemble vs oracle: " + "; ".join(bad)
            for k in util.COUNT_KEYS + ["n_es_in_cutoff", "polar_iterations", "iterator_failed"]:
                assert int(p[k]) == int(ref[k]), (label, k, p[k], ref[k])
        for b, (S, p) in enumerate(zip(beads, per)):  # alone: the same bits
            S.energy()
            for k, _ in util.ENERGY_KEYS:
                assert S.observables[k] == p[k], (cell, b, k, S.observables[k], p[k])
            util.assert_matches_oracle(S.observables, S.dipoles(), util.oracle_energy(lists[b], basis, opts), lists[b], opts, label=f"{cell} bead {b} alone")
    finally:
        for S in beads:
            S.close()


# ---- 5. the image stays the reference's -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", B.VARIANTS)
@pytest.mark.parametrize("G", sorted(B.SIZES.values()))
@pytest.mark.parametrize("cell", B.SKEWED)
def test_the_image_stays_the_reference_one(cell, G, variant):
    """LJ + Ewald without polarization in the cells where a nearest-image search finds more pairs inside the cutoff than the reference
    (test_lattice_tie_preconditions counts them): the counts to the bit, the energies at REL_TOL, with the fused pair kernel and with the sweep"""
    atoms, basis, opts, _ = B.box(cell, G, variant)
    o = util.nonpolar(opts)
    ref = oracle_without_polarization(cell, G, variant)
    for kernel, name in ((1, "fused"), (2, "sweep")):
        energy.configure("pair_kernel", kernel)
        try:
            S = energy.System(atoms, basis, o)
        finally:
            energy.configure("pair_kernel", 0)
        try:
            S.energy()
            assert S.last_pair_kernel() == name
            label = f"{cell} G={G} {variant} {name}"
            util.assert_matches_oracle(S.observables, None, ref, atoms, o, label=label, deviations=SEEN.setdefault(label, {}))
        finally:
            S.close()


# ---- 3. the other terms that form an image ------------------------------------------------------------------------------------------------------
TERM_CELLS = ("tri_general", "hex60")
TERMS = ("axilrod_teller", "disp", "crystal", "rdm", "sg", "autoreject", "cavity_grid")


def term_case(cell, term):
    """(atoms, basis, opts) of the G = 6 crystal box of `cell` with one term on, as that term's own GPU file sets it up"""
    atoms, basis, opts, _ = B.box(cell, PANEL)
    n = len(atoms["charge"])
    rng = np.random.default_rng(77)
    if term == "axilrod_teller":
        atoms.update(c6=np.zeros(n), c9=rng.uniform(300.0, 1500.0, n))
        return atoms, basis, dict(util.nonpolar(opts), axilrod_teller=1)
    if term == "disp":  # epsilon and sigma are the term's alpha (1 / A) and r0 (A): the species A and B of gen_box.DISP_SPECIES
        a = np.arange(n) % 2 == 0
        atoms.update(epsilon=np.where(a, 3.10, 2.85), sigma=np.where(a, 3.45, 3.70), c6=np.where(a, 64.3, 129.6), c8=np.where(a, 1623.0, 4187.0),
                     c10=np.where(a, 49060.0, 155500.0), has_disp=np.ones(n, np.int32))
        return atoms, basis, {"rd_only": 1, "disp_expansion": 1, "damp_dispersion": 1}
    if term == "crystal":
        return atoms, basis, {"rd_only": 1, "rd_lrc": 1, "rd_crystal": 1, "rd_crystal_order": 2}
    if term == "rdm":
        return atoms, basis, {"rd_only": 1, "rd_lrc": 1, "halgren_mixing": 1, "lj_buffered_14_7": 1}
    if term == "sg":
        return atoms, basis, {"rd_only": 1, "sg": 1}
    if term == "autoreject":
        return atoms, basis, dict(util.nonpolar(opts), cavity_autoreject=1, cavity_autoreject_absolute=1, cavity_autoreject_scale=0.9)
    return atoms, basis, util.nonpolar(opts)


@pytest.mark.parametrize("term", TERMS)
@pytest.mark.parametrize("cell", TERM_CELLS)
def test_other_terms_against_their_restatements(cell, term):
    import cavity_autoreject_ref as CA
    import sg_ref
    import test_gpu_cavity as CAV
    import test_gpu_pair_term_walk as PTW
    import three_body_ref

    atoms, basis, o = term_case(cell, term)
    label = f"{cell} {term}"
    S = energy.System(atoms, basis, o)
    try:
        if term == "cavity_grid":  # exact integers: occupancy, open list, dart hits; the centres and the probability to the bit
            for G, radius in ((6, 2.0), (9, 2.6)):
                CAV.assert_update(S, basis, G, radius, CAV.darts_for(basis, seed=40 + G), f"{label} G={G} radius={radius}")
            return
        S.energy()
        r = S.observables
        if term == "axilrod_teller":
            want = three_body_ref.for_case(atoms, basis, o)
            dev = abs(r["three_body_energy"] - want) / abs(want)
            assert dev < 1e-11, (label, r["three_body_energy"], want)
            SEEN[label] = {"three_body_energy": dev}
        elif term == "sg":
            info = S.silvera_goldman_info()
            want = sg_ref.for_case(atoms, basis, o, cutoff=info["cutoff"], fast=True)
            assert abs(r["rd_energy"] - want["rd"]) <= 1e-12 * want["mag"], (label, r["rd_energy"], want)
            assert info["n_terms"] == want["n_terms"] > 0, (label, info, want)
            SEEN[label] = {"rd_energy / summed magnitudes": abs(r["rd_energy"] - want["rd"]) / want["mag"]}
        elif term == "autoreject":
            want = CA.counts(atoms, basis, o, *CA.rules_of(o))
            info = S.cavity_autoreject_info()
            assert want["n_replaced"] > 0, (label, want["n_replaced"])  # (sigma_ij up to 3.2 A at 0.9 against contacts from 2.35 A on)
            for k in ("n_replaced", "n_absolute", "n_unmeasured_frozen"):
                assert info[k] == want[k], (label, k, info[k], want[k])
        else:
            key = {"disp": "disp", "crystal": "crystal", "rdm": "rdm"}[term]
            want = PTW.restated(key, atoms, basis, o)
            PTW.check_sum(key, PTW.result_bits(r), PTW.info_of(key, S), want, label)
            SEEN[label] = {"lj_pairs / summed magnitudes": abs(r["lj_pairs"] - want["lj_pairs"]) / want["mag"]}
    finally:
        S.close()


# ---- 4. trial moves --------------------------------------------------------------------------------------------------------------------------
import volume_trial_cases as VC  # noqa: E402

TRIAL_CELLS = ("tri_general", "hex60", "ortho")
TRIAL_SOLVES = ("nonpolar", "compact", "matrix_free")
COUNT_KEYS = ("n_lj_in_cutoff", "n_es_in_cutoff")


def trial_box(cell, solve):
    atoms, basis, opts, info = B.box(cell, PANEL)
    return atoms, basis, (util.nonpolar(opts) if solve == "nonpolar" else dict(opts, solver=solve)), info


def on_site(atoms, mol_range, site):
    """the molecule [first, end) moved rigidly so that its first atom sits on `site`"""
    first, end = mol_range
    return atoms["pos"][first:end] + (site - atoms["pos"][first])


def evaluation_matches(S, atoms, basis, o, label):
    S.energy()
    polar = bool(o.get("polarization"))
    util.assert_matches_oracle(S.observables, S.dipoles() if polar else None, util.oracle_energy(atoms, basis, o), atoms, o, label=label)


@pytest.mark.parametrize("solve", TRIAL_SOLVES)
@pytest.mark.parametrize("cell", TRIAL_CELLS)
def test_displacement_onto_a_vacant_lattice_site_and_off_again(cell, solve):
    """a sorbate's first atom lands exactly on a vacant site two cells away from the home cell (ties at 1.5 and 2.5 with the lattice), the
    move is accepted, and the molecule moves back: every trial and both accepted configurations against the oracle"""
    atoms, basis, o, info = trial_box(cell, solve)
    mol = info["sorbates"][0]
    first, end = mol
    site = info["vacant"][0] + np.array([2.0, -1.0, 1.0]) @ basis
    home = atoms["pos"][first:end].copy()
    S = energy.System(atoms, basis, o)
    try:
        S.energy()
        pos = atoms["pos"].copy()
        for step, new in (("onto the site", on_site(atoms, mol, site)), ("off again", home)):
            S.trial_energy(first, new)
            pos = pos.copy()
            pos[first:end] = new
            util.check_trial_against_oracle(S.trial_observables, atoms, basis, o, pos, label=f"{cell} {solve} {step}")
            S.accept()
            evaluation_matches(S, util.with_positions(atoms, pos), basis, o, f"{cell} {solve} accepted {step}")
    finally:
        S.close()


@pytest.mark.parametrize("solve", TRIAL_SOLVES)
@pytest.mark.parametrize("cell", TRIAL_CELLS)
def test_insertion_at_a_vacant_site_and_removal_of_a_lattice_atom(cell, solve):
    atoms, basis, o, info = trial_box(cell, solve)
    first, end = info["sorbates"][0]
    mol = {k: np.array(v[first:end]) for k, v in atoms.items()}
    mol["pos"] = on_site(atoms, (first, end), info["vacant"][1])
    S = energy.System(atoms, basis, o, max_atoms=len(atoms["charge"]) + 8)
    try:
        S.energy()
        S.trial_insert_energy(S.n, mol)
        grown = VC.appended(atoms, mol)
        util.check_trial_against_oracle(S.trial_observables, grown, basis, o, grown["pos"], label=f"{cell} {solve} insertion")
        S.reject()
        k = info["n_lattice"] // 2  # a lattice atom: in the crystal variant a molecule of its own
        S.trial_remove_energy(k, 1)
        less = VC.without(atoms, k, k + 1)
        util.check_trial_against_oracle(S.trial_observables, less, basis, o, less["pos"], label=f"{cell} {solve} removal")
        S.accept()
        evaluation_matches(S, less, basis, o, f"{cell} {solve} after the removal")
    finally:
        S.close()


@pytest.mark.parametrize("cell", TRIAL_CELLS)
def test_insertion_candidates_at_all_vacant_sites_equal_the_single_trials(cell):
    """mpmc_insert_candidates has the delta path only (no polarizable box): LJ + Ewald.  One batch with a pose on every vacant site, each
    entry the single trial's bits; the first three single trials against the oracle"""
    atoms, basis, o, info = trial_box(cell, "nonpolar")
    assert VC.candidates_allowed(o)
    first, end = info["sorbates"][0]
    mol = {k: np.array(v[first:end]) for k, v in atoms.items()}
    poses = np.stack([on_site(atoms, (first, end), site) for site in info["vacant"]])
    S = energy.System(atoms, basis, o, max_atoms=len(atoms["charge"]) + 8)
    try:
        S.energy()
        batch = S.insert_candidates(mol, poses)
        assert len(batch) == len(info["vacant"]) >= 40
        for c, pose in enumerate(poses):
            one = dict(mol, pos=pose)
            S.trial_insert_energy(S.n, one)
            single = dict(S.trial_observables)
            if c < 3:
                grown = VC.appended(atoms, one)
                util.check_trial_against_oracle(single, grown, basis, o, grown["pos"], label=f"{cell} candidate {c}")
            S.reject()
            for k in util.TRIAL_KEYS + list(COUNT_KEYS):
                assert batch[c][k] == single[k], (cell, c, k, batch[c][k], single[k])
    finally:
        S.close()


@pytest.mark.parametrize("accept", (False, True))
@pytest.mark.parametrize("scale", (0.98, 1.03))
@pytest.mark.parametrize("solve", TRIAL_SOLVES)
@pytest.mark.parametrize("cell", TRIAL_CELLS)
def test_volume_trial(cell, solve, scale, accept):
    atoms, basis, o, _ = trial_box(cell, solve)
    S = energy.System(atoms, basis, o)
    try:
        S.energy()
        before = dict(S.observables)
        S.trial_volume_energy(scale)
        sa, sb = VC.scaled(atoms, basis, scale)
        util.check_trial_against_oracle(S.trial_observables, sa, sb, o, sa["pos"], label=f"{cell} {solve} volume x {scale}")
        if accept:
            S.accept()
            evaluation_matches(S, sa, sb, o, f"{cell} {solve} accepted volume x {scale}")
        else:
            S.reject()
            S.energy()
            for k, _ in util.ENERGY_KEYS:
                assert S.observables[k] == before[k], (cell, solve, scale, k)
    finally:
        S.close()


# ---- 6. the margins of the uniform-image test ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solve", ("compact", "matrix_free"))
@pytest.mark.parametrize("cell", B.LAYERS)
def test_tile_pairs_whose_extreme_is_a_tie(cell, solve):
    """The layered boxes in list order: every tile is one lattice layer, and two tile pairs half a cell apart along c pass k_classify's
    uniform-image test only with the margin at 0, with an index that all 4 096 of their pairs round away from
    (test_lattice_tie_preconditions.test_a_tile_pair_whose_extreme_is_a_tie_needs_the_margin).  They lie beyond the damping range: under
    `compact` the far-field walk of the panel contraction takes whatever index the classes call common."""
    atoms, basis, opts, _ = B.box(cell, B.G_LAYERS)
    o = dict(opts, solver=solve)
    label = f"{cell} {solve}"
    energy.configure("pair_kernel", 2)
    energy.configure("spatial_sort", 0)
    try:
        S = energy.System(atoms, basis, o)
    finally:
        energy.configure("pair_kernel", 0)
        energy.configure("spatial_sort", 1)
    try:
        S.energy()
        util.assert_matches_oracle(S.observables, S.dipoles(), B.oracle(cell, B.G_LAYERS), atoms, o, label=label, deviations=SEEN.setdefault(label, {}))
        assert S.last_pair_kernel() == "sweep"
        if solve == "compact":
            masks = sorted(set((panel_table(S)[:, 2] & 15).tolist()))
            ps = S.pair_stats()
            print(f"\n{label}: {ps}, panel masks (common directions | 8 far) {masks}")
            # far-field panels whose only common index is the one along c, next to far-field panels without one (the pairs on the tie)
            assert 8 | 4 in masks and 8 in masks and ps["tile_pairs_beyond_cutoff"] > 0, (label, masks, ps)
    finally:
        S.close()
