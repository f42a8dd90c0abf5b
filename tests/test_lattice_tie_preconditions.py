"""CPU: what makes the comparisons of tests/test_gpu_lattice_ties.py mean something.  The boxes of tests/lattice_tie_boxes.py must hold
the half-cell ties and the not-nearest images they are built for, in numbers, and the oracle's answer on them must be well defined:

  - at least 100 tie components per lattice direction (||f| - (k + 1/2)| < 1e-9 with f the reference's own sum), k = 1 and k = 2 among them;
  - in every non-orthorhombic box at least 20 tie components whose image index moves when the three-term sum is fused
    (rint(fma(R2, d2, fma(R1, d1, R0 d0))), computed from exact rationals with one rounding per fma): a kernel that fuses the sum of
    a predicate-free walk contracts such a pair with a displacement of another image than the one its stored tensor was made for;
  - in the 60 degree, 120 degree and rhombohedral cells at least 50 pairs whose nearest image (27 images, brute force) lies inside the
    cutoff while the image the reference takes lies outside: a nearest-image search would count them;
  - no two atoms of different molecules closer than 2.3 A (nearest image), finite oracle energies, no atom whose static field is a
    rounding residue (at least 1e-3 of max|q| / d_nn^2, so that the standard per-atom bounds of util.assert_matches_oracle apply as they
    stand), and the oracle's pair counts equal to a numpy restatement of the rint image and the two cutoff predicates;
  - the sizes sit where the launch paths switch (util.ladder_constants).
R, the volume and the cutoff are the oracle's (orc_pbc_update).  Run with -s for the counts.
"""
import numpy as np
import pytest

import util
import lattice_tie_boxes as B
from oracle import pbc_update

BOXES = [(name, G) for name in B.CELLS for G in B.SIZES.values()] + [(name, B.SIZES["panel"]) for name in B.SLABS]
CONST = util.ladder_constants()
SAMPLE = 6000  # tie components per direction that get the exact-rational fused sum (all of them up to G = 6)


def geometry(name, G):
    atoms, basis, _, info = B.box(name, G)
    R, vol, cut = pbc_update(basis)
    return atoms, basis, info, R, vol, cut


def test_sizes_sit_on_the_launch_paths():
    """two tiles (no panel table: it starts at three), four tiles (the smallest with one), and a box of more tile pairs than any other
    lattice box of the suite that still stays under 2 000 atoms.  All three lie at or below kSingleLaunchTiles and below kSweepMinPairs
    tile pairs (64 tiles, 4 033 atoms): the GPU file switches the pair sweep on for the large box (pair_kernel = 2), as test_gpu_pair_sweep does."""
    tile = CONST["kTile"]
    sweep_tiles = util.size_ladder()["sweep"][1]
    for name in B.CELLS:
        nt = {size: B.n_tiles(B.box(name, G)[0], tile) for size, G in B.SIZES.items()}
        n_large = len(B.box(name, B.SIZES["large"])[0]["charge"])
        assert nt["small"] == 2 and nt["panel"] == 4 and 16 < nt["large"] <= CONST["kSingleLaunchTiles"], (name, nt)
        assert nt["large"] < sweep_tiles and n_large < 2000 < tile * (sweep_tiles - 1), (name, nt, n_large, sweep_tiles)
        assert nt["large"] * (nt["large"] + 1) // 2 <= CONST["kOneStreamMaxPairs"], (name, nt)
    for name in B.SLABS:
        assert 8 <= B.n_tiles(B.box(name, B.SIZES["panel"])[0], tile) <= 10, name


@pytest.mark.parametrize("name,G", BOXES)
def test_ties_in_every_lattice_direction(name, G):
    atoms, basis, info, R, vol, cut = geometry(name, G)
    assert vol > 0
    if name == "tri_general":
        assert np.all(basis != 0.0), basis
    _, _, d = B.pair_displacements(atoms)
    ties = B.tie_components(d, R)
    print(f"\n{name} G = {G}: {len(atoms['charge'])} atoms, tie components per direction " + " / ".join(str(len(h)) for h, _ in ties))
    for p, (hit, k) in enumerate(ties):
        assert len(hit) >= 100, (name, G, p, len(hit))
        assert np.any(k == 1) and np.any(k == 2), (name, G, p, sorted(set(k.tolist())))


@pytest.mark.parametrize("name,G", [b for b in BOXES if b[0] in B.TRICLINIC + B.SLABS])
def test_a_fused_sum_takes_another_image_at_some_ties(name, G):
    atoms, basis, info, R, vol, cut = geometry(name, G)
    _, _, d = B.pair_displacements(atoms)
    rng = np.random.default_rng(G)
    counts, looked = [], []
    for p, (hit, _) in enumerate(B.tie_components(d, R)):
        if len(hit) > SAMPLE:
            hit = np.sort(rng.choice(hit, size=SAMPLE, replace=False))
        counts.append(int(B.fused_index_differs(d[hit], R, p).sum()))
        looked.append(len(hit))
    print(f"\n{name} G = {G}: fused index differs from the reference's at " + " / ".join(f"{c} of {n}" for c, n in zip(counts, looked)) + " tie components")
    assert sum(counts) >= 20, (name, G, counts, looked)


@pytest.mark.parametrize("name,G", [b for b in BOXES if b[0] in B.SKEWED])
def test_the_reference_image_is_not_the_nearest_one(name, G):
    atoms, basis, info, R, vol, cut = geometry(name, G)
    lengths = np.linalg.norm(basis, axis=1)
    spacing = 1.0 / np.linalg.norm(R, axis=0)  # plane spacing of lattice direction p = 1 / |column p of R|
    assert cut == pytest.approx(0.5 * lengths.min(), rel=1e-12) and spacing.min() < 0.9 * lengths.min(), (cut, lengths, spacing)
    count = B.nearer_image_pairs(atoms, basis, R, cut)
    print(f"\n{name} G = {G}: cutoff {cut:.3f}, plane spacings {spacing.round(3).tolist()}, {count} pairs with a nearer image inside the cutoff than the reference's")
    assert count >= 50, (name, G, count)


@pytest.mark.parametrize("variant", B.VARIANTS)
@pytest.mark.parametrize("name,G", BOXES)
def test_the_oracle_answer_is_well_defined(name, G, variant):
    atoms, basis, opts, info = B.box(name, G, variant)
    R, vol, cut = pbc_update(basis)
    i, j, d = B.pair_displacements(atoms)
    near = B.nearest_image_distances(d, basis)
    inter = atoms["mol_id"][i] != atoms["mol_id"][j]
    assert near[inter].min() >= B.MIN_DIST, (name, G, variant, near[inter].min())
    # the vacant sites the trial moves fill are as far from everything as the occupied ones
    dv = B.nearest_image_distances(info["vacant"][:, None, :] - atoms["pos"][None, :, :], basis)
    assert dv.min() >= B.MIN_DIST, (name, G, dv.min())
    ref = B.oracle(name, G, variant)
    for k, _ in util.ENERGY_KEYS:
        assert np.isfinite(ref[k]), (name, G, variant, k, ref[k])
    assert ref["polarization_energy"] < 0.0 and ref["iterator_failed"] == 0 and ref["polar_iterations"] == opts["polar_max_iter"]
    # every atom's static field is a sum that does not cancel: the nearest neighbour's field q / d_nn^2 is its largest term
    e = np.abs(ref["ef_static"]).max(axis=1)
    s_nn = float(np.abs(atoms["charge"]).max() / near[inter].min() ** 2)
    print(f"\n{name} G = {G} {variant}: min |E_i| / (max|q| / d_nn^2) = {e.min() / s_nn:.2e}, d_nn {near[inter].min():.3f}")
    assert e.min() >= 1e-3 * s_nn, (name, G, variant, e.min(), s_nn)
    assert np.all(np.isfinite(ref["mu"])) and np.abs(ref["mu"]).max() > 0.0
    want = B.restated_counts(atoms, basis, R, cut)
    got = {k: int(ref[k]) for k in want}
    assert got == want, (name, G, variant, got, want)
    if variant == "framework":
        assert want["n_frozen"] == info["n_lattice"] * (info["n_lattice"] - 1) // 2


def test_the_restatements_take_the_reference_image():
    """polar_direct_ref.minimum_image (which polar_relax_ref and polar_wolf_ref import) against the oracle's orc_minimum_image on the
    ties of a skewed box, displacement by displacement, to the bit"""
    import polar_direct_ref
    from oracle import OracleSystem

    for name in ("tri_general", "rhombo"):
        atoms, basis, opts, _ = B.box(name, B.SIZES["panel"])
        O = OracleSystem(atoms, basis, opts)
        d = polar_direct_ref.minimum_image(atoms["pos"], basis)
        _, _, raw = B.pair_displacements(atoms)
        i, j = np.triu_indices(len(atoms["pos"]), 1)
        for p, (hit, _) in enumerate(B.tie_components(raw, O.recip)):
            for n in hit[:400]:
                _, want, _ = O.minimum_image(int(i[n]), int(j[n]))
                assert np.array_equal(d[i[n], j[n]], want), (name, p, int(i[n]), int(j[n]), d[i[n], j[n]], want)


@pytest.mark.parametrize("name", B.LAYERS)
def test_a_tile_pair_whose_extreme_is_a_tie_needs_the_margin(name):
    """the layered boxes: one lattice layer per tile of the list order.  At least one tile pair passes k_classify's uniform-image test
    along c with the margin at 0 and not with 1e-9, while all 4 096 of its pairs round to the other image index; it lies beyond the
    damping range (the far-field walk of the panel contraction would take the common index) and has no common index along a or b"""
    atoms, basis, opts, info = B.box(name, B.G_LAYERS)
    tile = CONST["kTile"]
    R, vol, cut = pbc_update(basis)
    n_lat = info["n_lattice"]
    assert B.G_LAYERS ** 2 == tile and n_lat == tile * B.LAYER_COUNT and len(atoms["charge"]) < 2000
    assert R[0, 2] == 0.0 and R[1, 2] == 0.0  # the raw fractional c is one product
    z = atoms["pos"][:n_lat, 2].reshape(B.LAYER_COUNT, tile)
    assert np.all(z == z[:, :1])  # ... of one double per layer
    cases = B.margin_cases(atoms, R, tile)
    print(f"\n{name}: (tile I, tile J, direction, index of the bounds, pairs that round to another) {cases}")
    assert cases and all(p == 2 and other == tile * tile for _, _, p, _, other in cases), cases
    far = 30.0 / opts["polar_damp"]
    for I, J, _, _, _ in cases:
        d = atoms["pos"][I * tile:(I + 1) * tile, None, :] - atoms["pos"][None, J * tile:(J + 1) * tile, :]
        assert B.reference_distance(d, basis, R).min() > 2.0 * far, (name, I, J)
        assert len(np.unique(B.reference_image(d, R)[..., 0])) > 1 and len(np.unique(B.reference_image(d, R)[..., 1])) > 1
    i, j, dd = B.pair_displacements(atoms)
    inter = atoms["mol_id"][i] != atoms["mol_id"][j]
    assert B.nearest_image_distances(dd, basis)[inter].min() >= B.MIN_DIST
    ref = B.oracle(name, B.G_LAYERS)
    assert all(np.isfinite(ref[k]) for k, _ in util.ENERGY_KEYS) and ref["iterator_failed"] == 0
    got = {k: int(ref[k]) for k in B.restated_counts(atoms, basis, R, cut)}
    assert got == B.restated_counts(atoms, basis, R, cut)
