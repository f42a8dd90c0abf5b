"""CPU: the preconditions of tests/test_gpu_polar_trial_matrix.py.  Conditions on its inputs (tests/polar_trial_cases.py), checked with
numpy and the restatements alone, before any device runs.  Each is a condition, not a measurement: a seed or an index that broke one would
be replaced, the condition stays.

  conditioning   every accepted and every trial configuration the GPU file compares, under every configuration it runs there: the
                 restatement's own static field E0, perturbed by a relative 1e-13 of seeded normal noise, moves mu and ef_induced by at most
                 CAP * 1e-13 of their largest component and polarization_energy by at most CAP * 1e-13 relative, and the iteration count
                 by nothing (the cap and the procedure of tests/test_polar_ragged_preconditions.py).  Run with -s for the factors.
  distances      no trial brings a moved atom closer than 2.3 A to an atom of another molecule, and no trial configuration of a ragged box has
                 an intermolecular distance below that; the slabs carry planted pairs 2.0 to 2.3 A apart from the start: no mover is an
                 atom of such a pair, and every trial configuration has the same close pairs at the same distances as the start
  tiles          in list order the large moves of the 512-atom box cover tiles 0 to 4 and 4 to 7, their union is exactly eight; those of the
                 513-atom box cover 0 to 4 and 5 to 8, nine
  class flips    on the orthorhombic slab in list order, from the tiles' wrapped fractional extents times the cell lengths -- the bound
                 k_classify forms in an orthorhombic cell: the jumper's tile lies beyond the cutoff and beyond kTholeFarX / polar_damp
                 of at least three tiles before the long jump and at gap zero of them after it; the counts of far and of beyond-cutoff
                 tile pairs fall by at least three each, and the bystander's move changes neither
                 under the spatial order (restated: compute_spatial_order's nested bisection) the same jump changes the counts too
  sequence       the rejected one-molecule move and the accepted one behind it share no tile, in list order (the Gauss-Seidel contexts)
                 and under the spatial order (all others): the accepted move's store pass repairs a tile it did not move
  lattice hop    the raw range of the hopper's tile along the hop grows by one cell length and its wrapped extents change by rounding at
                 most, in the order the hop is made for: the third cell vector in list order, the first under the spatial order
"""
import numpy as np
import pytest

import util
import polar_ragged_boxes as B
import polar_trial_cases as C

EPS = 1e-13
CAP = 100.0
MIN_DISTANCE = 2.3

RUNGS = C.RAGGED + C.SLABS
WORST = {}


def reference_cases():
    """(rung, reference configuration): the solver settings of the plain Jacobi solve are one configuration to the restatement"""
    seen = []
    for rung in RUNGS:
        for _, cfg, _ in C.compared_configurations(rung):
            if (rung, C.reference_name(cfg)) not in seen:
                seen.append((rung, C.reference_name(cfg)))
    return seen


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for rung, (f, where) in WORST.items():  # (with -s: the record in CHANGELOG.md)
        print(f"\nlargest factor, {rung}: {f:.2f} ({where})")


@pytest.mark.parametrize("rung,ref", reference_cases())
def test_conditioning(rung, ref):
    cfg = "jac_compact" if ref == "jac" else ref
    done = set()
    for label, c, pos in C.compared_configurations(rung):
        if C.reference_name(c) != ref or C._key(pos) in done:
            continue
        done.add(C._key(pos))
        E0 = C.field_of(rung, cfg, pos)
        base = C.restated(rung, cfg, pos)
        noise = np.random.default_rng(977).normal(size=E0.shape)
        moved = C.solve(rung, cfg, pos, E0 * (1.0 + EPS * noise))
        factors = {}
        for k in ("mu", "ef_induced"):
            top = float(np.abs(base[k]).max())
            d = float(np.abs(moved[k] - base[k]).max())
            factors[k] = d / (EPS * top) if top else (0.0 if d == 0.0 else float("inf"))
        u = base["polarization_energy"]
        du = abs(moved["polarization_energy"] - u)
        factors["energy"] = du / (EPS * abs(u)) if u else (0.0 if du == 0.0 else float("inf"))
        print(f"\n{rung} {ref} {label}: " + " ".join(f"{k} {v:.2f}" for k, v in factors.items()) + f" iterations {base['polar_iterations']}")
        for k in ("polar_iterations", "iterator_failed", "contractions"):
            assert moved.get(k) == base.get(k), (rung, ref, label, k, moved.get(k), base.get(k))
        assert base["iterator_failed"] == 0 and np.isfinite(u), (rung, ref, label)
        top = max(factors.values())
        assert top <= CAP, (rung, ref, label, factors)
        if top > WORST.get(rung, (-1.0, ""))[0]:
            WORST[rung] = (top, f"{ref}, {label}")
    assert done, (rung, ref)


def moves_of(rung):
    """[(label, positions before, first, new positions)] of every trial of the GPU file on this box"""
    atoms = B.box(rung)[0]
    out = []
    if rung in C.SEQUENCE:
        pos = atoms["pos"].copy()
        for label, first, new, accept in C.sequence(rung):
            out.append((f"sequence: {label}", pos, first, new))
            pos = C.applied(pos, first, new) if accept else pos
    if rung in C.LARGE:
        pos = atoms["pos"].copy()
        for k, (first, new, accept) in enumerate(C.large_moves(rung)):
            out.append((f"large move {k}", pos, first, new))
            pos = C.applied(pos, first, new) if accept else pos
    if rung in C.SLABS:
        P, site, nudge = C.flip_positions(rung)
        out += [("long jump", P["start"], C.JUMPER, site), ("bystander", P["start"], C.BYSTANDER, nudge),
                ("long jump behind the bystander", P["nudged"], C.JUMPER, site),
                ("jump back", P["nudged_jumped"], C.JUMPER, P["nudged"][C.JUMPER:C.JUMPER + 1])]
        for axis in (0, 2):
            i, new, ph, (a, nw) = C.hop_positions(rung, axis)
            out += [(f"hop along {axis}", P["start"], i, new), (f"one molecule behind the hop along {axis}", ph, a, nw)]
    return out


def close_pairs(atoms, basis, pos):
    """{(i, j): distance} of the intermolecular pairs i < j closer than MIN_DISTANCE"""
    R = np.linalg.inv(basis)
    d = (pos[:, None, :] - pos[None, :, :]) @ R
    d -= np.rint(d)
    r = np.sqrt(((d @ basis) ** 2).sum(axis=-1))
    mol = np.asarray(atoms["mol_id"])
    n = len(pos)
    ok = (r < MIN_DISTANCE) & (mol[:, None] != mol[None, :]) & (np.arange(n)[:, None] < np.arange(n)[None, :])
    return {(int(i), int(j)): float(r[i, j]) for i, j in np.argwhere(ok)}


@pytest.mark.parametrize("rung", RUNGS)
def test_no_move_makes_a_contact(rung):
    atoms, basis, _ = B.box(rung)
    R = np.linalg.inv(basis)
    mol = np.asarray(atoms["mol_id"])
    start = C.min_intermolecular(atoms, basis, atoms["pos"])
    planted_pairs = close_pairs(atoms, basis, atoms["pos"])
    planted = {i for pair in planted_pairs for i in pair}
    print(f"\n{rung}: intermolecular pairs below {MIN_DISTANCE} A at the start {sorted(planted_pairs)}")
    for label, pos, first, new in moves_of(rung):
        trial = C.applied(pos, first, new)
        closest = np.inf
        for t in range(first, first + len(new)):
            d = (trial - trial[t]) @ R
            d -= np.rint(d)
            r = np.sqrt(((d @ basis) ** 2).sum(axis=1))
            closest = min(closest, float(r[mol != mol[t]].min()))
        whole = C.min_intermolecular(atoms, basis, trial)
        print(f"\n{rung} {label}: closest to a moved atom {closest:.3f} A, in the configuration {whole:.3f} A")
        assert closest >= MIN_DISTANCE, (rung, label, closest)
        assert whole >= min(MIN_DISTANCE, start), (rung, label, whole, start)  # (the slabs' planted pairs: 2.0 A from the start)
        assert not planted & set(range(first, first + len(new))), (rung, label, sorted(planted))
        assert close_pairs(atoms, basis, trial) == planted_pairs, (rung, label)  # the same pairs at the same distances, to the bit
    if rung in C.RAGGED:
        assert start >= MIN_DISTANCE, (rung, start)


@pytest.mark.parametrize("rung", C.SLABS)
def test_the_vacancy_and_the_single_atom_movers(rung):
    atoms = B.box(rung)[0]
    assert len(atoms["charge"]) == C.SLAB_N and C.LATTICE[0] * C.LATTICE[1] * C.LATTICE[2] - C.SLAB_N == 38
    site, clearance = C.vacancy(rung)
    print(f"\n{rung}: clearance of the vacancy {clearance:.3f} A")
    assert clearance >= 3.6, (rung, clearance)
    assert C.JUMPER // C.TILE == 4 and C.BYSTANDER // C.TILE == 10
    for i in (C.JUMPER, C.BYSTANDER, C.hopper(rung, 0), C.hopper(rung, 2)):
        assert C.lone_movable_polarizable(atoms, i) and atoms["charge"][i] != 0.0, (rung, i)


@pytest.mark.parametrize("rung", sorted(C.LARGE))
def test_large_moves_cover_eight_tiles_exactly_and_nine(rung):
    atoms = B.box(rung)[0]
    assert tuple(C.whole_molecules(atoms, *r) for r in C.LARGE[rung]) == C.LARGE_EXPECTED[rung]
    moves = C.large_moves(rung)
    spans = [C.tiles_of(first, first + len(new)) for first, new, _ in moves]
    assert [accept for _, _, accept in moves] == [False, True, True, True]
    assert all(len(new) <= C.TRIAL_MAX for _, new, _ in moves)
    assert spans[0] == [0, 1, 2, 3, 4] and spans[2] == [0] and spans[3] == [7], spans
    assert spans[1] == ([4, 5, 6, 7] if rung == 512 else [5, 6, 7, 8]), spans
    assert len(set(spans[0]) | set(spans[1])) == (8 if rung == 512 else 9)
    assert -(-rung // C.TILE) == (8 if rung == 512 else 9)


@pytest.mark.parametrize("rung", sorted(C.SEQUENCE, key=str))
def test_the_sequence_is_what_it_says(rung):
    atoms = B.box(rung)[0]
    steps = C.sequence(rung)
    assert [len(new) for _, _, new, _ in steps] == [steps[0][2].shape[0], steps[1][2].shape[0], 65, 1]
    assert [accept for *_, accept in steps] == [False, True, True, False]
    spans = [set(C.tiles_of(first, first + len(new))) for _, first, new, _ in steps]
    assert not spans[0] & spans[1] and not spans[0] & spans[2], spans  # (the rejected tile is repaired by a move that does not move it)
    # ... and under the spatial order, in which every context but the Gauss-Seidel ones runs the sequence
    perm, _ = C.spatial_order(atoms["pos"], B.box(rung)[1])
    slot = np.empty(len(perm), dtype=int)
    slot[perm] = np.arange(len(perm))
    ordered = [{int(slot[i]) // C.TILE for i in range(first, first + len(new))} for _, first, new, _ in steps]
    print(f"\n{rung}: tiles of the steps in list order {spans}, under the spatial order {ordered}")
    assert not ordered[0] & ordered[1], ordered
    assert atoms["frozen"][steps[3][1]] == 1
    for _, first, new, _ in steps[:3]:  # whole molecules
        ends = {e for _, e in util.molecules(atoms)}
        assert C.molecule_at(atoms, first)[0] == first and first + len(new) in ends


def test_class_flips_in_list_order():
    rung = C.SLABS[0]
    atoms, basis, o = B.box(rung)
    cutoff, far = C.cutoff_of(basis), C.thole_far_x() / o["polar_damp"]
    assert cutoff == 12.6 and far == 30.0 / 2.1304
    P, _, _ = C.flip_positions(rung)
    tile = C.JUMPER // C.TILE
    before, after = C.tile_gaps(P["start"], basis, tile), C.tile_gaps(P["jumped"], basis, tile)
    flipped = [t for t in range(len(before)) if before[t] > max(cutoff, far) and after[t] == 0.0]
    print(f"\ntile {tile}: gaps before {np.round(before, 2).tolist()}\n        after  {np.round(after, 2).tolist()}\nflipped {flipped}")
    assert len(flipped) >= 3, flipped
    counts = {k: C.class_counts(p, basis, cutoff, o["polar_damp"]) for k, p in P.items()}
    print(f"(far, beyond) {counts}")
    assert counts["start"] == (76, 76), counts  # (what the ragged ladder measured on the device)
    for a, b in (("start", "jumped"), ("nudged", "nudged_jumped")):
        assert counts[a][0] - counts[b][0] >= 3 and counts[a][1] - counts[b][1] >= 3, counts
    assert counts["nudged"] == counts["start"], counts
    away = C.tile_gaps(P["start"], basis, C.BYSTANDER // C.TILE)
    assert away[tile] > max(cutoff, far) and away[16] > max(cutoff, far), away  # far from both ends of the jump


@pytest.mark.parametrize("rung", C.SLABS)
def test_the_long_jump_flips_a_class_under_the_spatial_order(rung):
    """the order of a fresh context (the nested bisection: 18 tiles are below the aligned grid's size) stays while trials run: the classes
    of the start, restated, are the 5 far and 5 beyond-cutoff tile pairs the ragged ladder measured, and the long jump changes the counts"""
    atoms, basis, o = B.box(rung)
    P, _, _ = C.flip_positions(rung)
    perm, origin = C.spatial_order(P["start"], basis)
    counts = {k: C.ordered_class_counts(P[k], basis, perm, origin, C.cutoff_of(basis), o["polar_damp"]) for k in ("start", "jumped", "nudged", "nudged_jumped")}
    print(f"\n{rung}: (far, beyond) {counts}; the jumper sits in tile {int(np.nonzero(perm == C.JUMPER)[0][0]) // C.TILE} of the spatial order")
    assert counts["start"] == (5, 5), counts
    assert counts["jumped"] != counts["start"] and counts["nudged_jumped"] != counts["nudged"], counts


@pytest.mark.parametrize("axis", [0, 2])
@pytest.mark.parametrize("rung", C.SLABS)
def test_lattice_hop(rung, axis):
    atoms, basis, _ = B.box(rung)
    i, new, ph, _ = C.hop_positions(rung, axis)
    perm, origin = C.hop_order(rung, axis)  # (the list order for the third cell vector, the spatial order for the first)
    tile = C.HOP_TILE[axis]
    assert int(np.nonzero(perm == i)[0][0]) // C.TILE == tile
    r0, r1 = C.raw_ranges(atoms["pos"], basis, perm)[tile], C.raw_ranges(ph, basis, perm)[tile]
    grown = (r1[1, axis] - r1[0, axis]) - (r0[1, axis] - r0[0, axis])
    print(f"\n{rung} axis {axis}: atom {i}, raw range {r0[:, axis]} -> {r1[:, axis]}")
    assert abs(grown - 1.0) <= 1e-12, grown  # one cell length, in units of it
    others = [d for d in range(3) if d != axis]
    assert np.array_equal(r0[:, others], r1[:, others]) or np.abs(r0[:, others] - r1[:, others]).max() <= 1e-12
    w0, w1 = C.wrapped_extents(atoms["pos"], basis, perm, origin), C.wrapped_extents(ph, basis, perm, origin)
    assert np.abs(w0 - w1).max() <= 1e-12
    if axis == 0:  # under the spatial order the tile is compact along x before the hop: it has common x images to lose
        assert r0[1, 0] - r0[0, 0] < 0.5, r0
    if axis == 2:  # in list order no tile has a common x image with another to lose, and every one is compact in z
        r = C.raw_ranges(atoms["pos"], basis)
        assert np.all(r[:-1, 1, 0] - r[:-1, 0, 0] > 0.5) and np.all(r[:, 1, 2] - r[:, 0, 2] < 0.1)
