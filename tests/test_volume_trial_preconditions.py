"""CPU: the preconditions of tests/test_gpu_volume_trial_followups.py.  Conditions on its inputs (tests/volume_trial_cases.py), checked with
numpy and the restatements alone, before any device runs.  Run with -s for the figures.

  distances      every scaled configuration the GPU file evaluates keeps its smallest intermolecular distance at or above
                 min(2.3 A, the smallest of the unscaled configuration) -- the bound of tests/test_polar_trial_preconditions.py -- wherever
                 the cell grows.  Where it shrinks, a box that starts above 2.3 A stays above it (the ragged rungs, the ion boxes, the
                 lattice boxes).  The one box that starts below and shrinks is the slab at FLIP_SCALE, whose planted pairs are 2.0 A apart
                 from the start: rigid molecules in a cell scaled by s < 1 come closer by at most the uniform share (1 - s) r plus
                 (1 - s) (rho_i + rho_j), rho the distance of an atom from its molecule's centre of mass; the slab's smallest distance is
                 held to that bound of its own start, 2.0 s - (1 - s) 2 rho_max, to a floor of 1.9 A (0.95 of the planted distance;
                 1.917 A at FLIP_SCALE) and to the conditioning cap below.
  precision      jac_esor_prec runs into the iteration limit with iterator_failed on the 257- and 513-atom rungs, unscaled already, and
                 converges on ion216_polar: why the GPU file runs it there
  conditioning   every scaled polarizable configuration, under every solve the GPU file runs on it: the restatement's static field E0,
                 perturbed by a relative 1e-13 of seeded normal noise, moves mu and ef_induced by at most 100 x 1e-13 of their largest
                 component and the polarization energy by at most 100 x 1e-13 relative, and the iteration count by nothing
  class flips    FLIP_SCALE changes the (far, beyond) counts of the slab in list order: (76, 76) -> (63, 76) at 0.98.  Under the
                 spatial order of the accepted configuration the counts are (5, 5) at every scale of the search grid and at 0.9 and 1.1:
                 a volume move cannot flip a class there (volume_trial_cases' docstring has the argument), so the GPU file observes the
                 flip in list order and runs the spatial order beside it
  drift          DRIFT_SCALE shifts some atom of the 513-atom box by more than kResortDrift and every atom by less than half the
                 shortest width of the scaled cell
  tiles          sorted129 is one atom above the spatial sort's n > 2 kTile with a last tile of one atom; edge190 pads to 192 and, one
                 three-atom molecule longer, to 256; the molecule the sequence removes is not the one it appended
  far points     every insertion point is further than 2.5 A from every atom of the configuration it is used in and of the scaled one
"""
import numpy as np
import pytest

import util
import polar_direct_ref as pdr
import polar_ewald_full_ref as pef
import polar_gs_ranked_ref as gsr
import polar_ragged_boxes as B
import polar_relax_ref as rx
import polar_trial_cases as C
import polar_wolf_ref as pw
import volume_trial_cases as V
from test_polar_trial_preconditions import CAP, EPS, MIN_DISTANCE

# The slab's planted pairs stand 2.0 A apart and list-order flips exist only where the cell shrinks, so the slab cannot keep the 2.0 A of its
# start.  Its floor: 0.95 of the planted distance, half the compression the search range [0.9, 1.1] allows.  (At FLIP_SCALE 0.98: 1.917 A.)
SLAB_FLOOR = 0.95 * 2.0
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k, v in WORST.items():  # (with -s: the record in CHANGELOG.md)
        print(f"\nlargest {k}: {v}")


def radius(atoms):
    """the largest distance of an atom from its molecule's centre of mass"""
    pos, mass = np.asarray(atoms["pos"]), np.asarray(atoms["mass"])
    out = 0.0
    for a, b in util.molecules(atoms):
        com = (mass[a:b, None] * pos[a:b]).sum(axis=0) / mass[a:b].sum()
        out = max(out, float(np.linalg.norm(pos[a:b] - com, axis=1).max()))
    return out


def test_scaled_boxes_keep_their_distances():
    for label, atoms, basis, s, sa, sb in V.scaled_boxes():
        start = C.min_intermolecular(atoms, basis, atoms["pos"])
        got = C.min_intermolecular(sa, sb, sa["pos"])
        print(f"\n{label}: smallest intermolecular distance {start:.3f} -> {got:.3f} A")
        if s >= 1.0 or start >= MIN_DISTANCE:
            assert got >= min(MIN_DISTANCE, start), (label, start, got)
        else:
            assert label.startswith(V.SLAB), label  # the only box that starts below the bound and shrinks
            assert got >= s * start - (1.0 - s) * 2.0 * radius(atoms), (label, start, got)  # (the geometry of a rigid shift: it restates host_scale)
            assert got >= SLAB_FLOOR, (label, got)


# ---- conditioning -------------------------------------------------------------------------------------------------------------------------------
def polar_cases():
    """[(label, atoms, basis, options, field, solve)] of every scaled polarizable configuration under every solve the GPU file runs on it"""
    out = []
    seen = []
    for key, cfg in V.POLAR_CASES:
        if (key, C.reference_name(cfg)) in seen:  # (the solver settings of the plain Jacobi solve are one configuration to the restatement)
            continue
        seen.append((key, C.reference_name(cfg)))
        atoms, basis, _ = V.polar_box(key, cfg)
        shrunk, sb = V.scaled(atoms, basis, V.SHRINK)
        fn = pw.solve if C.family(cfg) == "wolf" else rx.solve
        for tag, a, b in [(f"x {V.REJECT_SCALE}",) + V.scaled(atoms, basis, V.REJECT_SCALE), (f"x {V.SHRINK}", shrunk, sb),
                          (f"x {V.SHRINK} x {V.GROW}",) + V.scaled(shrunk, sb, V.GROW)]:
            out.append((f"{key} {C.reference_name(cfg)} {tag}", a, b, V.reference_options(key, cfg), rx.static_field, fn))
    a, b = V.scaled(*B.box(V.SLAB)[:2], V.flip_scale())
    out.append((f"{V.SLAB} jac x {V.flip_scale()}", a, b, C.reference_options(V.SLAB, "jac_compact"), rx.static_field, rx.solve))
    solves = {"pef": (rx.static_field, pef.solve), "direct": (pdr.static_field, pdr.solve), "gs_ranked": (rx.static_field, gsr.solve)}
    for name, (field, fn) in solves.items():
        atoms, basis, o = V.extra_solve(name)
        a, b = V.scaled(atoms, basis, V.REJECT_SCALE)
        out.append((f"{name} {V.EXTRA_SOLVES[name][0]} x {V.REJECT_SCALE}", a, b, o, field, fn))
    for name in V.FROZEN + ("ion216_gs", "ion216_triclinic_rdm_ljwh"):
        atoms, basis, o = V.fixture(name)
        for s in (V.SHRINK, V.GROW) if name in V.FROZEN else (V.REJECT_SCALE,):
            a, b = V.scaled(atoms, basis, s)
            out.append((f"{name} x {s}", a, b, o, rx.static_field, rx.solve))
    return out


POLAR_CASES = polar_cases()


@pytest.mark.parametrize("k", range(len(POLAR_CASES)), ids=[c[0].replace(" ", "_") for c in POLAR_CASES])
def test_conditioning(k):
    label, atoms, basis, o, field, solve = POLAR_CASES[k]
    E0 = np.asarray(field(atoms, basis, o))
    base = solve(atoms, basis, o, E0=E0)
    noise = np.random.default_rng(977).normal(size=E0.shape)
    moved = solve(atoms, basis, o, E0=E0 * (1.0 + EPS * noise))
    factors = {}
    for key in ("mu", "ef_induced"):
        if key in base:
            top = float(np.abs(base[key]).max())
            d = float(np.abs(moved[key] - base[key]).max())
            factors[key] = d / (EPS * top) if top else (0.0 if d == 0.0 else float("inf"))
    u = base["polarization_energy"]
    du = abs(moved["polarization_energy"] - u)
    factors["energy"] = du / (EPS * abs(u)) if u else (0.0 if du == 0.0 else float("inf"))
    print(f"\n{label}: " + " ".join(f"{key} {v:.2f}" for key, v in factors.items()) + f" iterations {base.get('polar_iterations')}")
    for key in ("polar_iterations", "iterator_failed", "contractions"):
        assert moved.get(key) == base.get(key), (label, key, moved.get(key), base.get(key))
    assert not base.get("iterator_failed") and np.isfinite(u) and u != 0.0, label
    top = max(factors.values())
    assert top <= CAP, (label, factors)
    if top > WORST.get("conditioning factor", (-1.0, ""))[0]:
        WORST["conditioning factor"] = (round(top, 2), label)


def test_the_precision_terminated_solve_needs_another_box():
    """why jac_esor_prec runs on the ion fixture and not on the ragged rungs: on those the restatement runs into the iteration limit and
    reports iterator_failed, unscaled already; on the fixture it converges"""
    cfg = V.PRECISION_CONFIG
    for rung in V.POLAR_RUNGS:
        atoms, basis, _ = B.box(rung)
        o = C.reference_options(rung, cfg)
        r = rx.solve(atoms, basis, o, E0=rx.static_field(atoms, basis, o))
        print(f"\n{rung} {cfg}: iterations {r['polar_iterations']} iterator_failed {r['iterator_failed']}")
        assert r["iterator_failed"] == 1 and r["polar_iterations"] == rx.MAX_ITERATION_COUNT, (rung, r["polar_iterations"], r["iterator_failed"])
    atoms, basis, _ = V.polar_box(V.PRECISION_BOX, cfg)
    o = V.reference_options(V.PRECISION_BOX, cfg)
    r = rx.solve(atoms, basis, o, E0=rx.static_field(atoms, basis, o))
    assert r["iterator_failed"] == 0 and r["polar_iterations"] < 10, (r["polar_iterations"], r["iterator_failed"])
    assert (V.PRECISION_BOX, cfg) in V.POLAR_CASES and not any(c == cfg for k, c in V.POLAR_CASES if k in V.POLAR_RUNGS)


# ---- class flips ----------------------------------------------------------------------------------------------------------------------------------
def test_flip_scale_changes_the_classes_in_list_order_and_no_scale_does_under_the_spatial_order():
    s, start, got = V.flip_search()
    print(f"\nFLIP_SCALE {s}: (far, beyond) in list order {start[0]} -> {got[0]}, under the spatial order {start[1]} -> {got[1]}")
    assert 0.9 <= s <= 1.1
    assert start == ((76, 76), (5, 5)), start  # (what tests/test_polar_trial_preconditions.py restates for the same slab)
    assert got[0] != start[0] and abs(got[0][0] - start[0][0]) >= 3, (start, got)
    assert (s, got[0]) == (0.98, (63, 76)), (s, got)  # the figures of the record
    # the spatial order: the counts of the accepted configuration at every scale of the grid and at both ends of the range
    for t in V.FLIP_GRID + [0.9, 1.1]:
        assert V.slab_counts(t)[1] == start[1], (t, V.slab_counts(t))
    # ... and why: most molecules have one site, and the far pairs are further apart than any scale of the range brings below the far range
    atoms, basis, o = B.box(V.SLAB)
    sizes = [b - a for a, b in util.molecules(atoms)]
    assert sizes.count(1) == 999 and sizes.count(3) == 30
    assert C.thole_far_x() / o["polar_damp"] > 1.1 * C.cutoff_of(basis)


# ---- drift ----------------------------------------------------------------------------------------------------------------------------------------
def test_drift_scale_outruns_the_resort_threshold():
    atoms, basis, _ = B.box(V.DRIFT_RUNG)
    pos, b = V.host_scale(atoms, basis, V.DRIFT_SCALE)
    shift = np.linalg.norm(pos - atoms["pos"], axis=1)
    width, width0 = float(V.cell_widths(b).min()), float(V.cell_widths(basis).min())
    print(f"\nDRIFT_SCALE {V.DRIFT_SCALE}: shifts {shift.min():.3f} to {shift.max():.3f} A, kResortDrift {V.resort_drift()} A, shortest width of the "
          f"scaled cell {width:.3f} A (of the accepted one {width0:.3f} A)")
    assert V.resort_drift() == 2.0
    assert shift.max() > V.resort_drift()
    assert shift.max() < 0.5 * width, (shift.max(), width)
    assert V.DRIFT_RUNG > 256 and V.DRIFT_RUNG > 2 * util.ladder_constants()["kTile"]  # a bulk update of a sorted list: the drift check runs
    # the jitter of the GPU test stays below the threshold, its control crosses it
    assert 0.01 * np.sqrt(3.0) < V.resort_drift() < 2.5


# ---- tiles ----------------------------------------------------------------------------------------------------------------------------------------
def test_lattice_boxes_sit_on_their_edges():
    tile = util.ladder_constants()["kTile"]
    pad = lambda n: -(-n // tile) * tile
    for name, n in (("sorted129", 129), ("edge190", 190)):
        atoms, basis, opts, vacant = V.lattice_box(name)
        sizes = [b - a for a, b in util.molecules(atoms)]
        assert len(atoms["pos"]) == n and set(sizes) == {1, 3} and len(vacant) >= 2, (name, len(atoms["pos"]), set(sizes))
        assert len(set(np.round(atoms["mass"], 6))) > 1 and abs(float(atoms["charge"].sum())) < 1e-12
        assert not util.nonpolar(opts)["polarization"] and not opts.get("rd_only")
        hist = V.list_edit_history(name)
        assert [len(a["pos"]) for _, a, _ in hist] == [n, n + 3, n + 3, n, n, n + 3]
        r0, r1 = util.molecules(hist[2][1])[V.REMOVED]
        assert r1 - r0 == 3 and r1 <= n  # a three-atom molecule of the original list, not the appended one
    assert 129 == 2 * tile + 1 and pad(129) == 3 * tile  # three tiles, the last with one atom, just above n > 2 kTile
    assert (pad(190), pad(193)) == (192, 256) and tile == 64


# ---- far points -----------------------------------------------------------------------------------------------------------------------------------
def test_insertion_points_are_far_from_every_atom_in_both_cells():
    seen = []
    for name in V.LATTICE:
        _, _, _, vacant = V.lattice_box(name)
        hist = dict((label, (a, b)) for label, a, b in V.list_edit_history(name))
        for label, point, s in (("start", vacant[0], V.GROW), ("fewer", vacant[1] * V.GROW, V.SHRINK)):
            a, b = hist[label]
            seen.append((f"{name} {label}", V.clearance(a, b, point), V.clearance(*V.scaled(a, b, s), point)))
    for name in V.TERM_FIXTURES:
        atoms, basis, opts = V.fixture(name)
        if V.insertion_allowed(opts) and not V.is_polarizable(opts):
            for k in range(4):
                p = V.far_point(atoms, basis, V.REJECT_SCALE, seed=100 + k)
                seen.append((f"{name} point {k}", V.clearance(atoms, basis, p), V.clearance(*V.scaled(atoms, basis, V.REJECT_SCALE), p)))
    for label, here, there in seen:
        print(f"\n{label}: {here:.3f} A from the nearest atom, {there:.3f} A in the scaled cell")
        assert here > V.FAR and there > V.FAR, (label, here, there)
    assert any("ion216_wolf" in s[0] for s in seen) and any("lj64_rc2" in s[0] for s in seen) and any("h2_64_sg" in s[0] for s in seen)


# ---- displacement moves ---------------------------------------------------------------------------------------------------------------------------
def test_every_displacement_keeps_clear_of_its_neighbours():
    """volume_trial_cases.displacement searches its seed for this; here the search is shown to end on every box the GPU file moves a molecule
    of, and the slab's jumper, whose jitter is fixed, is held to the same bound"""
    boxes = [(name,) + V.fixture(name)[:2] for name in V.TERM_FIXTURES + list(V.FROZEN) + ["ion64_es", "water64_polar"]]
    boxes += [(str(key),) + V.polar_box(key, cfg)[:2] for key, cfg in V.POLAR_CASES[::len(V.POLAR_CONFIGS)]]
    for label, atoms, basis in boxes:
        shapes = [("", atoms, basis)] + [(f" x {s}",) + V.scaled(atoms, basis, s) for s in (V.SHRINK, V.GROW)]
        for tag, a, b in shapes:
            for where, seed in ((0.5, 7), (0.25, 17), (0.25, 23)):
                first, new = V.displacement(a, b, where=where, seed=seed)
                assert not np.any(a["frozen"][first:first + len(new)]), (label, tag)
    atoms, basis, _ = B.box(V.SLAB)
    start = C.min_intermolecular(atoms, basis, atoms["pos"])
    for tag, a, b in (("", atoms, basis),) + ((" scaled",) + V.scaled(atoms, basis, V.flip_scale()),):
        moved = C.applied(a["pos"], C.JUMPER, C.jitter(a["pos"], C.JUMPER, 47))
        d = (moved - moved[C.JUMPER]) @ np.linalg.inv(b)
        r = np.linalg.norm((d - np.rint(d)) @ b, axis=1)
        r[C.JUMPER] = np.inf
        print(f"\n{V.SLAB}{tag}: the jumper's jitter leaves it {r.min():.3f} A from its nearest neighbour")
        assert r.min() >= min(MIN_DISTANCE, start), (tag, r.min())
