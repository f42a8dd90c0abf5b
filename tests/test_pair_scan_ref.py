"""CPU: the arbitrary-precision references of tests/pair_scan_ref.py against the fp64 restatements, and the grids against their promises.

The GPU scans (tests/test_gpu_pair_scans.py) assert e_gpu <= max(B, 4 e_cpu).  The second branch exists for expressions that are
ill-conditioned in fp64 themselves; it must not swallow a scan, so here, without a device, e_cpu <= B / 4 is asserted on at least 95 % of
the points of every scan, and e_cpu <= 1e-9 everywhere (a reference that restated another formula would be off by far more).

Share of the points with e_cpu <= B / 4, measured here: 100 % on every real-space scan (largest e_cpu 4.2e-15) and on the k-space scans
in the cell; at least 95 % on the k-space scans whose atoms lie up to 1000 cells from the origin (largest e_cpu 6.1e-13, with the three
k-vectors of ewald_kmax = 1, where nothing averages the rounding of a phase of 1e4 rad out): their unwrapping reach is log-spaced from 1
to 1000 cells so that the far configurations stay a small share.
"""
import numpy as np
import pytest

import pair_scan_ref as P

M = P.M


def scans():
    out = []
    for alpha in ("default", "table_end"):
        for intra in (False, True):
            for cellname in ("cubic", "triclinic"):
                out.append(("ewald", (alpha, intra, cellname)))
    for order in (2, 4):
        for t in (20.0, 77.0):
            out.append(("ewald", ("default", False, "cubic", order, t)))
    out += sorted({("field", (a, i, c, pa, P.field_kernel_that_runs(k, a, pa) == "sweep")) for k, c, i, a, pa in P.FIELD_CASES}, key=str)
    out += [("wolf", ("cubic",)), ("wolf", ("triclinic",)), ("sg", (0, 0.0)), ("sg", (1, 20.0)), ("sg", (1, 77.0))]
    out += [("rd_model", (f, r)) for f in P.RD_FORMS for r in P.RD_RULES]
    out += [("recip", c) for c in P.RECIP_CASES] + [("thole", c) for c in P.THOLE_CASES]
    out += [("wolf_field", (a,)) for a in P.WOLF_ALPHAS] + [("crystal", ())]
    out += [("line", ())] + [("disp", f) for f in P.DISP_FLAGS]
    return out


BUILDERS = {"ewald": P.ewald_scan, "field": P.field_scan, "wolf": P.wolf_scan, "sg": P.sg_scan, "rd_model": P.rd_model_scan, "recip": P.recip_scan,
            "line": P.line_scan, "disp": P.disp_scan, "thole": P.thole_scan, "wolf_field": P.wolf_field_scan,
            "crystal": P.crystal_scan}


@pytest.mark.parametrize("kind,args", scans(), ids=lambda v: "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v))
def test_references_agree_with_the_fp64_restatements(kind, args):
    sc = BUILDERS[kind](*args)
    assert len(sc.points) >= 64
    for key in sc.keys():
        e = sc.e_cpu(key)
        share = sc.share_within(key)
        print(f"{sc.name} {key}: {len(e)} points, max e_cpu {e.max():.3e}, share within B / 4 {share:.4f}")
        assert share >= 0.95, (sc.name, key, share)
        assert e.max() <= 1e-9, (sc.name, key, e.max(), sc.points[int(np.argmax(e))])
    if kind in ("ewald", "sg", "rd_model", "disp", "crystal"):  # the scans that are also walked as displacement trials: the guard for the differences
        k0 = P.rest_index(sc)
        for key in sc.keys():
            ed = np.array([P.delta_terms(sc, key, k, k0)[2] for k in range(len(sc.points))])
            assert (ed <= P.B_DEFAULT / 4).mean() >= 0.95, (sc.name, key, "differences", float((ed <= P.B_DEFAULT / 4).mean()))
            if key == "lj_pairs" and kind == "ewald":
                assert (ed <= P.B_TRIAL_LJ / 4).mean() >= 0.95 and (sc.e_cpu(key) <= P.B_TRIAL_LJ / 4).mean() >= 0.95, (sc.name, key, "B_TRIAL_LJ")


def test_a_scan_is_computed_once_and_shared():
    assert P.ewald_scan("default", False, "cubic") is P.ewald_scan("default", False, "cubic")


def test_grids_hold_the_boundary_points_they_promise():
    alpha = P.ALPHAS["table_end"]
    g = P.ewald_grid(alpha)
    s = set(g.tolist())
    assert np.all(np.diff(g) > 0) and g[0] == 0.8
    n_pieces = 0
    for j in range(1, P.TABLE_PIECES):
        exact = M(j) / (128 * M(alpha))
        if not (0.8 <= float(exact) < P.CUTOFF):
            continue
        n_pieces += 1
        below = max(p for p in g if M(float(p)) < exact)
        above = min(p for p in g if M(float(p)) >= exact)
        assert float(np.nextafter(below, np.inf)) == above, j  # the two doubles on either side of the boundary
        assert int(M(float(below)) * M(alpha) * 128) == j - 1 and int(M(float(above)) * M(alpha) * 128) == j
        assert float((M(j) + M(1) / 2) / (128 * M(alpha))) in s  # the midpoint of the piece
    assert n_pieces > 470  # alpha r from 0.27 to 3.99
    # both sides of the cutoff, 1 ulp and 1e-9 relative, and the cutoff itself
    for p in (np.nextafter(P.CUTOFF, 0.0), np.nextafter(P.CUTOFF, np.inf), P.CUTOFF * (1 - 1e-9), P.CUTOFF * (1 + 1e-9), P.CUTOFF, P.REST_R):
        assert float(p) in s, p
    # where exp_fast's rint switches: alpha^2 r^2 log2(e) within 1e-12 of a half-integer
    log2e = 1 / P.mp.log(2)
    halves = [p for p in g if abs((M(alpha) * M(float(p))) ** 2 * log2e - P.mp.floor((M(alpha) * M(float(p))) ** 2 * log2e) - M(1) / 2) < M(10) ** -12]
    assert len(halves) >= 20, len(halves)


def test_branch_points_of_the_other_terms():
    g = set(P.sg_grid().tolist())
    rm = P.SG["RM"] * P.SG["BOHR"]
    for p in (np.nextafter(rm, 0.0), np.nextafter(rm, np.inf), rm * (1 - 1e-9), rm * (1 + 1e-9)):
        assert float(p) in g
    assert min(g) == 0.3
    below = [p for p in g if p / P.SG["BOHR"] < P.SG["RM"]]
    assert max(below) < rm <= min(p for p in g if p >= rm)
    # Silvera-Goldman's first exponent is positive at short range: the scan reaches those arguments
    assert P.SG["ALPHA"] - P.SG["BETA"] * (0.3 / P.SG["BOHR"]) > 0.5
    sc = P.rd_model_scan("drd", "lb")
    sig = 0.5 * (P.SIGMA[0] + P.SIGMA[1])
    pts = set(sc.points)
    for p in (np.nextafter(0.4 * sig, 0.0), np.nextafter(0.4 * sig, np.inf)):
        assert float(p) in pts
    k = sc.points.index(float(np.nextafter(0.4 * sig, 0.0)))
    assert sc.scale["lj_pairs"][k] > M(10) ** 39  # (MAXVALUE below 0.4 sigma)
    assert 12.0 * (1.0 - min(pts) / sig) > 7.0  # DREIDING's exponent up to +7.2 is scanned
    # lambda r = kTholeFarX, where the kernels drop the Thole damping, and the ends lambda r = 0.01 and 35
    far, t = P.thole_far_x() / P.POLAR_DAMP, set(P.thole_grid().tolist())
    for p in (np.nextafter(far, 0.0), np.nextafter(far, np.inf), far * (1 - 1e-9), far * (1 + 1e-9), far):
        assert float(p) in t, p
    assert min(t) == 0.01 / P.POLAR_DAMP and max(t) * P.POLAR_DAMP > 34.999999 and P.REST_R in t


def test_kmax_zero_enumerates_no_k_vector():
    assert len(P.k_vectors(0)) == 0 and P.k_vectors(0).shape == (0, 3)
    assert len(P.k_vectors(1)) == 3 and len(P.k_vectors(7)) == 709
    sc = P.recip_scan(2, 0, "cubic", False)
    assert all(v == 0 for v in sc.ref["es_recip"]) and all(v == 0.0 for v in sc.cpu["es_recip"])
    # the enumeration is a half space: no vector and its negative, no zero vector
    L = {tuple(v) for v in P.k_vectors(7).tolist()}
    assert (0, 0, 0) not in L and not any((-a, -b, -c) in L for a, b, c in L)


def test_k_space_sums_in_long_double_match_mpmath():
    """the factorised long-double phases against term-by-term mpmath, 1000 cells out in a triclinic cell"""
    pos = P.recip_positions(2, "triclinic", True)[10]
    at = P.recip_atoms(pos)
    a = P.recip_longdouble(at["pos"], at["charge"], P.TRICLINIC, P.ALPHAS["default"], 3, 0.25)
    b = P.recip_mp(at["pos"], at["charge"], P.TRICLINIC, P.ALPHAS["default"], 3, 0.25)
    bound = 1e-15 if P.LONGDOUBLE_OK else 1e-11  # (a 64-bit mantissa leaves 5e-17 of a phase of 1e5 rad)
    assert abs(P.ld_to_mp(a["es_recip"][0]) - b["es_recip"][0]) <= bound * b["es_recip"][1]
    assert abs(P.ld_to_mp(a["es_recip"][1]) - b["es_recip"][1]) <= bound * b["es_recip"][1]
    for i in range(2):
        for c in range(3):
            assert abs(P.ld_to_mp(a["field"][0][i, c]) - b["field"][0][i][c]) <= bound * b["field"][1][i][c]
