"""Every pair function of the HIP path against arbitrary-precision scans, point by point (tests/pair_scan_ref.py).

A scan is one live context holding two atoms (a few hold 65), moved from point to point with update_positions, trial_energy / reject,
trial_insert_energy or ONE insert_candidates batch; at every point and for every observable

    e_gpu <= max(B, 4 e_cpu),     e = |value - ref| / scale,

with `ref` the 50-digit value, `scale` the summed magnitudes of the terms the formula adds and `cpu` the fp64 restatement (the oracle,
sg_ref, rd_model_ref, ...).  B = 1e-12, the margin the README claims; field components that went through the sweep's erfc table take the
table's pinned host bounds (tests/test_erfc_table.py: 5e-13 below alpha r = 2, 1e-10 up to 4) on their real-space share plus 1e-12.  No
bound comes from a run of the kernels.  tests/test_pair_scan_ref.py shows on the CPU that e_cpu <= B / 4 on (nearly) all points, so the
second branch cannot swallow a scan.  Each scan asserts which kernel ran.  Every check prints one line
`SCAN|scan|route|observable|points|max e_gpu|max e_cpu|where`.
"""
import numpy as np
import pytest

import pair_scan_ref as P
from mpmcxx_amd import energy

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_device():
    if energy.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests need an MI355X")


@pytest.fixture
def pair_kernel():
    """energy.configure("pair_kernel", v) for the contexts a test creates; back to the default afterwards"""
    def choose(v):
        energy.configure("pair_kernel", v)
    yield choose
    energy.configure("pair_kernel", 0)


KERNELS = {"sweep": 2, "fused": 1}
BASE_R = P.REST_R


def at_x(r):
    return np.array([[float(r), 0.0, 0.0]])


def walk(S, points, keys, first=1, pos_of=at_x, after=None):
    """full evaluations: atom `first` moved to every point with update_positions; {key: values}"""
    out = {k: [] for k in keys}
    for p in points:
        S.update_positions(first, pos_of(p))
        S.energy()
        o = S.observables
        for k in keys:
            out[k].append(o[k])
        if after is not None:
            after(S)
    return out


def walk_trials(S, points, keys, first=1, pos_of=at_x):
    """displacement trials from the resting configuration: trial_energy / reject at every point; {key: values of the trial configuration}"""
    S.energy()
    out = {k: [] for k in keys}
    for p in points:
        S.trial_energy(first, pos_of(p))
        assert not S.last_trial_was_full()
        for k in keys:
            out[k].append(S.trial_observables[k])
        S.reject()
    return out


# ---- (a) Ewald real space ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", ["default", "table_end"])
@pytest.mark.parametrize("intra", [False, True], ids=["inter", "intra"])
@pytest.mark.parametrize("cellname", ["cubic", "triclinic"])
@pytest.mark.parametrize("kernel", ["sweep", "fused"])
def test_ewald_real_space_energies(kernel, cellname, intra, alpha, pair_kernel):
    sc = P.ewald_scan(alpha, intra, cellname)
    pair_kernel(KERNELS[kernel])
    S = energy.System(P.pair_atoms(BASE_R, intra), P.cell(cellname), sc.extra["opts"])
    got = walk(S, sc.points, ["lj_pairs", "es_real"])
    assert S.last_pair_kernel() == kernel
    S.close()
    for k in ("lj_pairs", "es_real"):
        sc.check(k, got[k], kernel)


@pytest.mark.parametrize("kernel,cellname,intra,alpha,polar_alpha", P.FIELD_CASES)
def test_ewald_static_field_rows(kernel, cellname, intra, alpha, polar_alpha, pair_kernel):
    """both rows of the static field (real_term + recip_term in long double) with polarization on, one Jacobi iteration"""
    ran = P.field_kernel_that_runs(kernel, alpha, polar_alpha)
    sc = P.field_scan(alpha, intra, cellname, polar_alpha, ran == "sweep")
    pair_kernel(KERNELS[kernel])
    S = energy.System(P.pair_atoms(BASE_R, intra, polarizability=P.POLARIZABILITY), P.cell(cellname), sc.extra["opts"])
    rows = []
    walk(S, sc.points, [], after=lambda S: rows.append(S.dipoles()[1].reshape(-1)))
    assert S.last_pair_kernel() == ran and S.observables["polar_iterations"] == 1
    S.close()
    rows = np.array(rows)
    for t, k in enumerate(P.FIELD_KEYS):
        sc.check(k, rows[:, t], f"{kernel}->{ran}")


# ---- (b) the trial kernels -------------------------------------------------------------------------------------------------------------------------
def delta_check(sc, key, got, base, label, k0=None, bound=P.B_DEFAULT):
    """trial totals minus the resting totals against the 50-digit difference; the scale is that of both configurations (k0: the resting point)"""
    if k0 is None:
        k0 = P.rest_index(sc)
    worst = 0.0
    bad = []
    for k, g in enumerate(got):
        ref, scale, ec = P.delta_terms(sc, key, k, k0)
        eg = P.err(g - base[key], ref, scale)
        worst = max(worst, eg)
        if not eg <= max(bound, 4.0 * ec):
            bad.append((sc.points[k], eg, ec))
    print(f"SCAN|{sc.name}|{label}|{key}|{len(got)}|{worst:.3e}|-|-")
    assert not bad, (sc.name, label, key, bound, len(bad), max(bad, key=lambda t: t[1]))


@pytest.mark.parametrize("intra", [False, True], ids=["inter", "intra"])
@pytest.mark.parametrize("cellname", ["cubic", "triclinic"])
def test_displacement_trials(cellname, intra):
    sc = P.ewald_scan("default", intra, cellname)
    S = energy.System(P.pair_atoms(BASE_R, intra), P.cell(cellname), sc.extra["opts"])
    got = walk_trials(S, sc.points, ["lj_pairs", "es_real"])
    base = dict(S.observables)
    S.close()
    for k in ("lj_pairs", "es_real"):
        delta_check(sc, k, got[k], base, "trial_energy")
    delta_check(sc, "lj_pairs", got["lj_pairs"], base, "trial_energy, fast_rsqrt's claim", bound=P.B_TRIAL_LJ)


def one_ion(i, r=0.0):
    a = P.pair_atoms(r)
    return {k: v[i:i + 1].copy() for k, v in a.items()}


@pytest.mark.parametrize("cellname", ["cubic", "triclinic"])
def test_insertion_trials_single_and_batched(cellname):
    """the second ion inserted beside the resident first one: single trials on a thinned grid, ONE batch with every point; the batch equals
    the single trials bit for bit"""
    sc = P.ewald_scan("default", False, cellname)
    S = energy.System(one_ion(0), P.cell(cellname), sc.extra["opts"])
    S.energy()
    mol = one_ion(1)
    pts = np.array(sc.points)
    batch = S.insert_candidates(mol, np.array([at_x(r) for r in pts]))
    assert S.insert_batch_counts() == (1, len(pts))
    index = list(range(0, len(pts), 4))
    single = []
    for k in index:
        S.trial_insert_energy(1, dict(mol, pos=at_x(pts[k])))
        assert not S.last_trial_was_full()
        single.append(dict(S.trial_observables))
        S.reject()
    S.close()
    for key in ("lj_pairs", "es_real"):
        sc.check(key, [b[key] for b in batch], "insert_candidates")
        sc.check(key, [s[key] for s in single], "trial_insert_energy", index=index)
    tight = P.Scan(sc.name, sc.points)  # the same references under the bound that fast_rsqrt's own claim gives (pair_scan_ref.B_TRIAL_LJ)
    tight.ref, tight.scale, tight.cpu = sc.ref, sc.scale, sc.cpu
    tight.bound = {"lj_pairs": [P.B_TRIAL_LJ] * len(sc.points)}
    tight.check("lj_pairs", [b["lj_pairs"] for b in batch], "insert_candidates, fast_rsqrt's claim")
    for s, k in zip(single, index):
        assert s == batch[k], (pts[k], s, batch[k])


# ---- (c) Feynman-Hibbs ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("temperature", [20.0, 77.0])
@pytest.mark.parametrize("order", [2, 4])
def test_feynman_hibbs(order, temperature):
    sc = P.ewald_scan("default", False, "cubic", order, temperature)
    S = energy.System(P.pair_atoms(BASE_R), P.CUBIC, sc.extra["opts"])
    got = walk(S, sc.points, ["lj_pairs", "es_real"])
    assert S.last_pair_kernel() == "fused"  # (the sweep has no FH terms)
    S.update_positions(1, at_x(BASE_R))
    trial = walk_trials(S, sc.points, ["lj_pairs", "es_real"])
    base = dict(S.observables)
    S.close()
    for k in ("lj_pairs", "es_real"):
        sc.check(k, got[k], "energy")
        delta_check(sc, k, trial[k], base, "trial_energy")


# ---- (d) Wolf -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cellname", ["cubic", "triclinic"])
def test_wolf_energy(cellname):
    sc = P.wolf_scan(cellname)
    S = energy.System(P.pair_atoms(BASE_R), P.cell(cellname), sc.extra["opts"])
    got = walk(S, sc.points, ["coulombic_energy"])
    assert S.last_pair_kernel() == "fused"
    S.close()
    sc.check("coulombic_energy", got["coulombic_energy"], "energy")


# ---- (f) the other rd terms -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fh,temperature", [(0, 0.0), (1, 20.0), (1, 77.0)])
def test_silvera_goldman(fh, temperature):
    sc = P.sg_scan(fh, temperature)
    S = energy.System(P.h2_pair(BASE_R), P.CUBIC, sc.extra["opts"])
    got = walk(S, sc.points, ["rd_energy"])
    assert S.silvera_goldman_info()["enabled"] == 1 and S.silvera_goldman_info()["feynman_hibbs"] == fh
    S.update_positions(1, at_x(BASE_R))
    trial = walk_trials(S, sc.points, ["rd_energy"])
    base = dict(S.observables)
    S.close()
    sc.check("rd_energy", got["rd_energy"], "energy")
    delta_check(sc, "rd_energy", trial["rd_energy"], base, "trial_energy")


@pytest.mark.parametrize("rule", list(P.RD_RULES))
@pytest.mark.parametrize("form", list(P.RD_FORMS))
def test_rd_model(form, rule):
    sc = P.rd_model_scan(form, rule)
    S = energy.System(P.pair_atoms(BASE_R), P.CUBIC, sc.extra["opts"])
    S.set_rd_model(P.RD_FORMS[form], P.RD_RULES[rule])
    got = walk(S, sc.points, ["lj_pairs"])
    S.update_positions(1, at_x(BASE_R))
    S.energy()
    if (form, rule) != ("lj", "lb"):  # (that pair IS the plain term)
        assert S.rd_model_info()["n_terms"] == 1, S.rd_model_info()
    trial = walk_trials(S, sc.points, ["lj_pairs"])
    base = dict(S.observables)
    S.close()
    sc.check("lj_pairs", got["lj_pairs"], "energy")
    delta_check(sc, "lj_pairs", trial["lj_pairs"], base, "trial_energy")


# ---- (g) reciprocal space ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_atoms,kmax,cellname,unwrapped", P.RECIP_CASES)
def test_reciprocal_space(n_atoms, kmax, cellname, unwrapped):
    """es_recip and the static field on the first and the last atom (65 atoms: two tiles, the second with one atom)"""
    sc = P.recip_scan(n_atoms, kmax, cellname, unwrapped)
    poss, rows = sc.extra["positions"], sc.extra["rows"]
    S = energy.System(P.recip_atoms(poss[0]), P.cell(cellname), sc.extra["opts"])
    es, field = [], []
    for pos in poss:
        S.update_positions(0, pos)
        S.energy()
        es.append(S.observables["es_recip"])
        E = S.dipoles()[1]
        field.append(np.concatenate([E[i] for i in rows]))
    S.close()
    if kmax == 0:
        assert all(v == 0.0 for v in es), es
    sc.check("es_recip", es, "energy")
    field = np.array(field)
    for t, k in enumerate(P.FIELD_KEYS):
        sc.check(k, field[:, t], "energy")


# ---- (a) 65 ions: the moving pair in an off-diagonal tile pair -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["sweep", "fused"])
def test_ion_passing_another_in_an_off_diagonal_tile_pair(kernel, pair_kernel):
    sc = P.line_scan()
    pair_kernel(KERNELS[kernel])
    S = energy.System(P.line_atoms(), P.CUBIC, sc.extra["opts"])
    got = walk(S, sc.points, ["lj_pairs", "es_real"], first=64, pos_of=lambda t: P.line_atoms(t)["pos"][64:65])
    assert S.last_pair_kernel() == kernel
    k0 = int(np.argmin([float(v) for v in sc.scale["lj_pairs"]]))  # the resting point: where the moving ion is closest to nobody
    S.update_positions(64, P.line_atoms(sc.points[k0])["pos"][64:65])
    S.energy()
    base = dict(S.observables)
    trial = {k: [] for k in ("lj_pairs", "es_real")}
    for t in sc.points:
        S.trial_energy(64, P.line_atoms(t)["pos"][64:65])
        assert not S.last_trial_was_full()
        for k in trial:
            trial[k].append(S.trial_observables[k])
        S.reject()
    S.close()
    for k in ("lj_pairs", "es_real"):
        sc.check(k, got[k], kernel)
        delta_check(sc, k, trial[k], base, kernel + ",trial_energy", k0)


@pytest.mark.parametrize("damp,schmidt,extrapolate", P.DISP_FLAGS)
def test_disp_expansion(damp, schmidt, extrapolate):
    sc = P.disp_scan(damp, schmidt, extrapolate)
    S = energy.System(P.disp_atoms(BASE_R), P.CUBIC, sc.extra["opts"])
    S.set_disp_expansion(True, np.array(P.DISP["c6"]), np.array(P.DISP["c8"]), np.array(P.DISP["c10"]), damp=damp, extrapolate_c10=extrapolate, schmidt=schmidt)
    got = walk(S, sc.points, ["lj_pairs"])
    assert S.disp_expansion() == S.observables["rd_energy"] == got["lj_pairs"][-1]
    S.update_positions(1, at_x(BASE_R))
    trial = walk_trials(S, sc.points, ["lj_pairs"])
    base = dict(S.observables)
    S.close()
    sc.check("lj_pairs", got["lj_pairs"], "energy")
    delta_check(sc, "lj_pairs", trial["lj_pairs"], base, "trial_energy")


# ---- (e) the Thole tensor ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,max_iter", P.THOLE_CASES)
def test_thole_dipoles(mode, max_iter):
    """the dipoles of a polarizable pair under the no-PBC static field, lambda r from 0.01 to 35, after 1, 2 and 10 iterations against the same
    recurrence at 50 digits (Jacobi with the compact, matrix-free and dense solvers, Gauss-Seidel), and the direct solve against the solved
    system; 1e-9 from lambda r = kTholeFarX on, where the kernels drop the damping"""
    sc = P.thole_scan(mode, max_iter)
    S = energy.System(P.thole_atoms(BASE_R), P.THOLE_BASIS, sc.extra["opts"])
    mu, iters, fields = [], set(), []

    def after(S):
        m, E, _ = S.dipoles()
        mu.append(m.reshape(-1))
        fields.append(E.reshape(-1))
        iters.add(S.observables["polar_iterations"])

    walk(S, sc.points, [], after=after)
    if mode == "direct":
        info = S.direct_info()
        assert info["n_unknowns"] == 6 and info["status"] == 0, info
    else:
        assert iters == {max_iter}, iters
    assert S.observables["iterator_failed"] == 0
    S.close()
    mu, fields = np.array(mu), np.array(fields)
    assert not np.any(mu[:, [1, 2, 4, 5]]) and not np.any(fields[:, [1, 2, 4, 5]])  # (a pair on the x axis: nothing across it)
    sc.check("mu0x", mu[:, 0], mode)
    sc.check("mu1x", mu[:, 3], mode)


# ---- (d) the Wolf static field ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a", P.WOLF_ALPHAS)
def test_polar_wolf_static_field(a):
    """polar_wolf_alpha 0, 0.13 and 1.0 in a 90 A cell: the last reaches a r = 43, exp_fast at -1849"""
    sc = P.wolf_field_scan(a)
    S = energy.System(P.thole_atoms(BASE_R), P.WOLF_BASIS, sc.extra["opts"])
    S.set_polar_wolf(True, a)
    rows = []
    walk(S, sc.points, [], after=lambda S: rows.append(S.dipoles()[1].reshape(-1)))
    assert S.observables["polar_iterations"] == 1 and S.observables["iterator_failed"] == 0
    S.set_polar_wolf(False)
    S.energy()
    plain = S.dipoles()[1].reshape(-1)
    S.close()
    rows = np.array(rows)
    assert np.isfinite(rows).all() and not np.any(rows[:, [1, 2, 4, 5]])
    assert not np.array_equal(plain, rows[-1])  # (the Wolf field was what the scan read: without it the last point has another field)
    sc.check("E0x", rows[:, 0], "energy")
    sc.check("E1x", rows[:, 3], "energy")


# ---- (f) rd_crystal ----------------------------------------------------------------------------------------------------------------------------------------
def test_rd_crystal_order_2():
    sc = P.crystal_scan()
    S = energy.System(P.pair_atoms(BASE_R), P.CUBIC, sc.extra["opts"])
    S.set_rd_crystal(True, 2)
    got = walk(S, sc.points, ["lj_pairs"])
    info = S.rd_crystal_info()
    assert info["n_image_terms"] > 1, info  # (the lattice sum ran: more image terms than the one minimum image)
    S.update_positions(1, at_x(BASE_R))
    trial = walk_trials(S, sc.points, ["lj_pairs"])
    base = dict(S.observables)
    S.close()
    sc.check("lj_pairs", got["lj_pairs"], "energy")
    delta_check(sc, "lj_pairs", trial["lj_pairs"], base, "trial_energy")
