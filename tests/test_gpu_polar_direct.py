"""GPU (MI355X): the direct dipole solve, `polar_iterative off` (csrc/kernels_chol.hip).

Yardsticks: the DIRECT_FIXTURES goldens (the reference's own LU inversion) and the numpy restatement tests/polar_direct_ref.py.
Tolerances (tests/test_polar_direct.py measures the margin: the reference sits within 5e-15 of the refined solution on every fixture,
far inside a quarter of 1e-9, so the contract stands as written): 1e-9 relative for polarization_energy and energy, 1e-9 of the largest
|mu| of the box for the dipoles with an absolute floor of 1e-30 (atoms with alpha = 0 must hold exactly 0 here), ef_static by the
suite's usual per-atom rule.  Run with -s for the measured deviations.
"""
import numpy as np
import pytest

import util
import polar_direct_ref as ref
from mpmcxx_amd import energy, gen_box

pytestmark = pytest.mark.gpu

REL = util.REL_TOL  # 1e-9
MU_FLOOR = 1e-30
NB, PANEL = 64, 192  # kCholNB, kCholPanel (csrc/kernels.h; test_constants_match_the_sources pins them)
E2R = 408.7816
DEBYE2SKA = 85.10597636


def test_constants_match_the_sources():
    txt = util.csrc_text("kernels.h")
    import re

    assert re.findall(r"kCholNB\s*=\s*(\d+)", txt) == [str(NB)] and re.findall(r"kCholPanel\s*=\s*(\d+)", txt) == [str(PANEL)]


@pytest.fixture(scope="module")
def boxes(tmp_path_factory):
    d = tmp_path_factory.mktemp("direct")
    return {name: util.load_generated(name, d) for name in gen_box.DIRECT_FIXTURES}


def check_mu(mu, mu_ref, atoms, label):
    mu, mu_ref = np.asarray(mu).reshape(-1, 3), np.asarray(mu_ref).reshape(-1, 3)
    top = np.abs(mu_ref).max()
    dev = np.abs(mu - mu_ref).max()
    assert dev <= REL * top + MU_FLOOR, f"{label}: mu off by {dev:.3e} (max |mu| {top:.3e}, rel {dev / top if top else 0:.2e})"
    return dev / top if top else 0.0


@pytest.mark.parametrize("name", gen_box.DIRECT_FIXTURES)
def test_golden(boxes, name):
    atoms, basis, o = boxes[name]
    g = util.golden(name)
    S = energy.System(atoms, basis, o)
    T = energy.System(atoms, basis, dict(o, polar_iterative=1))
    try:
        S.energy()
        T.energy()
        r, it = S.observables, T.observables
        for k_ours, k_gold in (("polarization_energy", "polar"), ("energy", "total"), ("NU", "NU")):
            assert util.close(r[k_ours], g[k_gold]), (name, k_ours, r[k_ours], g[k_gold])
        assert r["polar_iterations"] == 0 and r["iterator_failed"] == 0 and r["dipole_rrms"] == 0.0
        assert g["polar_iterations"] == 0 and g["iterator_failed"] == 0
        util.assert_counts(r, g, rd_only=False, label=name)
        # everything that does not depend on the solve: the same bits as the iterative evaluation of the same box
        for k in ("rd_energy", "coulombic_energy", "es_real", "es_recip", "es_self", "lj_pairs", "lrc_pair", "lrc_self", "N", "n_pairs",
                  "n_lj_in_cutoff", "n_es_in_cutoff", "n_intra", "n_rd_excluded", "n_es_excluded", "n_frozen", "vdw_energy", "three_body_energy"):
            assert r[k] == it[k], (name, k, r[k], it[k])
        mu, E, F = S.dipoles()
        sample = np.asarray(g.get("sample_atoms", np.arange(g["natoms"])))
        d = check_mu(mu[sample], g["mu"], atoms, name)
        bad, ratio, _ = util.field_errors(E[sample], g["ef_static"])
        assert bad.size == 0, (name, "ef_static", ratio)
        al = np.asarray(atoms["polarizability"])
        assert not np.any(mu[al == 0.0]) and not np.any(F[al == 0.0])
        pol = al != 0.0
        want_F = mu[pol] / al[pol, None] - E[pol]
        assert np.array_equal(F[pol], want_F), "ef_induced = mu / alpha - ef_static"
        info = S.direct_info()
        assert info["n_unknowns"] == 3 * int(pol.sum()) and info["status"] == 0
        assert info["residual"] <= 4 * info["n_unknowns"] * 2.0 ** -53, info
        total, _ = S.memory_usage()
        assert info["factor_bytes"] >= 8 * info["n_unknowns"] ** 2 and total >= info["factor_bytes"]
        print(f"\n{name}: polar rel {abs(r['polarization_energy'] - g['polar']) / abs(g['polar']):.2e} mu {d:.2e} residual {info['residual']:.2e}")
    finally:
        S.close()
        T.close()


def ladder_box(n_pol, cell, seed, ewald):
    """n_pol polarizable atoms and n_pol // 3 + 2 atoms with alpha = 0 on a jittered lattice (45 A^3 per atom), molecules of 1-3 sites, one
    molecule in eight frozen, a quarter of the charges zero"""
    rng = np.random.default_rng(seed)
    n = n_pol + n_pol // 3 + 2
    L = (45.0 * n) ** (1.0 / 3.0)
    basis = np.diag([L, L, L]) if cell == "cubic" else L * np.array([[1.0, 0.0, 0.0], [0.17, 1.0, 0.0], [-0.12, 0.21, 1.0]])
    g = int(np.ceil(n ** (1.0 / 3.0)))
    sites = rng.permutation(g ** 3)[:n]
    ijk = np.stack([sites // (g * g), (sites // g) % g, sites % g], axis=1).astype(np.float64)
    pos = ((ijk + 0.5 + rng.uniform(-0.1, 0.1, size=ijk.shape)) / g - 0.5) @ basis
    al = np.zeros(n)
    al[rng.permutation(n)[:n_pol]] = rng.uniform(0.3, 1.5, n_pol)
    sizes = rng.choice([1, 1, 2, 3], size=n)
    mol = np.repeat(np.arange(n), sizes)[:n].astype(np.int32)
    frozen = (rng.random(n) < 0.125)[mol].astype(np.int32)
    q = np.where(rng.random(n) < 0.25, 0.0, rng.uniform(-0.9, 0.9, n) * E2R)
    atoms = {"pos": pos, "charge": q, "polarizability": al, "epsilon": rng.uniform(5.0, 150.0, n), "sigma": rng.uniform(2.0, 3.4, n),
             "mol_id": mol, "frozen": frozen, "mass": rng.uniform(1.0, 40.0, n)}
    o = {"rd_only": 0, "rd_lrc": 1, "polarization": 1, "polar_iterative": 0, "polar_ewald": int(ewald), "polar_max_iter": 10, "polar_gs": 0,
         "polar_rrms": 0, "ewald_kmax": 7, "polar_precision": 0.0, "polar_gamma": 1.0, "polar_damp": 2.1304, "damp_type": "exponential",
         "ewald_alpha": None, "polar_ewald_alpha": None, "wolf": 0, "feynman_hibbs": 0, "feynman_hibbs_order": 0, "temperature": 0.0}
    return atoms, basis, o


# every block edge of the factorisation in unknowns (3 n_pol): the 64-wide block (21 | 22 atoms), the 192-wide panel (64 | 65; 128 | 129:
# the first box with a trailing update behind a panel, then two), the 256-atom row of the build's grid, the 1024-slot chunk of the index
# kernel (n = n_pol + n_pol / 3 + 2 atoms: 766 -> 1023, 767 -> 1024, 768 -> 1026), and the sizes the issue names
LADDER = [1, 2, 21, 22, 63, 64, 65, 128, 129, 255, 256, 257, 766, 767, 768, 1000, 2000]


@pytest.mark.parametrize("n_pol", LADDER)
def test_size_ladder_against_the_restatement(n_pol):
    k = LADDER.index(n_pol)
    cell, ewald = ("cubic", "triclinic")[k % 2], (k // 2) % 2 == 0 or n_pol < 22  # (no-PBC fields need a box that is not tiny)
    atoms, basis, o = ladder_box(n_pol, cell, 7000 + n_pol, ewald)
    S = energy.System(atoms, basis, o)
    try:
        S.energy()
        r = S.observables
        want = ref.solve(atoms, basis, o)
        assert np.all(np.linalg.eigvalsh(want["A"]) > 0), "the ladder box must be positive definite"
        info = S.direct_info()
        assert info["status"] == 0 and r["iterator_failed"] == 0 and info["n_unknowns"] == 3 * n_pol, (info, r["iterator_failed"])
        mu, E, _ = S.dipoles()
        bad, ratio, _ = util.field_errors(E, want["ef_static"])
        assert bad.size == 0, (n_pol, "ef_static", ratio)
        # the restatement's E0 is the oracle's; the energy is compared with the restated solve of OUR field too, so that a 1e-9-level
        # difference of the fields is not charged to the solve
        d = check_mu(mu, ref.solve(atoms, basis, o, E0=E)["mu"], atoms, f"n_pol {n_pol} (own field)")
        check_mu(mu, want["mu"], atoms, f"n_pol {n_pol}")
        assert util.close(r["polarization_energy"], want["polarization_energy"]), (n_pol, r["polarization_energy"], want["polarization_energy"])
        assert info["residual"] <= 4 * max(info["n_unknowns"], 64) * 2.0 ** -53, info
        print(f"\nn_pol {n_pol} {cell} ewald {int(ewald)}: mu {d:.2e} residual {info['residual']:.2e}")
    finally:
        S.close()


def test_iterative_solve_with_a_tight_precision_agrees(boxes):
    """two independent device paths.  Jacobi stops when every |d mu| < p DEBYE2SKA; its iteration matrix has spectral radius
    rho <= (cond - 1) / (cond + 1) = 0.19 at cond(A) = 1.455 (test_polar_direct), so the converged dipoles are within
    p DEBYE2SKA rho / (1 - rho) < p DEBYE2SKA of the exact ones (2 p DEBYE2SKA allowed), the energy within 0.5 sum |E0| times that."""
    atoms, basis, o = boxes["ion216_polar_direct"]
    p = 1e-10
    S = energy.System(atoms, basis, o)
    T = energy.System(atoms, basis, dict(o, polar_iterative=1, polar_precision=p))
    try:
        S.energy()
        T.energy()
        assert T.observables["iterator_failed"] == 0 and T.observables["polar_iterations"] > 5
        mu_d, E, _ = S.dipoles()
        mu_i, _, _ = T.dipoles()
        bound = 2 * p * DEBYE2SKA
        assert np.abs(mu_d - mu_i).max() <= bound, (np.abs(mu_d - mu_i).max(), bound)
        assert abs(S.observables["polarization_energy"] - T.observables["polarization_energy"]) <= 0.5 * np.abs(E).sum() * bound
    finally:
        S.close()
        T.close()


def test_trial_moves_box_change_growth(boxes):
    atoms, basis, o = boxes["water64_polar_direct"]
    S = energy.System(atoms, basis, o)
    try:
        S.energy()
        mols = util.molecules(atoms)
        pos = atoms["pos"].copy()
        for step, (mi, accept) in enumerate([(3, True), (10, False), (20, True), (3, True)]):
            first, end = mols[mi]
            new = util.moved(util.with_positions(atoms, pos), first, end - first, 100 + step, sigma=0.15)
            S.trial_energy(first, new)
            assert S.last_trial_was_full()
            trial = pos.copy()
            trial[first:end] = new
            util.check_trial_against_fresh(S, atoms, basis, o, trial, label=f"trial {step}")
            if accept:
                S.accept()
                pos = trial
            else:
                S.reject()
            S.energy()
            F = energy.System(util.with_positions(atoms, pos), basis, o)
            F.energy()
            bad = util.component_errors(S.observables, F.observables, util.TRIAL_KEYS, 1e-11)
            assert not bad, f"after {'accept' if accept else 'reject'} {step}: {bad}"
            F.close()
        # a box change
        b2 = np.asarray(basis) * 1.03
        S.set_box(b2)
        S.update_positions(0, pos * 1.03)
        S.energy()
        F = energy.System(util.with_positions(atoms, pos * 1.03), b2, o)
        F.energy()
        assert not util.component_errors(S.observables, F.observables, util.TRIAL_KEYS, 1e-11)
        F.close()
        # an atom list that grows past the capacity (193 -> 3 x 193 atoms in a 3 x 1 x 1 supercell)
        big = {k: np.concatenate([v] * 3) for k, v in atoms.items()}
        big["pos"] = np.concatenate([atoms["pos"] + s * np.asarray(basis)[0] for s in (-1, 0, 1)])
        big["mol_id"] = np.concatenate([atoms["mol_id"] + s * (int(atoms["mol_id"].max()) + 1) for s in (0, 1, 2)]).astype(np.int32)
        b3 = np.asarray(basis) * np.array([[3.0], [1.0], [1.0]])
        S.set_box(b3)
        S.set_atoms(big)
        S.energy()
        F = energy.System(big, b3, o)
        F.energy()
        assert not util.component_errors(S.observables, F.observables, util.TRIAL_KEYS, 1e-11)
        assert S.direct_info()["n_unknowns"] == F.direct_info()["n_unknowns"] == 3 * int((big["polarizability"] != 0).sum())
        want = ref.solve(big, b3, o)
        check_mu(S.dipoles()[0], want["mu"], big, "grown box")
        F.close()
    finally:
        S.close()


def test_pi_beads_and_gibbs(boxes):
    atoms, basis, o = boxes["ion216_polar_direct"]
    rng = np.random.default_rng(11)
    beads_pos = [atoms["pos"] + rng.normal(scale=0.05, size=atoms["pos"].shape) for _ in range(4)]
    beads = [energy.System(util.with_positions(atoms, p), basis, o) for p in beads_pos]
    try:
        sums, per, failed = energy.pi_potential_local(beads)
        assert not failed
        singles = []
        for p in beads_pos:
            F = energy.System(util.with_positions(atoms, p), basis, o)
            F.energy()
            singles.append(dict(F.observables))
            F.close()
        for b, s in zip(per, singles):  # (1e-11: the suite's bound between two contexts of one configuration)
            assert not util.component_errors(b, s, util.TRIAL_KEYS, 1e-11)
            assert b["polar_iterations"] == 0 and b["iterator_failed"] == 0
        acc = 0.0
        for b in per:
            acc += b["polarization_energy"]
        assert sums[2] == acc
        ea, eb = energy.gibbs_energy(beads[0], beads[1])
        assert abs(ea - singles[0]["energy"]) <= 1e-11 * abs(ea) and abs(eb - singles[1]["energy"]) <= 1e-11 * abs(eb)
    finally:
        for b in beads:
            b.close()


def test_three_evaluations_give_the_same_bits(boxes):
    atoms, basis, o = boxes["ion1000_polar_direct"]
    S = energy.System(atoms, basis, o)
    try:
        runs = []
        for _ in range(3):
            S.energy()
            runs.append((dict(S.observables), [a.copy() for a in S.dipoles()], S.direct_info()))
        for obs, dip, info in runs[1:]:
            assert obs == runs[0][0] and info == runs[0][2]
            assert all(np.array_equal(a, b) for a, b in zip(dip, runs[0][1]))
    finally:
        S.close()


def test_a_matrix_that_is_not_positive_definite_is_reported_not_solved():
    """two strongly polarizable atoms 1.5 A apart with almost no damping: the pair's block has the eigenvalue 1/alpha - 2/r^3 < 0 (confirmed
    with eigvalsh below before anything runs).  A handled numerical condition: iterator_failed = 1, zeros, and the context stays usable."""
    L = 30.0
    basis = np.diag([L, L, L])
    pos = np.array([[0.0, 0.0, 0.0], [1.5, 0.0, 0.0], [6.0, 1.0, 0.0], [-5.0, 4.0, 2.0], [3.0, -7.0, 5.0], [-4.0, -4.0, -6.0]])
    n = len(pos)
    atoms = {"pos": pos, "charge": np.array([0.3, -0.3, 0.5, -0.5, 0.4, -0.4]) * E2R, "polarizability": np.array([10.0, 10.0, 1.0, 1.0, 0.0, 1.2]),
             "epsilon": np.full(n, 50.0), "sigma": np.full(n, 3.0), "mol_id": np.arange(n, dtype=np.int32), "frozen": np.zeros(n, dtype=np.int32),
             "mass": np.full(n, 10.0)}
    _, _, o = ladder_box(4, "cubic", 1, True)
    o = dict(o, polar_damp=20.0)
    A, _ = ref.amatrix(atoms, basis, o)
    assert np.linalg.eigvalsh(A).min() < -0.1
    S = energy.System(atoms, basis, o)
    try:
        S.energy()
        r = S.observables
        assert r["iterator_failed"] == 1 and r["polar_iterations"] == 0 and r["polarization_energy"] == 0.0
        assert all(np.isfinite(r[k]) for k in ("energy", "rd_energy", "coulombic_energy", "NU"))
        info = S.direct_info()
        assert 1 <= info["status"] <= info["n_unknowns"] == 15, info
        assert b"pivot" in S._L.mpmc_last_error(S._h)
        mu, _, F = S.dipoles()
        assert not np.any(mu) and not np.any(F)
        # a healthy configuration in the same context afterwards
        good = pos.copy()
        good[1] = [4.0, 0.0, 0.0]
        S.update_positions(0, good)
        S.energy()
        g_atoms = util.with_positions(atoms, good)
        want = ref.solve(g_atoms, basis, o)
        assert np.linalg.eigvalsh(want["A"]).min() > 0
        assert S.observables["iterator_failed"] == 0 and S.direct_info()["status"] == 0
        check_mu(S.dipoles()[0], want["mu"], g_atoms, "healthy after failed")
        assert util.close(S.observables["polarization_energy"], want["polarization_energy"])
    finally:
        S.close()


def test_size_guard(boxes):
    """216 polarizable atoms: 648 unknowns padded to 768, a factor of 768^2 doubles = 4.5 MB.  A budget of 4 MB refuses it with
    memory_request_fail (2000) and names the size; nothing of that size is allocated; 5 MB lets it through."""
    atoms, basis, o = boxes["ion216_polar_direct"]
    S = energy.System(atoms, basis, o)
    try:
        S.configure("direct_budget_mb", 4)
        with pytest.raises(energy.MpmcError) as ei:
            S.energy()
        assert ei.value.code == 2000 and "4.5 MB" in str(ei.value) and "648 unknowns" in str(ei.value), str(ei.value)
        assert S.direct_info()["factor_bytes"] == 0
        S.configure("direct_budget_mb", 5)
        S.energy()
        assert util.close(S.observables["polarization_energy"], util.golden("ion216_polar_direct")["polar"])
        assert S.direct_info()["factor_bytes"] == 768 * 768 * 8
    finally:
        S.close()


def test_benchmark_box_10k_residuals(tmp_path):
    """the 10 000-atom benchmark box: the reported residual, and the residual recomputed on the host from mpmc_thole_amatrix rows (fetched
    in chunks from a second context) and the returned dipoles.  Bound: a backward-stable solve leaves |r| <= c n eps |A| |mu|; relative to
    max |E0| at cond(A) ~ 1.5 that is n 2^-53 up to a small factor (4 allowed)."""
    atoms, basis, o = util.load_generated("ion10k_polar", tmp_path)
    o = dict(o, polar_iterative=0)
    S = energy.System(atoms, basis, o)
    try:
        S.energy()
        info = S.direct_info()
        n = S.n
        assert info["status"] == 0 and info["n_unknowns"] == 3 * n and S.observables["iterator_failed"] == 0
        bound = 4 * 3 * n * 2.0 ** -53
        assert info["residual"] <= bound, (info, bound)
        mu, E, _ = S.dipoles()
        x = mu.reshape(-1)
        rmax, chunk = 0.0, 600
        for row0 in range(0, 3 * n, chunk):
            rows = min(chunk, 3 * n - row0)
            A = S.thole_amatrix(row0, rows)
            rmax = max(rmax, float(np.abs(E.reshape(-1)[row0:row0 + rows] - A @ x).max()))
        host = rmax / np.abs(E).max()
        assert host <= bound, (host, bound)
        print(f"\nion10k direct: polarization {S.observables['polarization_energy']!r} residual reported {info['residual']:.2e} host {host:.2e}")
    finally:
        S.close()
