"""GPU (MI355X): `polar_wolf` (the Wolf static field, csrc/kernels_wolf_field.hip) and `polar_palmo` (the Palmo-Krimm correction).

Yardsticks: the WOLF_FIXTURES goldens (the reference's own object code) and the numpy restatement tests/polar_wolf_ref.py, which sits
within 4e-15 of those goldens (tests/test_polar_wolf.py, profiles/polar_wolf_margin.txt).  Tolerances: 1e-9 relative per energy component
against a golden, per-atom arrays by the suite's rule (util.field_errors: 1e-9 |ref_i| + 1e-12 max |ref|), counts and iteration numbers
exact; against the restatement 1e-9 plus its margin (REF_REL).  The Palmo-Krimm correction is compared with (golden with palmo - golden
without) at 1e-9 |U_pol| absolute, since both goldens are only that good.  Run with -s for the measured deviations.
"""
import numpy as np
import pytest

import util
import polar_wolf_ref as ref
from mpmcxx_amd import energy, gen_box

pytestmark = pytest.mark.gpu

REL = util.REL_TOL            # 1e-9
REF_REL = REL + 4e-15         # the restatement's own margin against the reference (profiles/polar_wolf_margin.txt)
KEYS = ["energy", "rd_energy", "coulombic_energy", "polarization_energy", "es_real", "es_recip", "lj_pairs"]


@pytest.fixture(scope="module")
def boxes(tmp_path_factory):
    d = tmp_path_factory.mktemp("wolf")
    return {name: util.load_generated(name, d) for name in gen_box.WOLF_FIXTURES}


def against_golden(S, atoms, o, name, label=None):
    """one evaluated System against the golden `name`: components, counts, iteration numbers, per-atom arrays"""
    g = ref.golden(name)
    label = label or name
    r = S.observables
    util.assert_energies(r, g, False, label=label)
    util.assert_counts(r, g, rd_only=False, label=label)
    assert util.close(r["NU"], g["NU"]), (label, r["NU"], g["NU"])
    assert r["polar_iterations"] == g["polar_iterations"] and r["iterator_failed"] == g["iterator_failed"], (label, r["polar_iterations"], g["polar_iterations"])
    mu, E, F = S.dipoles()
    sample = np.asarray(g.get("sample_atoms", np.arange(g["natoms"])))
    devs = {}
    # (the reference never writes ef_induced on the direct path: its golden holds zeros there)
    for k, got in (("ef_static", E), ("mu", mu)) + ((("ef_induced", F),) if o["polar_iterative"] else ()):
        bad, ratio, _ = util.field_errors(got[sample], g[k])
        assert bad.size == 0, (label, k, bad[:5], ratio)
        devs[k] = ratio
    assert not np.any(mu[np.asarray(atoms["polarizability"]) == 0.0])
    print(f"\n{label}: polar rel {abs(r['polarization_energy'] - g['polar']) / abs(g['polar']):.2e} fields (fraction of bound) "
          + " ".join(f"{k} {v:.2e}" for k, v in devs.items()))
    return g


@pytest.mark.parametrize("name", [n for n in gen_box.WOLF_FIXTURES if n != "ion4000_pw1_gsp"])
def test_golden(boxes, name):
    atoms, basis, o = boxes[name]
    S = energy.System(atoms, basis, o)
    try:
        S.energy()
        against_golden(S, atoms, o, name)
        a = S.observables.copy()
        S.energy()
        assert S.observables == a, "a repeated evaluation must give the same bits"
    finally:
        S.close()


def test_large_box_with_a_large_alpha_r(boxes):
    """4000 atoms, polar_wolf_alpha 1 at R = 32 A: erfc and the Gaussian at arguments up to 32, most of them exact zeros in fp64"""
    name = "ion4000_pw1_gsp"
    atoms, basis, o = boxes[name]
    S = energy.System(atoms, basis, o)
    try:
        S.energy()
        against_golden(S, atoms, o, name)
    finally:
        S.close()


@pytest.mark.parametrize("base", gen_box.WOLF_BASES + ["ion216_polar_pw0"])
def test_palmo_correction(boxes, base):
    stem = base if base.endswith("pw0") else base + "_pw"
    atoms, basis, o = boxes[f"{stem}_gsp"]
    S = energy.System(atoms, basis, o)
    try:
        S.energy()
        corr, change = S.palmo_info()
        want = ref.solve(atoms, basis, o)
        u = abs(want["polarization_energy"])
        if not base.endswith("pw0"):
            gold = ref.golden(f"{stem}_gsp")["polar"] - ref.golden(f"{stem}_gs")["polar"]
            assert abs(corr - gold) <= REL * u, (base, corr, gold)
        assert abs(corr - want["correction"]) <= REF_REL * u, (base, corr, want["correction"])
        bad, ratio, _ = util.field_errors(change, want["ef_induced_change"], rel=REF_REL, absolute=REF_REL * np.abs(want["ef_induced"]).max())
        # (ef_induced_change is a difference of two induced fields that agree to a few digits: its error is that of the fields)
        assert bad.size == 0, (base, bad[:5], ratio)
        assert not np.any(change[np.asarray(atoms["polarizability"]) == 0.0])
        mu, _, _ = S.dipoles()
        assert abs(-0.5 * (mu * change).sum() - corr) <= 1e-15 * u  # (two orders of summation of one 216-term sum)
        print(f"\n{base}: correction {corr:.9e} (restatement {want['correction']:.9e}), of U_pol {corr / u:.2e}")
        # exactly zero under Jacobi and under the direct solve, and the bits of a context without the option
        for variant in ({"polar_gs": 0, "polar_max_iter": 10}, {"polar_iterative": 0}):
            o2 = dict(o, **variant)
            T, U = energy.System(atoms, basis, o2), energy.System(atoms, basis, dict(o2, polar_palmo=0))
            try:
                T.energy(), U.energy()
                c2, ch2 = T.palmo_info()
                assert c2 == 0.0 and not np.any(ch2), (base, variant, c2)
                assert T.observables == U.observables, (base, variant)
            finally:
                T.close(), U.close()
    finally:
        S.close()


@pytest.mark.parametrize("solver", ["matrix_free", "compact", "dense"])
@pytest.mark.parametrize("name", ["ion216_polar_pw_jac", "ion216_triclinic_pw_jac", "water64_polar_pw_gsp", "ion1000_gs_pw_gsp"])
def test_every_solver_and_pair_kernel(boxes, name, solver):
    """every `solver` value; the generic pair kernel and the fast sweep (forced by the switch the size-ladder tests use) with the field
    part off; repeated evaluations bit-identical"""
    atoms, basis, o = boxes[name]
    seen = []
    for pair_kernel in (1, 2):
        S = energy.System(atoms, basis, dict(o, solver=solver))
        try:
            S.configure("pair_kernel", pair_kernel)
            S.energy()
            assert S.last_pair_kernel() == ("fused" if pair_kernel == 1 else "sweep")
            against_golden(S, atoms, o, name, label=f"{name}/{solver}/pair_kernel {pair_kernel}")
            a = S.observables.copy()
            d = [x.copy() for x in S.dipoles()]
            S.energy()
            assert S.observables == a and all(np.array_equal(x, y) for x, y in zip(d, S.dipoles()))
            seen.append(d[1])
        finally:
            S.close()
    assert np.array_equal(seen[0], seen[1]), "the Wolf field does not depend on the pair kernel"


def test_field_entry_point_and_timing_slots(boxes):
    atoms, basis, o = boxes["ion216_polar_pw_gsp"]
    S = energy.System(atoms, basis, o)
    try:
        E = S.thole_field()
        bad, ratio, _ = util.field_errors(E, ref.golden("ion216_polar_pw_gsp")["ef_static"])
        assert bad.size == 0, ratio
        bad, ratio, _ = util.field_errors(E, ref.wolf_field(atoms, basis, 0.13), rel=REF_REL)
        assert bad.size == 0, ratio
        assert util.close(S.polar(), ref.golden("ion216_polar_pw_gsp")["polar"])
        S.set_profiling(True)
        S.timings(reset=True)
        S.energy()
        t = S.timings()
        assert t["field"]["launches"] >= 1 and t["recip"]["launches"] >= 1  # (the Coulomb energy still has its reciprocal part)
        assert t["dipole_iter"]["launches"] == 4 + 1, t["dipole_iter"]       # four sweeps and the Palmo-Krimm contraction
    finally:
        S.close()


@pytest.mark.parametrize("name,sizes", [("ion216_polar_pw_gsp", (1, 3, 64)), ("water64_polar_pw_gsp", (1, 3, 64))])
def test_trial_moves(boxes, name, sizes):
    """accepted and rejected moves of 1, 3 and 64 atoms on the delta path, each against the restatement; a full evaluation afterwards agrees"""
    atoms, basis, o = boxes[name]
    S = energy.System(atoms, basis, o)
    try:
        S.energy()
        pos = atoms["pos"].copy()
        n = pos.shape[0]
        step = 0
        for m in sizes:
            for accept in (True, False):
                first = (37 * (step + 1)) % (n - m)
                if m == 3 and name.startswith("water"):
                    first, _ = util.molecules(atoms)[5 + step]
                new = util.moved(util.with_positions(atoms, pos), first, m, 300 + step, sigma=0.12)
                S.trial_energy(first, new)
                assert not S.last_trial_was_full(), (name, m)
                trial = pos.copy()
                trial[first:first + m] = new
                want = ref.solve(util.with_positions(atoms, trial), basis, o)
                got = S.trial_observables
                assert abs(got["polarization_energy"] - want["polarization_energy"]) <= REF_REL * abs(want["polarization_energy"]), (name, m, accept)
                assert got["polar_iterations"] == want["polar_iterations"]
                corr, _ = S.palmo_info()
                assert abs(corr - want["correction"]) <= REF_REL * abs(want["polarization_energy"])
                util.check_trial_against_fresh(S, atoms, basis, o, trial, rel=REL, label=f"{name} m {m}")
                if accept:
                    S.accept()
                    pos = trial
                else:
                    S.reject()
                step += 1
        S.energy()
        F = energy.System(util.with_positions(atoms, pos), basis, o)
        try:
            F.energy()
            assert not util.component_errors(S.observables, F.observables, KEYS, 1e-11)
        finally:
            F.close()
    finally:
        S.close()


def test_trial_moves_that_fall_back_to_a_full_evaluation(boxes):
    """m > MPMC_TRIAL_MAX_ATOMS (256) on the 1000-atom box, and opts.wolf: a full evaluation of the trial configuration, the same answer"""
    for name, m, extra in (("ion1000_gs_pw_gsp", 300, {}), ("ion216_polar_pw_gsp", 3, {"wolf": 1})):
        atoms, basis, o = boxes[name]
        o = dict(o, **extra)
        S = energy.System(atoms, basis, o)
        try:
            S.energy()
            new = util.moved(atoms, 10, m, 77, sigma=0.1)
            S.trial_energy(10, new)
            assert S.last_trial_was_full(), name
            trial = atoms["pos"].copy()
            trial[10:10 + m] = new
            util.check_trial_against_fresh(S, atoms, basis, o, trial, rel=1e-11, label=name)
            want = ref.solve(util.with_positions(atoms, trial), basis, o)
            assert abs(S.trial_observables["polarization_energy"] - want["polarization_energy"]) <= REF_REL * abs(want["polarization_energy"])
            S.reject()
        finally:
            S.close()


def test_lifecycle(boxes):
    atoms, basis, o = boxes["ion216_polar_pw_gsp"]
    plain = {k: v for k, v in o.items() if k not in ("polar_wolf", "polar_wolf_alpha", "polar_palmo")}
    L = energy.lib()
    S, P = energy.System(atoms, basis, o), energy.System(atoms, basis, plain)
    try:
        S.energy(), P.energy()
        assert S.observables["polarization_energy"] != P.observables["polarization_energy"]
        # enabled = 0: the bits of a context that never called the setters
        S.set_polar_wolf(False)
        S.set_polar_palmo(False)
        S.energy()
        assert S.observables == P.observables and all(np.array_equal(a, b) for a, b in zip(S.dipoles(), P.dipoles()))
        assert S.palmo_info()[0] == 0.0
        # back on; the settings survive set_options, set_box (R changes: the cutoff term follows) and set_atoms with growth
        S.set_polar_wolf(True, 0.13)
        S.set_polar_palmo(True)
        S._check(L.mpmc_set_options(S.handle, energy.C.byref(energy.make_options(o))))
        S.energy()
        against_golden(S, atoms, o, "ion216_polar_pw_gsp", label="after set_options")
        b2 = np.asarray(basis) * 1.04
        S.set_box(b2)
        S.update_positions(0, atoms["pos"] * 1.04)
        S.energy()
        scaled = util.with_positions(atoms, atoms["pos"] * 1.04)
        want = ref.solve(scaled, b2, o)
        assert abs(S.observables["polarization_energy"] - want["polarization_energy"]) <= REF_REL * abs(want["polarization_energy"])
        bad, ratio, _ = util.field_errors(S.dipoles()[1], want["ef_static"], rel=REF_REL)
        assert bad.size == 0, ratio
        big, bbasis, _ = boxes["ion1000_gs_pw_gsp"]  # more atoms than the context was made for
        S.set_box(bbasis)
        S.set_atoms(big)
        S.energy()
        against_golden(S, big, o, "ion1000_gs_pw_gsp", label="after growth")
        # refusals
        for bad_alpha in (-0.1, 1.5, float("nan"), float("inf")):
            assert L.mpmc_set_polar_wolf(S.handle, 1, bad_alpha) == 4000, bad_alpha
        S.energy()
        against_golden(S, big, o, "ion1000_gs_pw_gsp", label="after refused settings")
        for bit in (8, 9):
            with pytest.raises(energy.MpmcError) as e:
                energy.System(atoms, basis, dict(o, unsupported_flags=1 << bit))
            assert e.value.code == 4004
    finally:
        S.close(), P.close()


def test_pi_bead_sums_and_gibbs(boxes):
    atoms, basis, o = boxes["water64_polar_pw_gsp"]
    beads, singles = [], []
    try:
        for b in range(4):
            p = gen_box.bead_positions(atoms["pos"], b)
            beads.append(energy.System(util.with_positions(atoms, p), basis, o))
            singles.append(energy.System(util.with_positions(atoms, p), basis, o))
        sums, per, failed = energy.pi_potential_local(beads)
        assert not failed
        for k, s in enumerate(singles):
            s.energy()
            assert per[k]["polarization_energy"] == s.observables["polarization_energy"] and per[k]["energy"] == s.observables["energy"]
            want = ref.solve(util.with_positions(atoms, gen_box.bead_positions(atoms["pos"], k)), basis, o)
            assert abs(per[k]["polarization_energy"] - want["polarization_energy"]) <= REF_REL * abs(want["polarization_energy"])
        assert sums[2] == sum(float(per[k]["polarization_energy"]) for k in range(4)) or util.close(sums[2], sum(per[k]["polarization_energy"] for k in range(4)), 1e-15)
        ea, eb = energy.gibbs_energy(beads[0], beads[1])
        assert ea == singles[0].observables["energy"] and eb == singles[1].observables["energy"]
    finally:
        for s in beads + singles:
            s.close()
