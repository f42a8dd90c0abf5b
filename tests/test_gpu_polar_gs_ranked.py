"""GPU (MI355X): `polar_gs_ranked` (mpmc_set_polar_gs_ranked: the rank pass and the sweep order of kernels_gs_rank.hip, the Gauss-Seidel
pipeline of kernels_gs.hip on the ranked view from the second iteration on).

Yardsticks: the GS_RANKED_FIXTURES goldens (the reference's own object code) with util.assert_matches_oracle's bounds -- 1e-9 relative per
energy component with no floor, iterations and iterator_failed equal, the per-atom fields as that function states -- and the numpy
restatement tests/polar_gs_ranked_ref.py, which sits within 1.3e-15 (energy) and 2.7e-15 (per-atom arrays) of those goldens
(tests/test_polar_gs_ranked.py) and whose rank pass runs in the reference's operation order: rmin must be its double, rank_metric and the
order its integers.  Run with -s for the measured deviations.
"""
import numpy as np
import pytest

import util
import polar_gs_ranked_ref as ref
from test_polar_gs_ranked import WORST, load_ranked
from mpmcxx_amd import energy, gen_box

pytestmark = pytest.mark.gpu

REL = util.REL_TOL                      # 1e-9
REF_REL_E = REL + 10.0 * WORST["energy"]  # ... plus ten times the restatement's own distance from the reference
REF_REL_MU = REL + 10.0 * WORST["mu"]
FLAG_POLAR_GS_RANKED = 1 << 10
ERR_INVALID_SETTING, ERR_UNSUPPORTED, ERR_ARG = 4000, 4004, -3
# the fixtures of the issue's table whose reference energies differ between ranked and plain sweeps (by 6.7e-7 relative at least)
APART = ["ion216_polar_gr_it2", "ion216_polar_gr_it4", "ion216_polar_nopbc_gr_it4", "water64_polar_gr_it4", "ion1000_gs_gr_it4"]


@pytest.fixture(scope="module")
def boxes(tmp_path_factory):
    d = tmp_path_factory.mktemp("gs_ranked")
    return {name: load_ranked(name, d) for name in gen_box.GS_RANKED_FIXTURES}


def plain_gs(o):
    return dict(o, polar_gs_ranked=0, polar_gs=1)


def oracle_of(name):
    """the golden `name` in the shape util.assert_matches_oracle compares with (the oracle's key names), and its sample of atoms"""
    g = ref.golden(name)
    o = {ours: g[gold] for ours, gold in util.ENERGY_KEYS}
    for k in util.COUNT_KEYS + ["n_es_in_cutoff", "polar_iterations", "iterator_failed", "dipole_rrms", "ef_static", "mu", "ef_induced"]:
        o[k] = g[k]
    return o, np.asarray(g["sample_atoms"])


def against_golden(S, atoms, o, name, label=None):
    want, sample = oracle_of(name)
    devs = {}
    dip = tuple(x[sample] for x in S.dipoles())
    util.assert_matches_oracle(S.observables, dip, want, {"polarizability": np.asarray(atoms["polarizability"])[sample]}, o, label=label or name,
                               deviations=devs)
    print(f"\n{label or name}: " + " ".join(f"{k} {v:.1e}" for k, v in devs.items() if v))


def against_rank_pass(S, atoms, basis, sweeps, label):
    """rmin the restatement's double, rank_metric and the order its integers, the info block what the evaluation did"""
    rmin, rank, order = ref.rank_pass(atoms, basis)
    info = S.polar_gs_ranked_info()
    got_rank, got_order = S.polar_gs_ranked()
    assert info["rmin"] == rmin, (label, info["rmin"].hex(), float(rmin).hex())
    assert np.array_equal(got_rank, rank) and np.array_equal(got_order, order), label
    assert info["enabled"] == 1 and info["acted"] == 1 and info["max_rank"] == int(rank.max()), (label, info)
    assert info["n_moved"] == int(np.count_nonzero(order != np.arange(order.size))) and info["ranked_sweeps"] == sweeps, (label, info)
    return info


def snapshot(S):
    return dict(S.observables), [x.copy() for x in S.dipoles()]


def same_bits(a, b):
    return a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))


def evaluated(atoms, basis, o):
    S = energy.System(atoms, basis, o)
    try:
        S.energy()
        return snapshot(S)
    finally:
        S.close()


@pytest.mark.parametrize("name", gen_box.GS_RANKED_FIXTURES)
def test_golden(boxes, name):
    atoms, basis, o = boxes[name]
    S = energy.System(atoms, basis, o)
    try:
        S.energy()
        against_golden(S, atoms, o, name)
        g = ref.golden(name)
        against_rank_pass(S, atoms, basis, g["polar_iterations"] - 1, name)
        relax = S.polar_relax_info()
        assert relax["contractions"] == g["polar_iterations"] + (1 if o.get("polar_palmo") else 0) and relax["store_filled"] == 0, relax
        assert S.palmo_info()[0] != 0.0 if o.get("polar_palmo") else S.palmo_info()[0] == 0.0
        a = snapshot(S)
        S.energy()
        assert same_bits(a, snapshot(S)), "a repeated evaluation must give the same bits"
    finally:
        S.close()


@pytest.mark.parametrize("name", APART)
def test_ranked_sweeps_are_not_plain_sweeps(boxes, name):
    """the device's own polar_gs energy is further from its ranked energy than 100 times the bound of the golden comparison: that
    comparison cannot be passed by sweeping in atom order"""
    atoms, basis, o = boxes[name]
    ranked, plain = evaluated(atoms, basis, o)[0]["polarization_energy"], evaluated(atoms, basis, plain_gs(o))[0]["polarization_energy"]
    print(f"\n{name}: ranked {ranked!r} polar_gs {plain!r} rel {abs(ranked - plain) / abs(plain):.2e}")
    assert abs(ranked - plain) > 100.0 * REL * abs(plain)


@pytest.mark.parametrize("name", ["ion216_polar_gr_it1", "ion216_triclinic_gr_it4"])
def test_equal_to_polar_gs_to_the_bit(boxes, name):
    """one sweep: no ranked sweep happens.  The triclinic box: by the unwrapped distance every rank is 0 and the order is the identity."""
    atoms, basis, o = boxes[name]
    S = energy.System(atoms, basis, o)
    try:
        S.energy()
        info = S.polar_gs_ranked_info()
        assert info["acted"] == 1 and info["ranked_sweeps"] == (0 if name.endswith("it1") else 3), info
        if "triclinic" in name:
            assert info["n_moved"] == 0 and info["max_rank"] == 0, info
        assert same_bits(snapshot(S), evaluated(atoms, basis, plain_gs(o)))
    finally:
        S.close()


MATRIX = {"ewald": {"polar_ewald": 1}, "nopbc": {"polar_ewald": 0}, "wolf": {"polar_ewald": 0, "polar_wolf": 1, "polar_wolf_alpha": 0.13},
          "rrms": {"polar_rrms": 1}, "precision": {"polar_precision": 1e-6, "polar_rrms": 1}, "sor": {"polar_sor": 1, "polar_gamma": 0.9, "polar_max_iter": 5},
          "esor_palmo": {"polar_esor": 1, "polar_gamma": 0.7, "polar_max_iter": 5, "polar_palmo": 1}}


@pytest.mark.parametrize("case", sorted(MATRIX))
def test_matrix_against_the_restatement(boxes, case):
    atoms, basis, base = boxes["ion216_polar_gr_it4"]
    o = dict(base, polar_max_iter=3)
    o.update(MATRIX[case])
    want = ref.solve(atoms, basis, o)
    S = energy.System(atoms, basis, o)
    try:
        S.energy()
        obs = S.observables
        mu, E0, F = S.dipoles()
        assert obs["polar_iterations"] == want["polar_iterations"] and obs["iterator_failed"] == want["iterator_failed"] == 0
        dev = abs(obs["polarization_energy"] - want["polarization_energy"]) / abs(want["polarization_energy"])
        lines = [f"energy {dev:.1e}"]
        assert dev <= REF_REL_E, (case, obs["polarization_energy"], want["polarization_energy"])
        for k, got in (("ef_static", E0), ("mu", mu), ("ef_induced", F)):
            bad, ratio, _ = util.field_errors(got, want[k], REF_REL_MU, 1e-12)
            lines.append(f"{k} {ratio:.1e} of its bound")
            assert bad.size == 0, (case, k, ratio)
        rr = want["dipole_rrms"]
        if rr:
            eps_mu = util.max_rel(np.asarray(mu).reshape(-1), want["mu"].reshape(-1))
            assert abs(obs["dipole_rrms"] - rr) <= min(REL + 4.0 * eps_mu / rr, 1e-6) * rr, (case, obs["dipole_rrms"], rr)
        else:
            assert obs["dipole_rrms"] == 0.0
        if "polar_palmo" in o:
            assert abs(S.palmo_info()[0] - want["correction"]) <= REL * abs(want["polarization_energy"]) and want["correction"] != 0.0
        against_rank_pass(S, atoms, basis, want["ranked_sweeps"], case)
        print(f"\n{case}: iterations {obs['polar_iterations']} " + " ".join(lines))
    finally:
        S.close()


def tiny(pos, alpha):
    n = len(alpha)
    return {"pos": np.asarray(pos, dtype=np.float64).reshape(n, 3), "charge": np.asarray([(-1.0) ** i * 30.0 for i in range(n)]),
            "polarizability": np.asarray(alpha, dtype=np.float64), "epsilon": np.full(n, 10.0), "sigma": np.full(n, 3.0),
            "mol_id": np.arange(n, dtype=np.int32), "frozen": np.zeros(n, dtype=np.int32), "mass": np.full(n, 12.0)}


HAND = {"threshold_tie": ([[0, 0, 0], [2, 0, 0], [5, 0, 0]], [1.5, 1.5, 1.5], 2.0, [1, 2, 1], [1, 0, 2]),  # the pair at exactly 3.0 counts: <=
        "no_polarizable_pair": ([[0, 0, 0], [2, 0, 0], [5, 0, 0]], [1.5, 0.0, 0.0], ref.MAXVALUE, [0, 0, 0], [0, 1, 2]),
        "one_atom": ([[1, 2, 3]], [1.5], ref.MAXVALUE, [0], [0])}


@pytest.mark.parametrize("case", sorted(HAND))
def test_hand_made_cases(boxes, case):
    pos, alpha, rmin, rank, order = HAND[case]
    atoms, basis = tiny(pos, alpha), np.diag([100.0, 100.0, 100.0])
    o = dict(boxes["ion216_polar_gr_it4"][2], polar_max_iter=3)
    S = energy.System(atoms, basis, o)
    try:
        S.energy()
        info = against_rank_pass(S, atoms, basis, 2, case)
        got_rank, got_order = S.polar_gs_ranked()
        assert info["rmin"] == rmin and got_rank.tolist() == rank and got_order.tolist() == order, (case, info, got_rank, got_order)
        if order == sorted(order):  # the identity: what polar_gs computes, to the bit
            assert same_bits(snapshot(S), evaluated(atoms, basis, plain_gs(o)))
        if len(alpha) > 1:  # (a lone atom feels the rounding residue of its own Ewald images, 1e-19 of a field: nothing to compare but the bits above)
            want = ref.solve(atoms, basis, o)
            assert abs(S.observables["polarization_energy"] - want["polarization_energy"]) <= REF_REL_E * abs(want["polarization_energy"])
            assert util.field_errors(S.dipoles()[0], want["mu"], REF_REL_MU, 1e-12)[0].size == 0
    finally:
        S.close()


def fcc_cluster():
    """a 5 x 5 x 5 block of an fcc lattice, nearest neighbours 2.0 apart: twelve of them and the six at 2 sqrt 2 <= 3.0 give the inner
    atoms rank 18, the faces, edges and corners less -- many distinct keys, many ties"""
    a = 2.0 * np.sqrt(2.0)
    cell = np.array([[0, 0, 0], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]])
    pts = np.array([(np.array([i, j, k]) + c) * a for i in range(5) for j in range(5) for k in range(5) for c in cell])
    return pts + 20.0


def test_dense_cluster_and_the_sort_on_large_keys():
    """The rank pass on a dense cluster (500 atoms, 8 tiles, ranks 3 .. 18), then the device's sort on keys the rank pass cannot produce
    (atoms no closer than rmin leave room for about 60 within 1.5 rmin of one of them): any values below n, above 64 too."""
    pos = fcc_cluster()
    n = pos.shape[0]
    atoms, basis = tiny(pos, np.full(n, 1.2)), np.diag([60.0, 60.0, 60.0])
    o = {"polarization": 1, "polar_iterative": 1, "polar_ewald": 1, "polar_max_iter": 2, "polar_damp": 2.1304, "damp_type": "exponential", "ewald_kmax": 7,
         "polar_gs_ranked": 1}
    S = energy.System(atoms, basis, o)
    try:
        S.energy()
        info = against_rank_pass(S, atoms, basis, 1, "fcc")
        assert info["max_rank"] == 18 and len(set(S.polar_gs_ranked()[0].tolist())) >= 5, info
        L = energy.lib()
        rng = np.random.default_rng(5)
        for keys in (rng.integers(0, n, size=n), rng.integers(60, 70, size=n), np.arange(n), np.arange(n)[::-1].copy(), np.zeros(n), np.full(n, n - 1),
                     np.where(np.arange(n) % 7 == 0, n - 1, 0)):
            keys = np.ascontiguousarray(keys, dtype=np.int32)
            got = np.zeros(n, dtype=np.int32)
            S._check(L.mpmc_debug_gs_rank_order(S.handle, energy._ip(keys), energy._ip(got)))
            assert np.array_equal(got, np.argsort(-keys.astype(np.int64), kind="stable")), keys[:8]
        with pytest.raises(energy.MpmcError) as e:  # the sort overwrote what the rank pass left
            S.polar_gs_ranked()
        assert e.value.code == ERR_ARG
    finally:
        S.close()


def test_trial_moves_evaluate_in_full(boxes):
    """three accepted and three rejected moves, each against a fresh context at 1e-11"""
    atoms, basis, o = boxes["ion216_polar_gr_it4"]
    S = energy.System(atoms, basis, o)
    try:
        S.energy()
        pos = atoms["pos"].copy()
        for step, (a, accept) in enumerate(((17, True), (130, False), (5, True), (64, False), (215, True), (99, False))):
            trial = util.moved(util.with_positions(atoms, pos), a, 1, seed=31 + step)
            S.trial_energy(a, trial)
            assert S.last_trial_was_full(), step
            full = pos.copy()
            full[a:a + 1] = trial
            util.check_trial_against_fresh(S, atoms, basis, o, full, rel=1e-11, label=f"ranked step {step}")
            S.accept() if accept else S.reject()
            pos = full if accept else pos
        S.energy()
        assert not util.component_errors(S.observables, evaluated(util.with_positions(atoms, pos), basis, o)[0], util.TRIAL_KEYS, 1e-11)
        against_rank_pass(S, util.with_positions(atoms, pos), basis, 3, "after the trials")
    finally:
        S.close()


def test_setter_on_off_on_and_its_lifetime(boxes):
    """set by hand on a plain context; off restores the context that never called it to the bit; the setting survives mpmc_set_options,
    mpmc_set_box, mpmc_set_atoms and capacity growth"""
    atoms, basis, o = boxes["ion216_polar_gr_it4"]
    plain = {k: v for k, v in o.items() if k != "polar_gs_ranked"}
    L = energy.lib()
    never = evaluated(atoms, basis, plain)
    S = energy.System(atoms, basis, plain)
    try:
        S.set_polar_gs_ranked(True)
        S.energy()
        against_golden(S, atoms, o, "ion216_polar_gr_it4", label="set by hand")
        first = snapshot(S)
        S.set_polar_gs_ranked(False)
        with pytest.raises(energy.MpmcError) as e:
            S.polar_gs_ranked()
        assert e.value.code == ERR_ARG
        S.energy()
        assert same_bits(snapshot(S), never) and S.polar_gs_ranked_info()["acted"] == 0 and S.polar_gs_ranked_info()["enabled"] == 0
        S.set_polar_gs_ranked(True)
        with pytest.raises(energy.MpmcError) as e:  # no evaluation since the setting changed
            S.polar_gs_ranked()
        assert e.value.code == ERR_ARG
        S.energy()
        assert same_bits(snapshot(S), first)
        S._check(L.mpmc_set_options(S.handle, energy.C.byref(energy.make_options(dict(plain, polar_max_iter=2)))))
        S.energy()
        against_golden(S, atoms, o, "ion216_polar_gr_it2", label="after set_options")
        tri, tbasis, to = boxes["ion216_triclinic_gr_it4"]
        S._check(L.mpmc_set_options(S.handle, energy.C.byref(energy.make_options(to))))
        S.set_box(tbasis)
        S.set_atoms(tri)
        S.energy()
        against_golden(S, tri, to, "ion216_triclinic_gr_it4", label="after set_box and set_atoms")
        big, bbasis, bo = boxes["ion1000_gs_gr_it4"]  # more atoms than the context was made for
        S._check(L.mpmc_set_options(S.handle, energy.C.byref(energy.make_options(bo))))
        S.set_box(bbasis)
        S.set_atoms(big)
        S.energy()
        against_golden(S, big, bo, "ion1000_gs_gr_it4", label="after growth")
        against_rank_pass(S, big, bbasis, 3, "after growth")
    finally:
        S.close()


def test_refusals(boxes):
    atoms, basis, o = boxes["ion216_polar_gr_it4"]
    with pytest.raises(energy.MpmcError) as e:  # the keyword's flag bit stays refused: the setter alone switches the behaviour on
        energy.System(atoms, basis, dict(o, unsupported_flags=FLAG_POLAR_GS_RANKED))
    assert e.value.code == ERR_UNSUPPORTED
    S = energy.System(atoms, basis, o)
    try:
        S.set_options(dict(o, polar_gs=1))  # both sweep orders
        with pytest.raises(energy.MpmcError) as e:
            S.energy()
        assert e.value.code == ERR_INVALID_SETTING
        S.set_options(o)
        S.energy_async()
        with pytest.raises(energy.MpmcError) as e:
            S.set_polar_gs_ranked(False)
        assert e.value.code == ERR_ARG
        S.energy_wait()
        S.trial_energy(0, atoms["pos"][0:1] + 0.1)
        with pytest.raises(energy.MpmcError) as e:
            S.set_polar_gs_ranked(False)
        assert e.value.code == ERR_ARG
        S.reject()
        S.energy()
        against_golden(S, atoms, o, "ion216_polar_gr_it4", label="after the refusals")
    finally:
        S.close()


@pytest.mark.parametrize("case", ["direct", "zodid", "ewald_full", "polarization_off"])
def test_no_effect_where_the_reference_has_none(boxes, case):
    atoms, basis, o = boxes["ion216_polar_gr_it4"]
    extra = {"direct": {"polar_iterative": 0}, "zodid": {"polar_zodid": 1}, "ewald_full": {"polar_ewald_full": 1}, "polarization_off": {"polarization": 0}}[case]
    on, off = dict(o, **extra), dict(o, polar_gs_ranked=0, **extra)
    S = energy.System(atoms, basis, on)
    try:
        S.energy()
        info = S.polar_gs_ranked_info()
        assert info["enabled"] == 1 and info["acted"] == 0 and info["ranked_sweeps"] == 0, info
        with pytest.raises(energy.MpmcError) as e:
            S.polar_gs_ranked()
        assert e.value.code == ERR_ARG
        if case == "polarization_off":  # (no dipoles to compare)
            T = energy.System(atoms, basis, off)
            try:
                T.energy()
                assert S.observables == T.observables
            finally:
                T.close()
        else:
            assert same_bits(snapshot(S), evaluated(atoms, basis, off))
    finally:
        S.close()


def test_eight_in_flight_give_the_bits_of_one_at_a_time(boxes):
    atoms, basis, o = boxes["ion216_polar_gr_it4"]
    one = evaluated(atoms, basis, o)
    many = [energy.System(atoms, basis, o) for _ in range(8)]
    try:
        for S in many:
            S.energy_async()
        for S in many:
            S.energy_wait()
        for S in many:
            assert same_bits(snapshot(S), one)
            assert S.polar_gs_ranked_info()["ranked_sweeps"] == 3
    finally:
        for S in many:
            S.close()


@pytest.fixture(scope="module")
def pimc_nvt(tmp_path_factory):
    """examples/pimc_nvt: the PI-NVT driver over the C++ facade, as tests/test_pimc_driver.py builds it"""
    import os
    import subprocess

    from mpmcxx_amd import build as mbuild

    mbuild.build_library()
    libdir = os.path.dirname(mbuild.LIB)
    exe = str(tmp_path_factory.mktemp("pimc_gs_ranked") / "pimc_nvt")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-I", os.path.join(util.ROOT, "include"), os.path.join(util.ROOT, "examples", "pimc_nvt.cpp"),
                           "-L", libdir, "-lmpmc_energy", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_facade_and_pimc_driver_reproduce_pi_gs_ranked(pimc_nvt, tmp_path):
    """tests/golden/pi_gs_ranked (tools/make_pi_gs_ranked_golden.sh: the stock binary on pi_gs with polar_gs_ranked in place of polar_gs): the
    reader takes the keyword, the facade hands it to mpmc_set_polar_gs_ranked, and the run reproduces the stock binary's rows with the
    tolerance of test_facade_and_pimc_driver_reproduce_pi_relax"""
    import json
    import os
    import subprocess

    from mpmcxx_amd import pqr

    import test_pimc_driver as tp

    out = subprocess.run([pimc_nvt, os.path.join(util.GOLDEN, "pi_gs_ranked", "input.in"), "-P", "4", "-o", str(tmp_path)], stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    r = json.loads(out.stdout.strip().splitlines()[-1])
    ours, gold = tp.rows(os.path.join(tmp_path, "gsranked.energy.dat")), tp.rows(os.path.join(util.GOLDEN, "pi_gs_ranked", "golden_energy.dat"))
    assert len(ours) == len(gold) == 11
    for a, b in zip(ours, gold):
        assert a[0] == b[0]
        for x, y in zip(a[1:], b[1:]):
            assert abs(float(x) - float(y)) <= 1e-9 * max(abs(float(y)), 1.0) + 1.1e-6, (a, b)  # 6 printed decimals
    ar, ar_d, ar_b = tp.golden_ar("pi_gs_ranked")
    assert f"{r['AR']:.5f}" == f"{ar:.5f}" and f"{r['AR_displace']:.5f}" == f"{ar_d:.5f}" and f"{r['AR_bead']:.5f}" == f"{ar_b:.5f}"
    for k in range(4):
        a = pqr.read_pqr(os.path.join(tmp_path, f"gsranked.final-{k:04d}.pqr"))["pos"]
        b = pqr.read_pqr(os.path.join(util.GOLDEN, "pi_gs_ranked", f"golden_final-{k:04d}.pqr"))["pos"]
        assert np.abs(a - b).max() <= 1.0e-6
