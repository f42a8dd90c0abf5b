"""GPU (MI355X): `polar_sor`, `polar_esor` and `polar_zodid` (mpmc_set_polar_relax: the relaxed instantiations of the dipole update
kernels, k_gs_blend behind the Gauss-Seidel sweeps, the relaxed finish of polar_ewald_full, the zeroth-order shortcut).

Yardsticks: the RELAX_FIXTURES goldens (the reference's own object code) with util.assert_matches_oracle's bounds -- 1e-9 relative per
energy component with no floor, iterations and iterator_failed equal, the per-atom fields as that function states -- and the numpy
restatement tests/polar_relax_ref.py, which sits within 8e-14 (energy) and 7e-13 (per-atom arrays) of those goldens
(tests/test_polar_relax.py).  Run with -s for the measured deviations.
"""
import numpy as np
import pytest

import util
import polar_relax_ref as ref
from mpmcxx_amd import energy, gen_box

pytestmark = pytest.mark.gpu

REL = util.REL_TOL           # 1e-9
REF_REL_E = REL + 8e-13      # ... plus ten times the restatement's own distance from the reference (energy; test_polar_relax.WORST)
FLAG_POLAR_SOR, FLAG_POLAR_ZODID = 1 << 11, 1 << 12
ERR_INVALID_SETTING, ERR_INCOMPATIBLE, ERR_UNSUPPORTED, ERR_ARG = 4000, 4002, 4004, -3


@pytest.fixture(scope="module")
def boxes(tmp_path_factory):
    d = tmp_path_factory.mktemp("relax")
    return {name: util.load_generated(name, d) for name in gen_box.RELAX_FIXTURES}


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


def snapshot(S):
    return dict(S.observables), [x.copy() for x in S.dipoles()]


def same_bits(a, b):
    return a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))


@pytest.mark.parametrize("name", gen_box.RELAX_FIXTURES)
def test_golden(boxes, name):
    atoms, basis, o = boxes[name]
    S = energy.System(atoms, basis, o)
    try:
        S.energy()
        against_golden(S, atoms, o, name)
        info = S.polar_relax_info()
        variant = name.rsplit("_rx_", 1)[1]
        assert info["scheme"] == energy.polar_relax_of(o)[0] and info["zodid"] == int(bool(o.get("polar_zodid"))), info
        g = ref.golden(name)
        if variant.startswith("zodid"):  # no A matrix, no iteration, nothing stored
            assert info["acted"] == 1 and info["contractions"] == 0 and info["store_filled"] == 0 and info["last_weight"] == 1.0, info
            assert S.observables["polar_iterations"] == 0 and S.observables["dipole_rrms"] == 0.0 and not np.any(S.dipoles()[2])
        elif variant.startswith("pef"):
            passes = S.ewald_full_info()["passes"]
            assert info["contractions"] == passes and info["store_filled"] == 1, info
            assert info["acted"] == (0 if variant == "pefzodid" else 1), info
            if variant != "pefzodid":
                assert info["last_weight"] == ref.weights(o, passes)[0], info
        else:
            it = g["polar_iterations"]
            ran = it - g["iterator_failed"]  # (a failed solve stops in front of its 128th contraction)
            assert info["acted"] == 1 and info["contractions"] == ran + (1 if o.get("polar_palmo") and o.get("polar_gs") else 0), info
            assert info["last_weight"] == ref.weights(o, ran)[0], info
        a = snapshot(S)
        S.energy()
        assert same_bits(a, snapshot(S)), "a repeated evaluation must give the same bits"
    finally:
        S.close()


@pytest.mark.parametrize("solver", ["matrix_free", "compact", "dense"])
@pytest.mark.parametrize("name", ["ion216_polar_rx_sor08", "ion216_polar_rx_esor06", "ion216_polar_rx_sorp"])
def test_every_solver(boxes, name, solver):
    """216 atoms: four tiles with a padded last one -- the panel table and both update kernels are reached (compact: the panel update;
    matrix-free and dense: the slot update); sorp batches its precision-terminated launches, each with its own weight"""
    atoms, basis, o = boxes[name]
    S = energy.System(atoms, basis, dict(o, solver=solver))
    try:
        S.energy()
        against_golden(S, atoms, o, name, label=f"{name}/{solver}")
        assert S.polar_relax_info()["store_filled"] == (0 if solver == "matrix_free" else 1)
    finally:
        S.close()


@pytest.mark.parametrize("name", ["ion216_polar", "ion1000_gs"])
def test_none_is_the_context_that_never_called(name):
    atoms, basis, o = util.load_fixture(name)
    A, B = energy.System(atoms, basis, o), energy.System(atoms, basis, o)
    try:
        B.set_polar_relax("none", False)
        A.energy(), B.energy()
        assert same_bits(snapshot(A), snapshot(B))
        B.set_polar_relax("sor", True)  # ... and on, then off again
        B.energy()
        assert B.observables["polar_iterations"] == 0
        B.set_polar_relax(0, False)
        B.energy()
        assert same_bits(snapshot(A), snapshot(B))
        info = B.polar_relax_info()
        assert info["scheme"] == 0 and info["zodid"] == 0 and info["acted"] == 0 and info["last_weight"] == 1.0, info
    finally:
        A.close(), B.close()


@pytest.mark.parametrize("gs", [0, 1])
def test_sor_with_gamma_one_is_the_plain_solve(gs):
    """w = (1, 0): the blend 1 new + 0 old is new to the bit, so the dipoles are the plain solve's.  The plain Jacobi solve takes its
    energy from the moments of the dipole differences, the relaxed one from -1/2 sum mu . E0: two roundings of one number, 648 terms of
    relative weight <= 1 each against a sum of the same sign -- bound 648 * 2^-53 * 10 < 1e-12."""
    atoms, basis, o = util.load_fixture("ion216_polar")
    o = dict(o, polar_gs=gs, polar_max_iter=6)
    A, B = energy.System(atoms, basis, o), energy.System(atoms, basis, dict(o, polar_sor=1, polar_gamma=1.0))
    try:
        A.energy(), B.energy()
        assert B.polar_relax_info()["acted"] == 1
        for x, y in zip(A.dipoles(), B.dipoles()):
            assert np.array_equal(x, y)
        a, b = A.observables["polarization_energy"], B.observables["polarization_energy"]
        print(f"\ngs {gs}: plain {a!r} sor(1.0) {b!r} rel {abs(a - b) / abs(a):.1e}")
        assert abs(a - b) <= 1e-12 * abs(a)
        assert A.observables["polar_iterations"] == B.observables["polar_iterations"] == 6
    finally:
        A.close(), B.close()


@pytest.mark.parametrize("name", ["water64_polar_rx_zodid", "ion216_polar_rx_zodid"])
def test_zodid_trial_moves(boxes, name):
    """three trial moves, the second rejected: O(m N) end to end (never a full evaluation, no contraction, no store), against a fresh
    context at 1e-11 and against the restatement at 1e-9 (+ its own margin)"""
    atoms, basis, o = boxes[name]
    S = energy.System(atoms, basis, o)
    try:
        S.energy()
        pos = atoms["pos"].copy()
        mols = util.molecules(atoms)
        for step, (m, accept) in enumerate(((3, True), (11, False), (len(mols) - 1, True))):
            a, b = mols[m]
            trial = util.moved(util.with_positions(atoms, pos), a, b - a, seed=100 + step)
            S.trial_energy(a, trial)
            assert not S.last_trial_was_full(), (name, step)
            info = S.polar_relax_info()
            assert info["contractions"] == 0 and info["store_filled"] == 0 and info["acted"] == 1, info
            full = pos.copy()
            full[a:b] = trial
            util.check_trial_against_fresh(S, atoms, basis, o, full, rel=1e-11, label=f"{name} step {step}")
            want = ref.solve(util.with_positions(atoms, full), basis, o)["polarization_energy"]
            got = S.trial_observables["polarization_energy"]
            assert abs(got - want) <= REF_REL_E * abs(want), (name, step, got, want)
            if accept:
                S.accept()
                pos = full
            else:
                S.reject()
        S.energy()  # the accepted configuration, evaluated in full, is what the trials left
        T = energy.System(util.with_positions(atoms, pos), basis, o)
        try:
            T.energy()
            assert not util.component_errors(S.observables, T.observables, util.TRIAL_KEYS, 1e-11)
        finally:
            T.close()
    finally:
        S.close()


def test_sor_trial_moves(boxes):
    atoms, basis, o = boxes["ion216_polar_rx_sor08"]
    S = energy.System(atoms, basis, o)
    try:
        S.energy()
        pos = atoms["pos"].copy()
        for step, (a, accept) in enumerate(((17, True), (130, False))):
            trial = util.moved(util.with_positions(atoms, pos), a, 1, seed=7 + step)
            S.trial_energy(a, trial)
            assert not S.last_trial_was_full(), step
            full = pos.copy()
            full[a:a + 1] = trial
            util.check_trial_against_fresh(S, atoms, basis, o, full, rel=1e-11, label=f"sor step {step}")
            want = ref.solve(util.with_positions(atoms, full), basis, o)["polarization_energy"]
            assert abs(S.trial_observables["polarization_energy"] - want) <= REF_REL_E * abs(want), step
            S.accept() if accept else S.reject()
            pos = full if accept else pos
        S.energy()
        T = energy.System(util.with_positions(atoms, pos), basis, o)
        try:
            T.energy()
            assert not util.component_errors(S.observables, T.observables, util.TRIAL_KEYS, 1e-11)
        finally:
            T.close()
    finally:
        S.close()


def test_the_setting_survives(boxes):
    """set by hand on a plain context; across mpmc_set_options, mpmc_set_box, mpmc_set_atoms and capacity growth"""
    atoms, basis, o = boxes["ion216_polar_rx_esor06"]
    plain = {k: v for k, v in o.items() if k != "polar_esor"}
    L = energy.lib()
    S = energy.System(atoms, basis, plain)
    try:
        S.set_polar_relax("esor")
        S.energy()
        against_golden(S, atoms, o, "ion216_polar_rx_esor06", label="set by hand")
        S._check(L.mpmc_set_options(S.handle, energy.C.byref(energy.make_options(dict(plain, polar_gamma=0.8)))))
        S.set_polar_relax("sor")
        S.energy()
        against_golden(S, atoms, o, "ion216_polar_rx_sor08", label="after set_options")
        tri, tbasis, to = boxes["ion216_triclinic_rx_sor08"]
        S.set_box(tbasis)
        S.set_atoms(tri)
        S.energy()
        against_golden(S, tri, to, "ion216_triclinic_rx_sor08", label="after set_box and set_atoms")
        big, bbasis, bo = boxes["ion1000_gs_rx_gsesor4"]  # more atoms than the context was made for
        S._check(L.mpmc_set_options(S.handle, energy.C.byref(energy.make_options(bo))))
        S.set_polar_relax("esor")
        S.set_box(bbasis)
        S.set_atoms(big)
        S.energy()
        against_golden(S, big, bo, "ion1000_gs_rx_gsesor4", label="after growth")
    finally:
        S.close()


def test_refusals(boxes):
    atoms, basis, o = boxes["ion216_polar_rx_sor08"]
    for bit in (FLAG_POLAR_SOR, FLAG_POLAR_ZODID):  # the keywords' flag bits stay refused: the setter alone switches the behaviour on
        with pytest.raises(energy.MpmcError) as e:
            energy.System(atoms, basis, dict(o, unsupported_flags=bit))
        assert e.value.code == ERR_UNSUPPORTED
    S = energy.System(atoms, basis, o)
    try:
        with pytest.raises(energy.MpmcError) as e:
            S.set_polar_relax(3)
        assert e.value.code == ERR_INVALID_SETTING
        S.set_options(dict(o, polar_gamma=-0.1))
        with pytest.raises(energy.MpmcError) as e:
            S.energy()
        assert e.value.code == ERR_INVALID_SETTING
        S.set_options(dict(o, polar_sor=0, polar_zodid=1, polar_iterative=0))  # zodid with the direct solve
        with pytest.raises(energy.MpmcError) as e:
            S.energy()
        assert e.value.code == ERR_INCOMPATIBLE
        S.set_options(o)
        S.energy_async()
        with pytest.raises(energy.MpmcError) as e:
            S.set_polar_relax("esor")
        assert e.value.code == ERR_ARG
        S.energy_wait()
        S.trial_energy(0, atoms["pos"][0:1] + 0.1)
        with pytest.raises(energy.MpmcError) as e:
            S.set_polar_relax("esor")
        assert e.value.code == ERR_ARG
        S.reject()
        S.energy()
        against_golden(S, atoms, o, "ion216_polar_rx_sor08", label="after the refusals")
    finally:
        S.close()


@pytest.fixture(scope="module")
def pimc_nvt(tmp_path_factory):
    """examples/pimc_nvt: the PI-NVT driver over the C++ facade, as tests/test_pimc_driver.py builds it"""
    import os
    import subprocess

    from mpmcxx_amd import build as mbuild

    mbuild.build_library()
    libdir = os.path.dirname(mbuild.LIB)
    exe = str(tmp_path_factory.mktemp("pimc_relax") / "pimc_nvt")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-I", os.path.join(util.ROOT, "include"), os.path.join(util.ROOT, "examples", "pimc_nvt.cpp"),
                           "-L", libdir, "-lmpmc_energy", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


@pytest.mark.parametrize("trial", [False, True], ids=["full", "trial_moves"])
def test_facade_and_pimc_driver_reproduce_pi_relax(pimc_nvt, trial, tmp_path):
    """tests/golden/pi_relax (tools/make_pi_relax_golden.sh: the stock binary on pi_gs with polar_esor 0.7 in place of polar_gs): the reader
    takes the keywords, the facade hands them to mpmc_set_polar_relax, and the run reproduces the stock binary's rows as the other pi_*
    cases are compared (tests/test_pimc_driver.py).  The polarization column tells the schemes apart: pi_gs differs there by 2e-5 K."""
    import json
    import os
    import subprocess

    from mpmcxx_amd import pqr

    import test_pimc_driver as tp

    out = subprocess.run([pimc_nvt, os.path.join(util.GOLDEN, "pi_relax", "input.in"), "-P", "4", "-o", str(tmp_path)] + (["--trial"] if trial else []),
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    r = json.loads(out.stdout.strip().splitlines()[-1])
    ours, gold = tp.rows(os.path.join(tmp_path, "relax.energy.dat")), tp.rows(os.path.join(util.GOLDEN, "pi_relax", "golden_energy.dat"))
    assert len(ours) == len(gold) == 11
    for a, b in zip(ours, gold):
        assert a[0] == b[0]
        for x, y in zip(a[1:], b[1:]):
            assert abs(float(x) - float(y)) <= 1e-9 * max(abs(float(y)), 1.0) + 1.1e-6, (a, b)  # 6 printed decimals
    ar, ar_d, ar_b = tp.golden_ar("pi_relax")
    assert f"{r['AR']:.5f}" == f"{ar:.5f}" and f"{r['AR_displace']:.5f}" == f"{ar_d:.5f}" and f"{r['AR_bead']:.5f}" == f"{ar_b:.5f}"
    for k in range(4):
        a = pqr.read_pqr(os.path.join(tmp_path, f"relax.final-{k:04d}.pqr"))["pos"]
        b = pqr.read_pqr(os.path.join(util.GOLDEN, "pi_relax", f"golden_final-{k:04d}.pqr"))["pos"]
        assert np.abs(a - b).max() <= 1.0e-6
