"""GPU (MI355X): `polar_ewald_full` (the dipole solve with an Ewald-summed induced field, csrc/kernels_ewald_full.hip).

Yardsticks: the EWALD_FULL_FIXTURES goldens (the reference's own object code) and the numpy restatement tests/polar_ewald_full_ref.py,
which sits within 4e-13 (energy) and 5e-12 (per-atom arrays, of the largest component) of those goldens (tests/test_polar_ewald_full.py).
Tolerances: 1e-9 relative on polarization_energy and energy, per-atom arrays within 1e-9 of the array's largest component, counts and pass
numbers exact; against the restatement 1e-9 plus its own margin.  Run with -s for the measured deviations.
"""
import os
import subprocess

import numpy as np
import pytest

import util
import polar_ewald_full_ref as ref
from mpmcxx_amd import energy, gen_box

pytestmark = pytest.mark.gpu

REL = util.REL_TOL                         # 1e-9
REF_REL_E, REF_REL_F = REL + 4e-13, REL + 5e-12  # ... plus the restatement's own distance from the reference (energy, per-atom arrays)
PLAIN = {"ion216_polar_pef": "ion216_polar", "water64_polar_pef": "water64_polar"}


@pytest.fixture(scope="module")
def boxes(tmp_path_factory):
    d = tmp_path_factory.mktemp("pef")
    return {name: util.load_generated(name, d) for name in gen_box.EWALD_FULL_FIXTURES}


@pytest.fixture(scope="module")
def restated(boxes):
    """the restatement of every box the tests below compare with it, solved once"""
    cache = {}

    def get(name, vector_weight=False):
        key = (name, vector_weight)
        if key not in cache:
            cache[key] = ref.solve(*boxes[name], vector_weight=vector_weight)
        return cache[key]

    return get


def snapshot(S):
    return dict(S.observables), [x.copy() for x in S.dipoles()], S.ewald_full_info()


def same_bits(a, b):
    return a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))


def against_golden(S, name, label=None):
    """one evaluated System against the golden `name`: the two energies, every other component, counts, per-atom arrays"""
    g = ref.golden(name)
    label = label or name
    r = S.observables
    for k_ours, k_gold in (("polarization_energy", "polar"), ("energy", "total")):
        assert util.close(r[k_ours], g[k_gold]), (label, k_ours, r[k_ours], g[k_gold])
    util.assert_energies(r, g, False, label=label)
    util.assert_counts(r, g, rd_only=False, label=label)
    assert r["polar_iterations"] == 0 and r["dipole_rrms"] == 0.0 and r["iterator_failed"] == 0, (label, r)
    mu, E, F = S.dipoles()
    sample = np.asarray(g["sample_atoms"])
    devs = {}
    for k, got in (("ef_static", E), ("mu", mu), ("ef_induced", F)):
        devs[k] = float(np.abs(got[sample] - g[k]).max() / np.abs(g[k]).max())
    print(f"\n{label}: polar rel {abs(r['polarization_energy'] - g['polar']) / abs(g['polar']):.2e} energy rel "
          f"{abs(r['energy'] - g['total']) / abs(g['total']):.2e} " + " ".join(f"{k} {v:.2e}" for k, v in devs.items()))
    assert max(devs.values()) <= REL, (label, devs)
    return g


@pytest.mark.parametrize("name", gen_box.EWALD_FULL_FIXTURES)
def test_golden(boxes, restated, name):
    atoms, basis, o = boxes[name]
    S = energy.System(atoms, basis, o)
    try:
        S.energy()
        against_golden(S, name)
        info = S.ewald_full_info()
        assert info["n_k"] == {7: 709, 5: 257}[o["ewald_kmax"]], info
        n = len(atoms["charge"])
        nt = -(-n // 64)
        assert info["store_bytes"] == nt * (nt + 1) // 2 * 64 * 64 * 16, info
        if not o.get("polar_precision"):
            assert info["passes"] == o["polar_max_iter"] + 1, info
        if n <= 1000:
            want = restated(name)
            assert info["n_real_pairs"] == want["n_real_pairs"], (info, want["n_real_pairs"])
            assert info["passes"] == want["passes"], (info, want["passes"])
        a = snapshot(S)
        S.energy()
        assert same_bits(a, snapshot(S)) and a[2] == S.ewald_full_info(), "a repeated evaluation must give the same bits"
    finally:
        S.close()


@pytest.mark.parametrize("name", ["ion216_polar_pef", "water64_polar_pef", "ion216_triclinic_pef"])
def test_vector_kweight_against_the_restatement(boxes, restated, name):
    atoms, basis, o = boxes[name]
    S = energy.System(atoms, basis, dict(o, polar_ewald_full_flags=energy.PEF_VECTOR_KWEIGHT))
    try:
        S.energy()
        want, scalar = restated(name, True), ref.golden(name)["polar"]
        got = S.observables["polarization_energy"]
        assert abs(got - want["polarization_energy"]) <= REF_REL_E * abs(want["polarization_energy"]), (name, got, want["polarization_energy"])
        assert abs(got - scalar) > 1e-3 * abs(scalar), (name, got, scalar)
        for k, x in zip(("mu", "ef_static", "ef_induced"), S.dipoles()):
            assert np.abs(x - want[k]).max() <= REF_REL_F * np.abs(want[k]).max(), (name, k)
        assert S.observables["polar_iterations"] == 0 and S.ewald_full_info()["passes"] == want["passes"]
        print(f"\n{name}: vector weight {got!r} K, the reference's scalar weight {scalar!r} K")
    finally:
        S.close()


def test_switches_that_change_nothing_under_the_term(boxes):
    atoms, basis, o = boxes["ion216_polar_pef"]
    S = energy.System(atoms, basis, o)
    try:
        S.energy()
        base = snapshot(S)
        variants = [{"polar_ewald": 0}, {"polar_iterative": 0}, {"polar_gs": 1}, {"polar_gamma": 1.03}, {"polar_rrms": 1}, {"polar_wolf": 1, "polar_wolf_alpha": 0.13}]
        variants += [{"solver": s} for s in ("auto", "matrix_free", "compact", "dense")]
        for extra in variants:
            T = energy.System(atoms, basis, dict(o, **extra))
            try:
                T.energy()
                assert same_bits(base, snapshot(T)), extra
            finally:
                T.close()
            S.set_options(dict(o, **extra))  # ... and on one live context, switched there and back
            S.energy()
            assert same_bits(base, snapshot(S)), ("live", extra)
            S.set_options(o)
            if "polar_wolf" in extra:
                S.set_polar_wolf(False)
    finally:
        S.close()


@pytest.mark.parametrize("name", ["ion216_polar_pef", "water64_polar_pef"])
def test_on_then_off_is_a_fresh_context(boxes, name):
    atoms, basis, _ = boxes[name]
    _, _, plain = util.load_fixture(PLAIN[name])
    S, P = energy.System(atoms, basis, plain), energy.System(atoms, basis, plain)
    try:
        P.energy()
        want = dict(P.observables), [x.copy() for x in P.dipoles()]
        S.set_polar_ewald_full(True)
        S.energy()
        assert S.observables["polarization_energy"] != want[0]["polarization_energy"]
        assert util.close(S.observables["polarization_energy"], ref.golden(name)["polar"])
        S.set_polar_ewald_full(False)
        S.energy()
        assert S.observables == want[0] and all(np.array_equal(a, b) for a, b in zip(S.dipoles(), want[1]))
    finally:
        S.close(), P.close()


def test_the_setting_survives_and_follows_growth(boxes):
    atoms, basis, o = boxes["ion216_polar_pef"]
    plain = {k: v for k, v in o.items() if k != "polar_ewald_full"}
    L = energy.lib()
    S = energy.System(atoms, basis, plain)
    try:
        S.set_polar_ewald_full(True)
        S.energy()
        first = snapshot(S)
        against_golden(S, "ion216_polar_pef", label="set by hand")
        S._check(L.mpmc_set_options(S.handle, energy.C.byref(energy.make_options(dict(plain, polar_max_iter=3)))))
        S.energy()
        against_golden(S, "ion216_polar_pef_it3", label="after set_options")
        S._check(L.mpmc_set_options(S.handle, energy.C.byref(energy.make_options(plain))))
        S.set_atoms(atoms)
        S.energy()
        assert same_bits(first, snapshot(S)), "after set_atoms"
        tri, tbasis, _ = boxes["ion216_triclinic_pef"]
        S.set_box(tbasis)
        S.energy()
        against_golden(S, "ion216_triclinic_pef", label="after set_box")
        big, bbasis, bo = boxes["ion1000_polar_pef"]  # more atoms than the context was made for
        S.set_box(bbasis)
        S.set_atoms(big)
        S.energy()
        against_golden(S, "ion1000_polar_pef", label="after growth")
        F = energy.System(big, bbasis, bo)
        try:
            F.energy()
            assert same_bits(snapshot(F), snapshot(S)) and F.ewald_full_info() == S.ewald_full_info(), "a grown context against a fresh one"
        finally:
            F.close()
    finally:
        S.close()


@pytest.mark.parametrize("off", [{"rd_only": 1}, {"polarization": 0}])
def test_nothing_changes_without_polarization(boxes, off):
    atoms, basis, o = boxes["water64_polar_pef"]
    plain = {k: v for k, v in o.items() if k != "polar_ewald_full"}
    S, P = energy.System(atoms, basis, dict(o, **off)), energy.System(atoms, basis, dict(plain, **off))
    try:
        S.energy(), P.energy()
        assert S.observables == P.observables, off
        assert S.observables["polarization_energy"] == 0.0
        assert S.ewald_full_info()["passes"] == 0
    finally:
        S.close(), P.close()


def test_entry_points_follow_the_term(boxes):
    """mpmc_energy_async / mpmc_energy_wait, the bead loop, dipoles on demand, mpmc_polar, mpmc_thole_field and the timing slots"""
    atoms, basis, o = boxes["water64_polar_pef"]
    g = ref.golden("water64_polar_pef")
    S = energy.System(atoms, basis, o)
    beads, singles = [], []
    try:
        S.energy()
        base = snapshot(S)
        S.energy_async()
        S.energy_wait()
        assert same_bits(base, snapshot(S)), "async / wait"
        S.set_dipoles_on_demand(True)
        S.energy()
        assert same_bits(base, snapshot(S)), "dipoles on demand"
        S.set_dipoles_on_demand(False)
        S.configure("pef_phase_table", 0)  # (the measurement switch: the phases recomputed in every pass are the table's)
        S.energy()
        assert same_bits(base, snapshot(S)), "without the phase table"
        S.configure("pef_phase_table", 1)
        assert util.close(S.polar(), g["polar"])
        assert np.abs(S.thole_field() - g["ef_static"]).max() <= REL * np.abs(g["ef_static"]).max()
        S.set_profiling(True)
        S.timings(reset=True)
        S.energy()
        t = S.timings()
        assert t["tensor"]["launches"] == 1 and t["dipole_iter"]["launches"] == 11 and t["reduce"]["launches"] >= 11, t
        S.set_profiling(False)
        for b in range(2):
            p = gen_box.bead_positions(atoms["pos"], b)
            beads.append(energy.System(util.with_positions(atoms, p), basis, o))
            singles.append(energy.System(util.with_positions(atoms, p), basis, o))
        sums, per, failed = energy.pi_potential_local(beads)
        assert not failed
        for k, s in enumerate(singles):
            s.energy()
            assert per[k] == s.observables, k
            assert all(np.array_equal(a, b) for a, b in zip(beads[k].dipoles(), s.dipoles())), k
            assert beads[k].ewald_full_info()["passes"] == 11
    finally:
        for s in [S] + beads + singles:
            s.close()


@pytest.mark.parametrize("name", ["water64_polar_pef", "ion1000_polar_pef"])
def test_trial_move(boxes, name):
    """a one-molecule trial runs a full evaluation of the trial configuration: the bits of a fresh context's full evaluation of the moved
    box; reject restores the accepted totals; accept, then mpmc_energy, re-bases to the same bits.
    The fresh context receives the moved molecule through update_positions behind a first evaluation, as the trial does: its atoms then
    sit in the same tiles.  A
    context that is CREATED on the moved box sorts its atoms anew, and in the molecular box a neighbour swap inside one tile changes the
    order of every sum -- measured there: lj_pairs, which this term does not touch, moves by one ulp (rel 1.3e-16) and the polarization
    energy with it (1.3e-16); that context is held to 1e-11 (util.check_trial_against_fresh), the rule of the other trial tests."""
    atoms, basis, o = boxes[name]
    S = energy.System(atoms, basis, o)
    try:
        S.energy()
        accepted = dict(S.observables)
        first, end = util.molecules(atoms)[7]
        new = util.moved(atoms, first, end - first, 41, sigma=0.05)
        trial = atoms["pos"].copy()
        trial[first:end] = new
        F = energy.System(atoms, basis, o)
        try:
            F.energy()  # (the spatial order is made with the first upload: from the accepted box, as S's was)
            F.update_positions(first, new)
            F.energy()
            fresh = dict(F.observables)
        finally:
            F.close()
        for accept in (False, True):
            S.trial_energy(first, new)
            assert S.last_trial_was_full(), name
            assert S.trial_observables == fresh, (name, util.component_errors(S.trial_observables, fresh, util.TRIAL_KEYS, 0.0))
            util.check_trial_against_fresh(S, atoms, basis, o, trial, rel=1e-11, label=name)
            if accept:
                S.accept()
                S.energy()
                assert S.observables == fresh, "accept, then a full evaluation"
            else:
                S.reject()
                S.energy()
                assert S.observables == accepted, "reject restores the accepted configuration"
    finally:
        S.close()


def test_refusals(boxes, tmp_path):
    atoms, basis, o = boxes["ion216_polar_pef"]
    L = energy.lib()
    S = energy.System(atoms, basis, o)
    try:
        S.energy()
        base = snapshot(S)
        for flags in (2, 4, 3, -1):
            assert L.mpmc_set_polar_ewald_full(S.handle, 1, flags) == 4000, flags
        S.energy()
        assert same_bits(base, snapshot(S)), "a refused setting leaves the context alone"
        S.set_polar_palmo(True)
        with pytest.raises(energy.MpmcError) as e:
            S.energy()
        assert e.value.code == 4004 and "ewald_palmo_contraction" in str(e.value), e.value
        S.set_polar_palmo(False)
        S.energy()
        assert same_bits(base, snapshot(S)), "after the refused evaluation"
        with pytest.raises(energy.MpmcError) as e:
            energy.System(atoms, basis, dict(o, unsupported_flags=1 << 7))
        assert e.value.code == 4004
    finally:
        S.close()
    import test_polar_ewald_full as cpu

    exe = cpu.build_check_program(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.split("\n")[:2] == ["pimc 4004", "gibbs 4004"], out.stdout + out.stderr
