"""GPU (MI355X): polarization energy from the moments of the first ceil(n/2) Jacobi iterations, dipoles on demand.

Boxes: the smallest that reach every branch -- ion216_polar, water64_polar (alpha = 0 sites, exclusions), ion1000_polar (panel table, its
update kernel), ion216_triclinic, ion216_polar under the dense solver; polar_max_iter 1, 2, 3, 10 (odd and even counts, rings of 2 and 6
vectors; under AUTO, n <= 3 runs matrix-free through k_dipole_update, n = 10 the tensor store and the panel update).
Energies against the oracle at the tolerance of test_gpu_parity (util.REL_TOL, no floor); on-demand against eager bit for bit.
Fall-back: the solves the moments do not cover must do what the parent commit did -- energies (bit patterns) and launch counts per
timing class recorded from the parent's library on the same kind of device, tests/golden/dipoles_on_demand_fallback_parent.json."""
import functools
import json
import os

import numpy as np
import pytest

import util
from mpmcxx_amd import energy

pytestmark = pytest.mark.gpu

CASES = [("ion216_polar", "auto"), ("water64_polar", "auto"), ("ion1000_polar", "auto"), ("ion216_triclinic", "auto"), ("ion216_polar", "dense")]
COUNTS = [1, 2, 3, 10]
ENERGY_BITS = ["energy", "rd_energy", "coulombic_energy", "polarization_energy", "es_real", "es_recip", "es_self", "lj_pairs"]

# the solves outside the moment identity: they run as in the parent commit.  `polar_palmo` is recorded where it acts, under
# Gauss-Seidel sweeps; under Jacobi iterations it changes nothing and such a context gives the bits of one without the option
# (test_gpu_polar_wolf.test_palmo_correction), moments included.
FALLBACK = {"gamma": {"polar_gamma": 1.03}, "precision": {"polar_precision": 1e-6, "polar_max_iter": 30}, "rrms": {"polar_rrms": 1},
            "gs": {"polar_gs": 1}, "palmo_gs": {"polar_palmo": 1, "polar_gs": 1}, "direct": {"polar_iterative": 0}}
FALLBACK_GOLDEN = os.path.join(util.GOLDEN, "dipoles_on_demand_fallback_parent.json")


@functools.lru_cache(maxsize=None)
def case(name, n):
    atoms, basis, opts = util.load_fixture(name)
    opts = dict(opts, polar_max_iter=n)
    return atoms, basis, opts, util.oracle_energy(atoms, basis, opts)


def half(n):
    return (n + 1) // 2


def fallback_record(label):
    """what one evaluation of ion216_polar under FALLBACK[label] gives: energies as bit patterns, iteration count, launches per class.

    The golden file holds this record for every label as the PARENT commit's library gives it on an MI355X.  To regenerate it (after a
    compiler or ROCm change that moves a last bit, or when FALLBACK changes): build the library of the commit before "Polarization energy
    from half the Jacobi contractions" (python -c "from mpmcxx_amd import build; build.build_library()" in a checkout of it) and run, in
    this tree on the GPU,
        MPMC_ENERGY_LIB=/path/to/that/libmpmc_energy.so python tests/test_gpu_dipoles_on_demand.py tests/golden/dipoles_on_demand_fallback_parent.json
    (the __main__ block below; energy.py loads the library the variable names instead of the tree's own)."""
    atoms, basis, opts = util.load_fixture("ion216_polar")
    S = energy.System(atoms, basis, dict(opts, **FALLBACK[label]))
    S.energy()  # (allocations, the position-independent terms: the recorded evaluation is a steady-state one)
    S.set_profiling(True)
    S.timings(reset=True)
    _, per, _ = energy.pi_potential_local([S])
    obs = dict(per[0])
    launches = {k: v["launches"] for k, v in S.timings(reset=True).items()}
    mu = S.dipoles()[0]
    after = {k: v["launches"] for k, v in S.timings(reset=True).items()}
    S.close()
    return {"energies": {k: float(obs[k]).hex() for k in ENERGY_BITS}, "dipole_rrms": float(obs["dipole_rrms"]).hex(),
            "polar_iterations": int(obs["polar_iterations"]), "iterator_failed": int(obs["iterator_failed"]), "launches": launches,
            "launches_behind_dipoles": after, "mu_abs_sum": float(np.abs(mu).sum()).hex()}


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("name,solver", CASES)
def test_moment_energy_and_dipoles_on_demand(name, solver, n):
    atoms, basis, opts, ref = case(name, n)
    opts = dict(opts, solver=solver)
    label = f"{name}/{solver}/n={n}"
    # eager: all n iterations, the energy from the moments of the first half
    E = energy.System(atoms, basis, opts)
    e_lone = E.energy()
    obs_e = dict(E.observables)
    dip_e = E.dipoles()
    util.assert_matches_oracle(obs_e, dip_e, ref, atoms, opts, label=label + " eager")
    # on demand: the bead loop stops after ceil(n/2) iterations
    L = energy.System(atoms, basis, opts)
    L.set_profiling(True)
    L.timings(reset=True)
    _, per, failed = energy.pi_potential_local([L])
    obs_l = dict(per[0])
    ran = L.timings(reset=True)
    assert not failed
    assert ran["dipole_iter"]["launches"] == half(n), (label, ran)
    for k in ENERGY_BITS:
        assert obs_l[k] == obs_e[k], (label, k, obs_l[k], obs_e[k])  # bit for bit: a bead is a lone evaluation
    assert obs_l["energy"] == e_lone
    assert obs_l["polar_iterations"] == n == obs_e["polar_iterations"]
    dip_l = L.dipoles()
    rest = L.timings(reset=True)
    assert rest["dipole_iter"]["launches"] == n - half(n), (label, rest)
    for got, want, what in zip(dip_l, dip_e, ("mu", "ef_static", "ef_induced")):
        assert np.array_equal(got, want), (label, what, float(np.abs(got - want).max()))
    again = L.dipoles()
    assert all(np.array_equal(a, b) for a, b in zip(again, dip_l))
    assert L.timings(reset=True)["dipole_iter"]["launches"] == 0  # nothing left to run
    util.assert_matches_oracle(obs_l, dip_l, ref, atoms, opts, label=label + " on demand")
    E.close()
    L.close()


@pytest.mark.parametrize("n", [3, 10])
def test_dropped_solve_is_an_error_not_stale_memory(n):
    atoms, basis, opts, _ = case("ion216_polar", n)
    S = energy.System(atoms, basis, opts)
    energy.pi_potential_local([S])
    S.update_positions(0, atoms["pos"][:3])  # (the same coordinates: it is the call that counts)
    with pytest.raises(energy.MpmcError) as ei:
        S.dipoles()
    assert "on demand" in str(ei.value)
    with pytest.raises(energy.MpmcError):
        S.dipoles()  # still refused
    _, per, _ = energy.pi_potential_local([S])
    mu = S.dipoles()[0]
    T = energy.System(atoms, basis, opts)
    T.energy()
    assert np.array_equal(mu, T.dipoles()[0])
    # an eager evaluation behind an open solve leaves complete dipoles as well
    energy.pi_potential_local([S])
    S.energy()
    assert np.array_equal(S.dipoles()[0], mu)
    # ... and a piece that does not solve them leaves none
    energy.pi_potential_local([S])
    S.lj()
    with pytest.raises(energy.MpmcError):
        S.dipoles()
    S.close()
    T.close()


def test_opt_in_and_debug_switch():
    atoms, basis, opts, _ = case("ion1000_polar", 10)
    S = energy.System(atoms, basis, opts)
    S.set_profiling(True)
    S.energy()
    S.timings(reset=True)
    e_eager = S.energy()
    assert S.timings(reset=True)["dipole_iter"]["launches"] == 10
    S.set_dipoles_on_demand(True)
    assert S.energy() == e_eager
    assert S.timings(reset=True)["dipole_iter"]["launches"] == 5
    assert S.time_kernel("panel", 2) > 0.0  # (finishes the open solve first)
    assert S.timings(reset=True)["dipole_iter"]["launches"] == 5
    mu = S.dipoles()[0]
    S.set_dipoles_on_demand(False)
    S.energy()
    assert np.array_equal(S.dipoles()[0], mu)
    S.configure("dipoles_on_demand", 0)  # the A/B key: the bead loop runs every iteration at once
    S.timings(reset=True)
    _, per, _ = energy.pi_potential_local([S])
    assert S.timings(reset=True)["dipole_iter"]["launches"] == 10 and per[0]["energy"] == e_eager
    S.close()


def test_trial_moves_stay_eager():
    atoms, basis, opts, _ = case("ion216_polar", 10)
    S = energy.System(atoms, basis, opts)
    S.set_dipoles_on_demand(True)
    S.energy()
    new = util.moved(atoms, 5, 1, seed=4)
    pos = atoms["pos"].copy()
    pos[5:6] = new
    S.set_profiling(True)
    S.timings(reset=True)
    et = S.trial_energy(5, new)
    assert S.timings(reset=True)["dipole_iter"]["launches"] == 10
    S.accept()
    T = energy.System(util.with_positions(atoms, pos), basis, opts)
    assert util.close(et, T.energy(), 1e-11)
    assert util.max_rel(S.dipoles()[0], T.dipoles()[0]) < 1e-9
    S.close()
    T.close()


@pytest.mark.parametrize("label", sorted(FALLBACK))
def test_uncovered_solves_run_as_in_the_parent(label):
    with open(FALLBACK_GOLDEN) as f:
        want = json.load(f)[label]
    got = fallback_record(label)
    assert got == want, (label, got, want)


def test_polar_palmo_under_jacobi_changes_nothing_on_this_path():
    """`polar_palmo` acts under Gauss-Seidel sweeps only: under Jacobi iterations the reference's correction is zero to the bit and nothing
    runs (test_gpu_polar_wolf.test_palmo_correction holds such a context to the BITS of one without the option).  So it takes the moment
    energy and the on-demand bead loop like that context: same bits, same launches, correction 0, dipoles complete when asked for."""
    atoms, basis, opts, ref = case("ion216_polar", 10)
    P, Q = energy.System(atoms, basis, dict(opts, polar_palmo=1)), energy.System(atoms, basis, opts)
    for S in (P, Q):
        S.set_profiling(True)
        S.timings(reset=True)
    _, per, failed = energy.pi_potential_local([P, Q])
    assert not failed
    tp, tq = P.timings(reset=True), Q.timings(reset=True)
    assert tp == {k: dict(v, ms=tp[k]["ms"]) for k, v in tq.items()} and tp["dipole_iter"]["launches"] == 5
    a, b = dict(per[0]), dict(per[1])
    assert a == b
    corr, change = P.palmo_info()
    assert corr == 0.0 and not np.any(change)
    dp, dq = P.dipoles(), Q.dipoles()
    assert all(np.array_equal(x, y) for x, y in zip(dp, dq))
    assert P.timings(reset=True)["dipole_iter"]["launches"] == 5
    util.assert_matches_oracle(a, dp, ref, atoms, opts, label="ion216_polar palmo jacobi")
    assert P.energy() == a["energy"]  # eager, lone: the same bits
    P.close()
    Q.close()


@pytest.mark.parametrize("n", [64, 65])
def test_iteration_count_at_the_cap_of_the_moment_path(n):
    """kMomentsMaxIter = 64 (csrc/kernels.h): n = 64 is the longest solve whose energy comes from the moments (ring of 33 vectors, moments
    m_0 .. m_64); n = 65 keeps -1/2 E0 . mu_n with every iteration run at once.  Both against the oracle, the dipoles too."""
    atoms, basis, opts, ref = case("ion216_polar", n)
    S = energy.System(atoms, basis, opts)
    S.set_profiling(True)
    S.timings(reset=True)
    _, per, failed = energy.pi_potential_local([S])
    assert not failed
    assert S.timings(reset=True)["dipole_iter"]["launches"] == (32 if n == 64 else 65)
    obs = dict(per[0])
    dip = S.dipoles()
    assert S.timings(reset=True)["dipole_iter"]["launches"] == (32 if n == 64 else 0)
    util.assert_matches_oracle(obs, dip, ref, atoms, opts, label=f"ion216_polar n={n}")
    assert S.energy() == obs["energy"]
    S.close()


if __name__ == "__main__":  # regenerate the fall-back golden from the library MPMC_ENERGY_LIB names (see fallback_record)
    import sys

    with open(sys.argv[1], "w") as f:
        json.dump({k: fallback_record(k) for k in sorted(FALLBACK)}, f, indent=1, sort_keys=True)
