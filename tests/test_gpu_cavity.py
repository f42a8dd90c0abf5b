"""GPU (MI355X): the cavity-bias grid of uVT moves (mpmc_set_cavity_grid, mpmc_cavity_update, mpmc_cavity_point, mpmc_cavity_get).

Everything is an integer or a bit pattern and is compared for equality with tests/cavity_ref.py, the numpy restatement of
System::cavity_update_grid, fed with the wrapped positions of System.update_com: the occupancy of every sphere centre, the centres, the
ordered list of empty centres, cavities_open, the dart hits, the probability and the cavity volume."""
import json
import math
import os
import subprocess

import numpy as np
import pytest

import cavity_ref
import util
from mpmcxx_amd import energy

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_INVALID_SETTING = -3, 4000
GRIDS = (1, 7, 10, 17)  # 1000 and 4913 centres are no multiples of 64; 1 is a single centre
# radius -> cavities_open for G = 1, 7, 10, 17 (found on the CPU with cavity_ref): none empty / all empty / in between
RADII = {
    "lj64": {4.0: (0, 0, 0, 0), 0.05: (1, 343, 1000, 4913), 2.5: (1, 108, 75, 507)},
    "water64_polar": {12.0: (0, 0, 0, 0), 0.05: (1, 343, 1000, 4913), 2.0: (0, 135, 413, 2024)},
    "ion216_triclinic": {2.5: (1, 72, 103, 771)},   # skewed basis
    "ion216_frozen": {2.5: (1, 31, 77, 958)},       # frozen molecules stay unwrapped
}


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def box(name):
    atoms, basis, opts = util.load_fixture(name)
    return atoms, basis, util.nonpolar(opts)


def volume_of(basis):
    return energy.pbc_compute(basis)[1]


def darts_for(basis, seed):
    rng = np.random.default_rng(seed)
    return -0.5 + rng.random((energy.cavity_num_darts(volume_of(basis)), 3))


def assert_update(S, basis, G, radius, frac, label):
    """one update of S against cavity_ref on S's own wrapped positions, every output; returns (result, reference)"""
    S.set_cavity_grid(G, radius)
    res = S.cavity_update(frac)
    occ, pos, open_index = S.cavity_grid()
    ref = cavity_ref.update(basis, volume_of(basis), S.update_com()[2], G, radius, frac)
    assert res["total_points"] == G ** 3 == ref["total_points"], label
    assert np.array_equal(occ.reshape(-1), ref["occupancy"]), (label, "occupancy", int(np.count_nonzero(occ.reshape(-1) != ref["occupancy"])))
    assert np.array_equal(bits(pos.reshape(-1, 3)), bits(ref["grid"])), (label, "sphere centres")
    assert np.array_equal(open_index, ref["open_index"]), (label, "open list")
    assert res["cavities_open"] == ref["cavities_open"] == len(open_index), (label, res, ref["cavities_open"])
    assert res["n_darts"] == ref["n_darts"] and res["hits"] == ref["hits"], (label, res, ref["hits"])
    assert bits(res["probability"]) == bits(ref["probability"]), (label, res, ref["probability"])
    assert bits(res["cavity_volume"]) == bits(ref["cavity_volume"]), (label, res, ref["cavity_volume"])
    return res, ref


# ---- 1. parity on the smallest boxes that reach every branch -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def systems():
    made = {}

    def get(name):
        if name not in made:
            atoms, basis, opts = box(name)
            made[name] = (energy.System(atoms, basis, opts), basis)
        return made[name]

    yield get
    for S, _ in made.values():
        S.close()


@pytest.mark.parametrize("G", GRIDS)
@pytest.mark.parametrize("name", list(RADII))
def test_parity_with_the_restatement(systems, name, G):
    S, basis = systems(name)
    frac = darts_for(basis, seed=1000 + G)
    for radius, expected_open in RADII[name].items():
        label = f"{name} G={G} radius={radius}"
        res, ref = assert_update(S, basis, G, radius, frac, label)
        assert ref["cavities_open"] == expected_open[GRIDS.index(G)], (label, ref["cavities_open"])
        grid = ref["grid"]
        for rank in range(res["cavities_open"]):
            assert np.array_equal(bits(S.cavity_point(rank)), bits(grid[ref["open_index"][rank]])), (label, rank)
        for rank in (-1, res["cavities_open"]):
            with pytest.raises(energy.MpmcError) as e:
                S.cavity_point(rank)
            assert e.value.code == ERR_ARG, label
        if res["cavities_open"] == 0:
            assert res["hits"] == 0 and res["cavity_volume"] == 0.0 and res["probability"] == 0.0, (label, res)


def test_parity_where_a_slice_streams_several_chunks():
    """lj1000, G = 40, radius 2.5 (8589 of 64000 centres empty): 1000 blocks of centres leave 3 slices of 334 atoms, two LDS chunks of 256 each;
    6400 darts in 100 waves walk the open list in 21 slices of two chunks, and most waves leave early (6208 hits)."""
    atoms, basis, opts = box("lj1000")
    S = energy.System(atoms, basis, opts)
    try:
        res, ref = assert_update(S, basis, 40, 2.5, darts_for(basis, 40), "lj1000 G=40")
        assert res["cavities_open"] == 8589 and res["n_darts"] == 6400
        for rank in (0, 1, 4294, 8588):
            assert np.array_equal(bits(S.cavity_point(rank)), bits(ref["grid"][ref["open_index"][rank]]))
    finally:
        S.close()


@pytest.mark.parametrize("G,waves,per,expected_open", [(41, 1077, 2, 9142), (65, 4292, 5, 39271)])
def test_parity_where_a_scan_thread_sums_several_waves(systems, G, waves, per, expected_open):
    """k_cavity_compact_scan gives each of its 1024 threads ceil(waves / 1024) wave counts; up to G = 40 (1000 waves) that is one.
    lj64, radius 2.5: G = 41 has 1077 waves of centres, two per thread, the 539th thread holds one and the rest none; G = 65 has 4292,
    five per thread.  cavities_open found on the CPU with cavity_ref."""
    assert (G ** 3 + 63) // 64 == waves and (waves + 1023) // 1024 == per and waves % per != 0
    S, basis = systems("lj64")
    res, ref = assert_update(S, basis, G, 2.5, darts_for(basis, seed=1000 + G), f"lj64 G={G}")
    assert res["cavities_open"] == expected_open, res
    for rank in (0, 1, expected_open // 2, expected_open - 1):
        assert np.array_equal(bits(S.cavity_point(rank)), bits(ref["grid"][ref["open_index"][rank]])), (G, rank)


# ---- 2. the boundary ---------------------------------------------------------------------------------------------------------------------------
def frozen_atoms(pos):
    n = len(pos)
    return {"pos": np.array(pos, dtype=np.float64), "charge": np.zeros(n), "polarizability": np.zeros(n), "epsilon": np.full(n, 100.0), "sigma": np.full(n, 3.0),
            "mass": np.full(n, 40.0), "mol_id": np.arange(n, dtype=np.int32), "frozen": np.ones(n, dtype=np.int32), "has_disp": np.zeros(n, dtype=np.int32)}


def test_the_boundary_is_strict():
    """Cubic cell of edge 32, G = 7: the centres are the multiples of 4 from -12 to 12, every coordinate below is exact.  Single-atom frozen
    molecules (frozen: wrapping cannot move them)."""
    below = math.nextafter(2.5, 0.0)
    pos = [(-9.5, -12.0, -12.0),   # centre (0,0,0) + (2.5, 0, 0): on the sphere, outside
           (-2.5, -2.0, -4.0),     # centre (2,2,2) = (-4,-4,-4) + (1.5, 2.0, 0): r^2 = 6.25 exactly, outside (of centre (2,3,2) likewise)
           (below, 8.0, 8.0),      # centre (3,5,5) = (0,8,8) + (nextafter(2.5, 0), 0, 0): inside
           (8.5, 8.0, -8.0), (8.0, 7.0, -7.5),  # two atoms inside the sphere of centre (5,5,1) = (8,8,-8)
           (4.0, 0.0, 0.0), (-4.0, 0.0, 0.0), (0.0, 4.0, 0.0), (0.0, -4.0, 0.0), (0.0, 0.0, 4.0), (0.0, 0.0, -4.0)]  # the six neighbours of the origin are occupied
    basis = np.diag([32.0, 32.0, 32.0])
    _, _, opts = box("lj64")
    S = energy.System(frozen_atoms(pos), basis, opts)
    try:
        assert np.array_equal(bits(S.update_com()[2]), bits(np.array(pos)))
        # darts around the empty origin, dart_frac = position / 32 (exact): on the sphere, r^2 = 6.25 exactly, just inside, the centre itself, far away
        dart_pos = np.array([(2.5, 0.0, 0.0), (1.5, 2.0, 0.0), (below, 0.0, 0.0), (0.0, 0.0, 0.0), (-14.0, 14.0, -14.0)])
        res, ref = assert_update(S, basis, 7, 2.5, dart_pos / 32.0, "boundary")
        assert np.array_equal(bits(cavity_ref.dart_positions(basis, dart_pos / 32.0)), bits(dart_pos))
        occ = S.cavity_grid()[0]
        assert occ[0, 0, 0] == 0 and occ[1, 0, 0] == 1        # the first atom: outside its own sphere, 1.5 from the next centre
        assert occ[2, 2, 2] == 0 and occ[2, 3, 2] == 0        # r^2 = 6.25 exactly, twice
        assert occ[3, 5, 5] == 1 and occ[5, 5, 1] == 2 and occ[3, 3, 3] == 0 and occ[4, 3, 3] == 1
        assert list(ref["hit"]) == [False, False, True, True, False] and res["hits"] == 2
    finally:
        S.close()


# ---- 3. it disturbs nothing --------------------------------------------------------------------------------------------------------------------
def test_an_update_disturbs_nothing():
    atoms, basis, opts = box("water64_polar")
    S = energy.System(atoms, basis, opts)
    plain = energy.System(atoms, basis, opts)
    named = energy.System(atoms, basis, dict(opts, cavity_bias=1, cavity_grid_size=10, cavity_radius=2.0))  # (switched on through the options, never updated)
    try:
        trial = util.moved(atoms, 0, 3, seed=3)
        e0 = S.energy()
        mem_energy = S.memory_usage()
        t0 = S.trial_energy(0, trial)
        obs0 = dict(S.trial_observables)
        S.reject()
        mem_before = S.memory_usage()
        S.set_cavity_grid(10, 2.0)
        res = S.cavity_update(darts_for(basis, 5))
        assert 0 < res["cavities_open"] < 1000
        t1 = S.trial_energy(0, trial)
        assert not S.last_trial_was_full() and bits(t1) == bits(t0) and S.trial_observables == obs0
        S.reject()
        assert bits(S.energy()) == bits(e0)
        # the device memory of a context that never updates a grid is what it was: nothing is allocated for the grid before its first update
        assert plain.energy() == e0 and named.energy() == e0
        assert plain.memory_usage() == named.memory_usage() == mem_energy
        assert S.memory_usage()[0] >= mem_before[0] + 3 * 1000 * 8 and S.memory_usage()[1] == mem_before[1]
    finally:
        for s in (S, plain, named):
            s.close()


# ---- 4. it follows the composition ------------------------------------------------------------------------------------------------------------
def test_updates_follow_accepted_and_rejected_exchanges():
    atoms, basis, opts = box("water64_polar")
    n = len(atoms["pos"])
    G, radius = 10, 2.0
    S = energy.System(atoms, basis, opts, max_atoms=n + 2)
    frac = darts_for(basis, 9)

    def check(label):
        res, ref = assert_update(S, basis, G, radius, frac, label)  # (no energy() in between: the exchange's upload is still pending)
        fresh = energy.System({k: np.array(v) for k, v in S.atoms.items()}, basis, opts)
        try:
            assert_update(fresh, basis, G, radius, frac, label + " (fresh)")
            assert fresh.cavity_update(frac) == res, label
            for a, b in zip(S.cavity_grid(), fresh.cavity_grid()):
                assert np.array_equal(a, b), label
        finally:
            fresh.close()
        return res

    def at_cavity(a, b, rank):
        p = S.atoms["pos"][a:b]
        return {k: np.array(v[a:b]) for k, v in S.atoms.items()} | {"pos": p - p[0] + S.cavity_point(rank)}

    try:
        S.energy()
        r0 = check("start")
        S.trial_insert_energy(n, at_cavity(n - 1, n, r0["cavities_open"] // 2))  # one more Xe atom on an empty centre: n + 1 atoms
        S.accept()
        r1 = check("accepted insertion")
        assert S.n == n + 1 and r1["cavities_open"] < r0["cavities_open"]
        S.trial_remove_energy(9, 3)  # the fourth water
        S.accept()
        r2 = check("accepted removal")
        assert S.n == n - 2 and r2["cavities_open"] >= r1["cavities_open"]
        S.trial_insert_energy(0, at_cavity(0, 3, 0))
        S.reject()
        assert check("rejected insertion") == r2
        two = [at_cavity(0, 3, rank) for rank in (0, r2["cavities_open"] - 1)]  # (both picked now: an accepted insertion ends the update's validity)
        for mol in two:  # n + 1, then n + 4 atoms: past max_atoms, the context is rebuilt and the setting survives
            S.trial_insert_energy(S.n, mol)
            S.accept()
        assert S.n == n + 4
        res = S.cavity_update(frac)  # (the grid is still on: no set_cavity_grid since the growth)
        assert res["total_points"] == G ** 3
        assert check("grown") == res
    finally:
        S.close()


# ---- 5. determinism and refusals ---------------------------------------------------------------------------------------------------------------
def refused(call, code=ERR_ARG):
    with pytest.raises(energy.MpmcError) as e:
        call()
    assert e.value.code == code and len(str(e.value)) > len(f"mpmc error {code}: "), str(e.value)


def test_determinism_and_refusals():
    atoms, basis, opts = box("lj64")
    S = energy.System(atoms, basis, opts)
    bare = energy.System({k: v for k, v in atoms.items() if k != "mass"}, basis, opts)
    frac = darts_for(basis, 11)
    try:
        refused(lambda: S.cavity_update(frac))  # the grid is off
        refused(lambda: S.set_cavity_grid(5, -1.0), ERR_INVALID_SETTING)
        refused(lambda: S.set_cavity_grid(129, 2.0), ERR_INVALID_SETTING)
        refused(lambda: S.set_cavity_grid(-3, 2.0), ERR_INVALID_SETTING)
        refused(lambda: S.set_cavity_grid(5, float("nan")), ERR_INVALID_SETTING)
        S.set_cavity_grid(10, 2.5)
        refused(lambda: S.cavity_point(0))  # no update yet
        first = S.cavity_update(frac)
        arrays = S.cavity_grid()
        assert S.cavity_update(frac) == first and all(np.array_equal(a, b) for a, b in zip(arrays, S.cavity_grid()))
        S.cavity_point(0)
        S.update_positions(0, atoms["pos"][:1] + 0.25)
        refused(lambda: S.cavity_point(0))  # the atoms moved since the update
        refused(lambda: S.cavity_grid())
        assert_update(S, basis, 10, 2.5, frac, "after update_positions")
        S.energy()
        S.trial_energy(3, util.moved(atoms, 3, 1, seed=4))
        refused(lambda: S.cavity_update(frac))  # a trial is open
        S.reject()
        assert_update(S, basis, 10, 2.5, frac, "after the refused update")
        bare.set_cavity_grid(10, 2.5)
        refused(lambda: bare.cavity_update(frac))  # no masses
        assert np.isfinite(bare.energy())
        # no darts: NaN volume as in the reference, exact counts
        for none in (None, np.zeros((0, 3))):
            res, ref = assert_update(S, basis, 10, 2.5, none, "no darts")
            assert res["n_darts"] == 0 and res["hits"] == 0 and math.isnan(res["cavity_volume"]) and res["cavities_open"] == ref["cavities_open"] > 0
        S.set_cavity_grid(0)
        refused(lambda: S.cavity_update(frac))
        assert np.isfinite(S.energy())
    finally:
        S.close()
        bare.close()


# ---- 6. the facade -----------------------------------------------------------------------------------------------------------------------------
def test_facade_draws_the_darts_from_the_callers_generator(tmp_path):
    lib = os.path.join(util.ROOT, "mpmcxx_amd")
    exe = str(tmp_path / "cavity_facade")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(util.ROOT, "include"),
                           os.path.join(util.ROOT, "tests", "cpp", "cavity_facade.cpp"), "-L", lib, "-lmpmc_energy", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib",
                           "-o", exe])
    G, radius = 10, 2.5
    out = subprocess.run([exe, os.path.join(util.GOLDEN, "lj64.in"), str(G), repr(radius)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    got = json.loads(out.stdout)
    atoms, basis, opts = box("lj64")
    S = energy.System(atoms, basis, opts)
    try:
        n_darts = cavity_ref.num_darts(volume_of(basis))
        u = cavity_ref.mt19937_uniforms(3 * n_darts + 1)  # the default-seeded std::mt19937 through uniform_real_distribution<double>
        frac = (-0.5 + u[:3 * n_darts]).reshape(n_darts, 3)
        ref = cavity_ref.update(basis, volume_of(basis), S.update_com()[2], G, radius, frac)
    finally:
        S.close()
    assert got["n_darts"] == n_darts == 409 and got["cavities_open"] == ref["cavities_open"] == 75 and got["hits"] == ref["hits"]
    assert got["probability"] == ref["probability"] and got["cavity_volume"] == ref["cavity_volume"] and got["u"] == u[-1]
    point = ref["grid"][ref["open_index"][cavity_ref.insertion_index(ref["cavities_open"], u[-1])]]
    assert got["point"] == [float(v) for v in point]
