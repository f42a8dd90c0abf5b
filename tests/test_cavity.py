"""The cavity-bias grid of uVT moves (mpmc_set_cavity_grid / mpmc_cavity_update), the parts that need no GPU: the exact distance threshold, the
sphere centres, the dart count, the uVT acceptance factor and the Python / reader wiring.  Everything is integers or bit-equality against
tests/cavity_ref.py."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import cavity_ref
import util
from mpmcxx_amd import energy, pqr

HEADER = os.path.join(util.ROOT, "include", "mpmc_energy.h")


def bits(x):
    return np.float64(x).view(np.uint64)


# ---- the threshold ----------------------------------------------------------------------------------------------------------------------
def test_r2_threshold_is_the_smallest_double_whose_root_reaches_the_radius():
    rng = np.random.default_rng(20240607)
    for R in [2.5] + list(rng.uniform(0.5, 8.0, size=200)):
        R = float(R)
        T = energy.cavity_r2_threshold(R)
        assert math.sqrt(T) >= R and math.sqrt(math.nextafter(T, 0.0)) < R, (R, T)
    # (the threshold may lie below the square: the correctly rounded root of the double below 6.25 is 2.5 already, and the reference keeps such r out)
    assert energy.cavity_r2_threshold(2.5) <= 6.25 and math.sqrt(6.25) == 2.5
    assert all(math.isnan(energy.cavity_r2_threshold(v)) for v in (0.0, -1.0, float("inf"), float("nan")))


def test_numpy_sqrt_is_math_sqrt():
    """cavity_ref takes numpy's square root of a vector where the reference takes sqrt of a scalar: the same correctly rounded function"""
    x = np.random.default_rng(5).uniform(0.0, 400.0, size=20000)
    assert all(float(a) == math.sqrt(float(b)) for a, b in zip(np.sqrt(x), x))


# ---- sphere centres -----------------------------------------------------------------------------------------------------------------------
CUBE32 = np.diag([32.0, 32.0, 32.0])


@pytest.mark.parametrize("name", ["lj64", "ion216_triclinic", "cube32"])
def test_grid_points_match_the_restatement_bit_for_bit(name):
    basis = CUBE32 if name == "cube32" else util.load_fixture(name)[1]
    for G in (1, 7, 10):
        ref = cavity_ref.grid_points(basis, G)
        at = 0
        for i in range(G):
            for j in range(G):
                for k in range(G):
                    got = energy.cavity_grid_point(basis, G, i, j, k)
                    one = cavity_ref.grid_point(basis, G, i, j, k)
                    assert [bits(v) for v in got] == [bits(v) for v in one] == [bits(v) for v in ref[at]], (name, G, i, j, k, got, one, ref[at])
                    at += 1


def test_cubic_cell_grid_of_seven_is_exact():
    for i in range(7):
        for j in range(7):
            for k in range(7):
                assert list(energy.cavity_grid_point(CUBE32, 7, i, j, k)) == [4.0 * (i + 1) - 16.0, 4.0 * (j + 1) - 16.0, 4.0 * (k + 1) - 16.0]
    with pytest.raises(energy.MpmcError):
        energy.cavity_grid_point(CUBE32, 7, 7, 0, 0)


def test_num_darts_truncates_toward_zero():
    assert energy.cavity_num_darts(999.99) == 99 and energy.cavity_num_darts(9.9) == 0 and energy.cavity_num_darts(4096.0) == 409
    assert all(energy.cavity_num_darts(v) == cavity_ref.num_darts(v) for v in (2744.0, 12144.0, 13824.000000000011, 1e5))


# ---- the acceptance factor ----------------------------------------------------------------------------------------------------------------
def test_uvt_boltzmann_factor_matches_the_restatement():
    """Equal bits: both sides call the same libm exp and round every other operation once, in the same order."""
    rng = np.random.default_rng(77)
    for _ in range(50):
        T, fug, V = rng.uniform(40, 400), rng.uniform(0.1, 50), rng.uniform(1e3, 1e5)
        N, e0 = float(rng.integers(1, 400)), rng.uniform(-5e4, 0)
        e1 = e0 + rng.normal(scale=3 * T)
        count, cv, prob = int(rng.integers(1, 4)), rng.uniform(10, V), rng.uniform(0.01, 1.0)
        for biased in (False, True):
            for mv in (cavity_ref.INSERT, cavity_ref.REMOVE, cavity_ref.DISPLACE):
                rc, got = energy.uvt_boltzmann_factor(mv, T, fug, V, N, e0, e1, sorbate_count=count, biased_move=biased, cavity_volume=cv, avg_cavity_probability=prob)
                want = cavity_ref.uvt_boltzmann_factor(mv, biased, T, fug, V, N, e0, e1, count, cv, prob)
                assert rc == 0 and bits(got) == bits(want), (biased, mv, got, want)


def test_uvt_boltzmann_factor_refuses_other_move_types():
    for biased in (False, True):
        for mv in ("spinflip", "volume", "adiabatic", 17):
            rc, _ = energy.uvt_boltzmann_factor(mv, 100.0, 1.0, 1e4, 10.0, -1.0, -2.0, biased_move=biased, cavity_volume=1.0, avg_cavity_probability=0.5)
            assert rc == energy.ERR_UNSUPPORTED == 4004


# ---- wiring -------------------------------------------------------------------------------------------------------------------------------
def squeezed(text):
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))


def test_header_declares_the_entry_points_and_the_structs_match():
    text = squeezed(open(HEADER).read())
    for decl in ("int mpmc_set_cavity_grid(mpmc_ctx *ctx, int grid_size, double radius);",
                 "int mpmc_cavity_update(mpmc_ctx *ctx, int n_darts, const double *dart_frac , mpmc_cavity_result *out);",
                 "int mpmc_cavity_point(mpmc_ctx *ctx, int64_t open_rank, double pos[3]);",
                 "int mpmc_cavity_get(mpmc_ctx *ctx, int32_t *occupancy , double *grid_pos , int32_t *open_flat_index );",
                 "int mpmc_cavity_num_darts(double volume);",
                 "int mpmc_cavity_grid_point(const double basis[9], int grid_size, int i, int j, int k, double pos[3]);",
                 "double mpmc_cavity_r2_threshold(double radius);",
                 "int mpmc_uvt_boltzmann_factor(const mpmc_uvt_move *move, double *boltzmann_factor);"):
        assert decl in text, decl
    assert re.search(r"#define MPMC_ABI_VERSION 6\b", text) and re.search(r"#define MPMC_K_COUNT 8\b", text)
    assert re.search(r"#define MPMC_CAVITY_MAX_GRID 128\b", text) and energy.CAVITY_MAX_GRID == 128
    # the structs as the header lays them out: four int64 + two doubles; three int32 (padded to 16 bytes) + eight doubles
    assert "typedef struct mpmc_cavity_result { int64_t total_points, cavities_open, n_darts, hits; double probability, cavity_volume; } mpmc_cavity_result;" in text
    assert ("typedef struct mpmc_uvt_move { int32_t movetype, biased_move, sorbate_count; double temperature, fugacity, volume, N, init_energy, final_energy, "
            "cavity_volume, avg_cavity_probability; } mpmc_uvt_move;") in text
    assert C.sizeof(energy.CavityResult) == 4 * 8 + 2 * 8 and C.sizeof(energy.UvtMove) == 16 + 8 * 8
    assert energy.UvtMove.temperature.offset == 16 and energy.CavityResult.probability.offset == 32
    L = energy.lib()
    assert all(hasattr(L, n) for n in ("mpmc_set_cavity_grid", "mpmc_cavity_update", "mpmc_cavity_point", "mpmc_cavity_get")) and L.mpmc_abi_version() == 6


# what the parent's reader returns for lj64.in (a file without the three keywords must read exactly as before)
LJ64_OPTIONS = {"rd_only": 1, "rd_lrc": 1, "polarization": 0, "polar_iterative": 0, "polar_ewald": 0, "polar_max_iter": 10, "polar_gs": 0, "polar_rrms": 0,
                "ewald_kmax": 7, "polar_precision": 0.0, "polar_gamma": 1.0, "polar_damp": 0.0, "damp_type": None, "ewald_alpha": None,
                "polar_ewald_alpha": None, "wolf": 0, "feynman_hibbs": 0, "feynman_hibbs_order": 0, "temperature": 100.0}


def test_readers_parse_the_three_keywords_and_nothing_else(tmp_path):
    src = os.path.join(util.GOLDEN, "lj64.in")
    got = pqr.read_input(src)["options"]
    assert got == LJ64_OPTIONS and list(got) == list(LJ64_OPTIONS)
    text = open(src).read().replace("pqr_input lj64.pqr", "pqr_input " + os.path.join(util.GOLDEN, "lj64.pqr"))
    for grid_key in ("cavity_grid", "cavity_grid_size"):  # (the reference's keyword, and the name of the field it fills)
        path = os.path.join(str(tmp_path), grid_key + ".in")
        with open(path, "w") as f:
            f.write(text + f"cavity_bias on\n{grid_key} 17\ncavity_radius 2.5\n")
        opts = pqr.read_input(path)["options"]
        assert {k: opts[k] for k in energy.CAVITY_KEYS} == {"cavity_bias": 1, "cavity_grid_size": 17, "cavity_radius": 2.5}
        assert {k: v for k, v in opts.items() if k not in energy.CAVITY_KEYS} == LJ64_OPTIONS
    header = open(os.path.join(util.ROOT, "include", "mpmc_io.hpp")).read()
    assert all(f'k == "{k}"' in header for k in ("cavity_bias", "cavity_grid", "cavity_grid_size", "cavity_radius"))


def test_insertion_index_and_the_uniform_stream():
    assert [cavity_ref.insertion_index(10, u) for u in (0.0, 0.04, 0.5, 0.999999)] == [9, 9, 5, 0]  # (4.5 rounds to even: 4)
    u = cavity_ref.mt19937_uniforms(3)
    assert [float(v) for v in u] == [0.1354770042967805, 0.8350085899945795, 0.96886777112423139]  # std::mt19937{} through uniform_real_distribution<double>
