"""Volume trials (mpmc_trial_volume_begin) and the NPT acceptance factor, the parts that need no GPU: the C ABI declares the entry points
and keeps its constants, mpmc_npt_boltzmann_factor is the ENSEMBLE_NPT branch of System::boltzmann_factor (reference
src/System.MonteCarlo.cpp:1441-1457) operand for operand, and the C++ facade's volume trials and the Gibbs example compile with plain g++
under -Wall -Wextra -Werror.  One GPU test runs the facade check (tests/cpp/volume_trial_check.cpp)."""
import ctypes
import json
import math
import os
import re
import subprocess

import pytest

import util

HEADER = os.path.join(util.ROOT, "include", "mpmc_energy.h")
SRC = os.path.join(util.ROOT, "tests", "cpp", "volume_trial_check.cpp")
LIBDIR = os.path.join(util.ROOT, "mpmcxx_amd")
ATM2REDUCED = 0.0073389366  # src/constants.h
VOLUME, DISPLACE, INSERT = 5, 2, 0  # MPMC_MOVETYPE_*


def squeezed(text):
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))


def test_header_declares_the_entry_points_and_keeps_the_abi():
    text = squeezed(open(HEADER).read())
    for decl in ("int mpmc_trial_volume_begin(mpmc_ctx *ctx, double basis_scale_factor);",
                 "int mpmc_trial_volume_get(mpmc_ctx *ctx, double basis[9], double reciprocal[9], double *volume, double *cutoff, double *pos );",
                 "int mpmc_debug_volume_trial_counts(mpmc_ctx *ctx, long long out4[4]);",
                 "int mpmc_npt_boltzmann_factor(const mpmc_npt_move *move, double *boltzmann_factor);"):
        assert decl in text, decl
    assert re.search(r"#define MPMC_ABI_VERSION 6\b", text) and re.search(r"#define MPMC_K_COUNT 8\b", text)
    assert re.search(r"#define MPMC_TRIAL_MAX_ATOMS 256\b", text)


def test_ctypes_declarations_and_struct_layouts():
    from mpmcxx_amd import energy

    L = energy.lib()
    for name in ("mpmc_trial_volume_begin", "mpmc_trial_volume_get", "mpmc_debug_volume_trial_counts", "mpmc_npt_boltzmann_factor"):
        assert getattr(L, name).argtypes is not None, name
    assert L.mpmc_abi_version() == 6
    assert ctypes.sizeof(energy.NptMove) == 8 + 7 * 8
    assert ctypes.sizeof(energy.Result) == 16 * 8 + 7 * 8 + 2 * 4 and len(energy.Timings().ms) == 8  # mpmc_result and mpmc_timings keep their layout


def npt_restated(movetype, T, pressure, N, init, final, v_old, v_new):
    delta_energy = final - init
    if movetype == VOLUME:
        return math.exp(-(delta_energy + pressure * ATM2REDUCED * (v_new - v_old) - (N + 1) * T * math.log(v_new / v_old)) / T)
    return math.exp(-delta_energy / T)


NPT_TABLE = [(T, p, N, init, final, v_old, v_new)
             for T in (77.0, 298.15)
             for p in (1.0, 250.0)
             for N, init, final in ((64.0, -43859.30447683911, -43861.5), (216.0, 1643134.465774632, 1643100.25), (1.0, -3.5, 2.25))
             for v_old, v_new in ((15625.0, 15625.0 * 1.04 ** 3), (27000.0, 27000.0 * 0.97 ** 3), (8000.0, 8000.0))]


def test_npt_factor_is_the_reference_expression_exactly():
    from mpmcxx_amd import energy

    for row in NPT_TABLE:
        for movetype in (VOLUME, DISPLACE):
            try:
                want = npt_restated(movetype, *row)
            except OverflowError:  # (math.exp raises where exp() returns inf)
                want = math.inf
            got = energy.npt_boltzmann_factor(movetype, *row)
            assert got == want, (movetype, row, got, want)
    assert energy.npt_boltzmann_factor("volume", *NPT_TABLE[0]) == energy.npt_boltzmann_factor(VOLUME, *NPT_TABLE[0])
    # a non-finite final_energy: delta_energy = +inf, -(inf + finite) / T = -inf, exp(-inf) = 0 -- the move is never accepted; a NaN stays a
    # NaN (the reference's `rand < boltzmann_factor` is then false as well)
    T, p, N, init, _, v_old, v_new = NPT_TABLE[0]
    for movetype in (VOLUME, DISPLACE):
        assert energy.npt_boltzmann_factor(movetype, T, p, N, init, math.inf, v_old, v_new) == 0.0
        assert math.isnan(energy.npt_boltzmann_factor(movetype, T, p, N, init, math.nan, v_old, v_new))


def test_npt_factor_refuses_other_moves():
    from mpmcxx_amd import energy

    with pytest.raises(energy.MpmcError) as e:
        energy.npt_boltzmann_factor(INSERT, *NPT_TABLE[0])
    assert e.value.code == 4004
    assert energy.lib().mpmc_npt_boltzmann_factor(None, None) == -3


def compile_plain(src, exe, extra=()):
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(util.ROOT, "include"), src, "-L", LIBDIR,
                           "-lmpmc_energy", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe] + list(extra))
    return exe


@pytest.fixture(scope="module")
def facade_check(tmp_path_factory):
    from mpmcxx_amd import build as mbuild

    mbuild.build_library()
    return compile_plain(SRC, str(tmp_path_factory.mktemp("volume") / "volume_trial_check"))


def test_facade_volume_trials_and_the_gibbs_example_compile_with_plain_gxx(facade_check, tmp_path):
    compile_plain(os.path.join(util.ROOT, "examples", "gibbs_nvt.cpp"), str(tmp_path / "gibbs_nvt"))
    from mpmcxx_amd import energy

    if energy.device_count() == 0:  # without a GPU the facade throws the library's error code as an int (no CPU fallback)
        out = subprocess.run([facade_check], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
        assert out.returncode == 1 and json.loads(out.stdout.strip())["error"] == 101


@pytest.mark.gpu
def test_facade_volume_trials_on_the_device(facade_check):
    out = subprocess.run([facade_check], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout, out.stderr)
    r = json.loads(out.stdout.strip())
    assert r["e_rej"] != r["e0"] and r["v_trial"] == pytest.approx(r["v0"] * 1.04 ** 3, rel=1e-14)
    assert r["e_back"] == r["e0"] and r["v_back"] == r["v0"]  # a rejected trial leaves the facade and the context alone: the same bits
    assert r["v_acc"] == pytest.approx(r["v0"] * 0.97 ** 3, rel=1e-14)
    for trial, again in (("e_acc", "e_acc_again"), ("e_acc", "e_acc_fresh"), ("e_two", "e_two_fresh")):
        assert abs(r[trial] - r[again]) <= 1e-11 * abs(r[again]), (trial, again, r)
    assert r["refused"] == 6001
