"""Exchange trials (mpmc_trial_insert_begin / mpmc_trial_remove_begin), the parts that need no GPU: the C ABI declares the two entry points
and stays at version 6, and the C++ facade's exchange trials compile with plain g++ under -Wall -Wextra -Werror."""
import json
import os
import re
import subprocess

import util

HEADER = os.path.join(util.ROOT, "include", "mpmc_energy.h")
SRC = os.path.join(util.ROOT, "tests", "cpp", "exchange_facade_check.cpp")
LIBDIR = os.path.join(util.ROOT, "mpmcxx_amd")


def squeezed(text):
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))


def test_header_declares_the_entry_points_and_keeps_the_abi():
    text = squeezed(open(HEADER).read())
    assert ("int mpmc_trial_insert_begin(mpmc_ctx *ctx, int at_index, int count, const double *pos, const double *charge, const double *polarizability, "
            "const double *epsilon, const double *sigma, const int32_t *frozen, const int32_t *has_disp, const double *mass);") in text
    assert "int mpmc_trial_remove_begin(mpmc_ctx *ctx, int first, int count);" in text
    assert re.search(r"#define MPMC_ABI_VERSION 6\b", text) and re.search(r"#define MPMC_K_COUNT 8\b", text)


def build(tmp_path):
    from mpmcxx_amd import build as mbuild

    mbuild.build_library()
    exe = os.path.join(str(tmp_path), "exchange_facade_check")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(util.ROOT, "include"), SRC, "-L", LIBDIR,
                           "-lmpmc_energy", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_facade_exchange_trials_compile_with_plain_gxx(tmp_path):
    exe = build(tmp_path)
    from mpmcxx_amd import energy

    lib = energy.lib()
    assert hasattr(lib, "mpmc_trial_insert_begin") and hasattr(lib, "mpmc_trial_remove_begin") and lib.mpmc_abi_version() == 6
    if energy.device_count() == 0:  # without a GPU the facade throws the library's error code as an int (no CPU fallback)
        out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
        assert out.returncode == 1 and json.loads(out.stdout.strip())["error"] == 101
