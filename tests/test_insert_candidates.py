"""Batched insertion candidates (mpmc_insert_candidates), the parts that need no GPU: the C ABI declares the call and its cap and stays at
version 6 with eight timing classes, the built library exports the two symbols, build.py lists the new source, the gfx950 code object
holds the two kernels (without scratch memory), the ctypes prototypes exist, and the C++ facade's call compiles with plain g++ under -Wall -Wextra
-Werror."""
import json
import os
import re
import subprocess

import util
from mpmcxx_amd import build as mbuild
from mpmcxx_amd import energy
from test_cabi import _kernel_notes

HEADER = os.path.join(util.ROOT, "include", "mpmc_energy.h")
SRC = os.path.join(util.ROOT, "tests", "cpp", "insert_candidates_check.cpp")
LIBDIR = os.path.join(util.ROOT, "mpmcxx_amd")


def squeezed(text):
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))


def header_constant(name):
    found = re.findall(r"#define " + name + r" (\d+)\b", open(HEADER).read())
    assert len(found) == 1, (name, found)
    return int(found[0])


def test_header_declares_the_call_and_keeps_the_abi():
    text = squeezed(open(HEADER).read())
    assert ("int mpmc_insert_candidates(mpmc_ctx *ctx, int count, int n_cand, const double *pos , const double *charge, const double *polarizability, "
            "const double *epsilon, const double *sigma, const int32_t *frozen, const int32_t *has_disp, const double *mass, mpmc_result *out );") in text
    assert "int mpmc_debug_insert_batch_counts(mpmc_ctx *ctx, long long *out2);" in text
    assert header_constant("MPMC_INSERT_MAX_CANDIDATES") >= 4096
    assert header_constant("MPMC_ABI_VERSION") == 6 and header_constant("MPMC_K_COUNT") == 8 and header_constant("MPMC_TRIAL_MAX_ATOMS") == 256


def test_library_exports_the_symbols_and_ctypes_binds_them():
    mbuild.build_library()
    L = energy.lib()
    assert L.mpmc_abi_version() == 6
    for name in ("mpmc_insert_candidates", "mpmc_debug_insert_batch_counts"):
        assert hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name
    assert len(L.mpmc_insert_candidates.argtypes) == 12 and len(L.mpmc_debug_insert_batch_counts.argtypes) == 2
    assert callable(energy.System.insert_candidates) and callable(energy.System.insert_batch_counts)


def test_build_lists_the_new_source_and_the_shared_header():
    assert "kernels_insert_batch.hip" in mbuild.SOURCES and "kernels_exchange.hip" in mbuild.SOURCES
    assert "exchange_kernels.h" in mbuild.HEADERS  # (a change of the shared block roles rebuilds both files)
    for f in ("kernels_insert_batch.hip", "exchange_kernels.h"):
        assert os.path.exists(os.path.join(mbuild.CSRC, f)), f


def test_code_object_holds_the_batch_kernels_without_scratch():
    """no VGPR spill and no scratch memory, at most 128 VGPRs (four waves per SIMD).  Like k_exchange_all and k_delta_all, whose three
    block roles it carries, the main kernel parks some of its many kernel-argument scalars in VGPR lanes; that costs no memory traffic."""
    notes = _kernel_notes("kernels_insert_batch.hip.o")
    main = [k for k in notes if "k_insert_batch_all" in k]
    finish = [k for k in notes if "k_insert_batch_finish" in k]
    assert len(main) == 4 and len(finish) == 1, list(notes)  # orthorhombic / skewed x plain / extended (Wolf, Feynman-Hibbs)
    for name in main + finish:
        meta = notes[name]
        assert meta["vgpr_spill_count"] == 0 and meta["private_segment_fixed_size"] == 0, (name, meta)
        assert meta["vgpr_count"] <= 128, (name, meta)
    # the single trial keeps its own four instantiations, built from the same block roles
    assert len([k for k in _kernel_notes("kernels_exchange.hip.o") if "k_exchange_all" in k]) == 4


def test_the_host_arithmetic_is_shared_not_restated():
    """xch_compose is the one place that turns posted changes into an mpmc_result: the single trial and the batch both call it"""
    text = util.csrc_text("trial.cpp")
    assert len(re.findall(r"static void xch_compose\(", text)) == 1
    assert len(re.findall(r"\bxch_compose\(c, ", text)) == 2
    assert len(re.findall(r"r\.es_real = a\.es_real \+ \(p\.es_real - p\.es_intra\)", text)) == 1
    assert len(re.findall(r"\bdelta_finish_sums\(", util.csrc_text("kernels_delta.hip"))) == 1
    assert len(re.findall(r"\bdelta_finish_sums\(", util.csrc_text("kernels_insert_batch.hip"))) == 1


def build(tmp_path):
    mbuild.build_library()
    exe = os.path.join(str(tmp_path), "insert_candidates_check")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(util.ROOT, "include"), SRC, "-L", LIBDIR,
                           "-lmpmc_energy", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_facade_call_compiles_with_plain_gxx(tmp_path):
    exe = build(tmp_path)
    if energy.device_count() == 0:  # without a GPU the facade throws the library's error code as an int (no CPU fallback)
        out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
        assert out.returncode == 1 and json.loads(out.stdout.strip())["error"] == 101
