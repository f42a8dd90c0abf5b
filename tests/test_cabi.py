"""CPU: the C-ABI library builds (hipcc cross-compiles gfx950), loads, and exports every symbol that
include/mpmc_energy.h declares.  No compute calls here (there is no GPU in this container)."""
import ctypes
import os
import re

import numpy as np
import pytest

import util
from mpmcxx_amd import build as mbuild
from mpmcxx_amd import energy


def declared_symbols():
    hdr = open(os.path.join(util.ROOT, "include", "mpmc_energy.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(mpmc_[a-z_0-9]+)\s*\(", hdr)))


def test_library_builds_and_exports_every_declared_symbol():
    path = mbuild.build_library()
    assert os.path.exists(path)
    L = ctypes.CDLL(path)
    syms = declared_symbols()
    assert len(syms) >= 30
    missing = [s for s in syms if not hasattr(L, s)]
    assert not missing, missing
    assert L.mpmc_abi_version() == 6


def test_code_object_is_gfx950():
    data = open(mbuild.build_library(), "rb").read()
    assert b"gfx950" in data
    for kern in (b"k_pair_fused", b"k_pair_sweep", b"k_recip_sf", b"k_dipole_iter_hybrid", b"k_dipole_iter_panel", b"k_build_panels", b"k_field_delta", b"k_dense_matvec", b"k_dense_symv", b"k_polar_energy_and_pairs", b"k_gs_stage", b"k_classify", b"k_atom_terms"):
        assert kern in data, kern


def test_struct_layouts_match_header():
    # sizes the C side compiled with (guards the ctypes mirrors in mpmcxx_amd/energy.py)
    assert ctypes.sizeof(energy.Options) == 12 * 4 + 5 * 8 + 8 + 2 * 4 + 8
    assert ctypes.sizeof(energy.Result) == 16 * 8 + 7 * 8 + 2 * 4
    assert ctypes.sizeof(energy.Timings) == 8 * 8 + 8 * 8
    assert ctypes.sizeof(energy.GibbsMove) == 2 * 4 + 10 * 8


def test_pbc_compute_matches_reference_values():
    # host helper (PeriodicBoundary::update) -- golden values come from the reference harness
    for name in ("ion216_polar", "ion216_triclinic", "ar2"):
        g = util.golden(name)
        R, vol, cut = energy.pbc_compute(np.array(g["basis"]).reshape(3, 3))
        assert vol == g["volume"] and cut == g["cutoff"]
        assert np.array_equal(R.reshape(-1), np.array(g["reciprocal_basis"]))


def test_no_cpu_fallback_without_device():
    if energy.device_count() > 0:
        pytest.skip("a GPU is present")
    atoms, basis, opts = util.load_fixture("ar2")
    with pytest.raises(energy.MpmcError) as ei:
        energy.System(atoms, basis, opts)
    assert ei.value.code == energy.ERR_NO_DEVICE
    assert "no CPU path" in str(ei.value)


def test_product_never_imports_the_oracle():
    pkg = os.path.join(util.ROOT, "mpmcxx_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "mpmc_oracle" not in txt and "import oracle" not in txt and "from oracle" not in txt, f


def test_library_keeps_its_internals_out_of_the_global_namespace():
    """Everything the library defines is either a C-ABI entry point (mpmc_*), mangled inside namespace mpmc, a template instantiation of
    the standard library (weak), or HIP's own registration data -- a host program's `prepare` or `fail` cannot collide with ours.  Also:
    bench.py reaches into oracle/ only inside its CPU-baseline leg."""
    import subprocess

    out = subprocess.run(["nm", "-D", "--defined-only", mbuild.build_library()], stdout=subprocess.PIPE, text=True, check=True).stdout
    strays = []
    for line in out.splitlines():
        parts = line.split()
        kind, name = parts[-2], parts[-1]
        if name.startswith(("mpmc_", "_ZN4mpmc", "_ZNK4mpmc", "_ZTHN4mpmc", "_ZTWN4mpmc", "__hip_")) or kind in ("W", "V", "u"):
            continue
        if "4mpmc" in name:  # kernels and their stubs: templates over mpmc:: types
            continue
        strays.append(line)
    assert not strays, strays
    src = open(os.path.join(util.ROOT, "bench.py")).read()
    head, leg = src.split("def cpu_baseline(", 1)
    leg_body, rest = leg.split("\ndef main(", 1)
    assert "from oracle import" not in head and "from oracle import" not in rest and "import oracle" not in rest


def test_library_reads_one_environment_variable_only():
    """measurement switches travel through mpmc_debug_configure (csrc/context.cpp), not through getenv: the one variable the library
    reads is MPMC_RCCL_LIB, the path of the RCCL it should dlopen (csrc/comm.cpp)."""
    import re

    hits = []
    for dirpath, _, files in os.walk(os.path.join(util.ROOT, "mpmcxx_amd", "csrc")):
        for f in files:
            for m in re.finditer(r'getenv\("([A-Z_0-9]+)"\)', open(os.path.join(dirpath, f)).read()):
                hits.append((f, m.group(1)))
    assert hits == [("comm.cpp", "MPMC_RCCL_LIB")], hits


def _kernel_notes(obj_name):
    """{kernel name: {field: int}} from the gfx950 code object inside a built object file (llvm-objcopy + clang-offload-bundler +
    llvm-readelf --notes: the AMDGPU metadata the runtime itself reads)"""
    import re
    import subprocess
    import tempfile

    llvm = "/opt/rocm/lib/llvm/bin"
    mbuild.build_library()
    obj = os.path.join(os.path.dirname(mbuild.LIB), ".obj", obj_name)
    if not (os.path.exists(obj) and os.path.exists(os.path.join(llvm, "llvm-readelf"))):
        pytest.skip("no object file / no llvm tools here")
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "f.bin"), os.path.join(d, "k.co")
        subprocess.check_call([os.path.join(llvm, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", obj, os.path.join(d, "copy.o")])
        subprocess.check_call([os.path.join(llvm, "clang-offload-bundler"), "--type=o", "--unbundle", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                               f"--input={fat}", f"--output={co}"])
        text = subprocess.check_output([os.path.join(llvm, "llvm-readelf"), "--notes", co], text=True)
    out, cur = {}, None
    for ln in text.splitlines():
        m = re.match(r"\s+\.name:\s+(\S+)", ln)
        if m:
            cur = out.setdefault(m.group(1), {})
        m = re.match(r"\s+\.(sgpr_spill_count|vgpr_spill_count|private_segment_fixed_size|vgpr_count|group_segment_fixed_size):\s+(\d+)", ln)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    return out


def test_hot_kernels_spill_nothing_and_the_contraction_has_two_forms():
    """A spilled SGPR is a v_writelane / v_readlane on the VALU, which is what the two dominant kernels are bound by (round 3: the panel kernel
    lost 2.8 % of the job rate to 34 of them); spilled VGPRs or scratch would be worse.  Orthorhombic instantiations: the production path."""
    panel = _kernel_notes("kernels_panel.hip.o")
    assert len([k for k in panel if "k_dipole_iter_panel" in k]) == 2, list(panel)  # orthorhombic and skewed
    hot = [k for k in panel if "k_dipole_iter_panelILi4ELb1EE" in k]  # <PIPE 4, orthorhombic>: the production instantiation
    assert len(hot) == 1, list(panel)
    assert panel[hot[0]]["sgpr_spill_count"] == 0 and panel[hot[0]]["vgpr_spill_count"] == 0 and panel[hot[0]]["private_segment_fixed_size"] == 0, panel[hot[0]]
    assert panel[hot[0]]["vgpr_count"] <= 128  # four waves per SIMD
    for name, meta in panel.items():
        assert meta["vgpr_spill_count"] == 0 and meta["private_segment_fixed_size"] == 0, (name, meta)
    sweep = _kernel_notes("kernels_pair.hip.o")
    assert any("k_pair_sweepILb1ELb0ELb1E" in k for k in sweep), list(sweep)
    for name, meta in sweep.items():
        assert meta["vgpr_spill_count"] == 0 and meta["private_segment_fixed_size"] == 0, (name, meta)
        assert meta["vgpr_count"] <= 128, (name, meta)
