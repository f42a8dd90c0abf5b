"""CPU: `polar_ewald_full` (the dipole solve with an Ewald-summed induced field) through the readers, the facades and the drivers, and
the yardstick of the GPU tests.

The numpy restatement (tests/polar_ewald_full_ref.py) must reproduce every EWALD_FULL_FIXTURES golden of up to 1000 atoms, which the
reference's own object code computed, within the project's parity margin of 1e-9; test_restatement_reproduces_every_golden prints how far
it is from them (measured: 4e-13 on the energy, 2e-12 on the dipoles, 5e-12 on the induced field at worst).
"""
import os
import re
import subprocess

import numpy as np
import pytest

import util
import polar_ewald_full_ref as ref
from mpmcxx_amd import build as mbuild
from mpmcxx_amd import gen_box, pqr

# the values of the issue's table (reference objects on the CPU), which regenerated goldens must give again
ANCHORS = {"ion216_polar_pef": -808.0459141067123, "ion216_polar_pef_it3": -808.0441504957867, "ion216_polar_pef_prec": -808.0459130398601,
           "water64_polar_pef": -110790.53226198729}
N_REAL_PAIRS = {"ion216_polar_pef": 11544, "water64_polar_pef": 5448}
SMALL = [n for n in gen_box.EWALD_FULL_FIXTURES if not n.startswith("ion4000")]  # (4000 atoms: the restatement's [n, n, 3] arrays)


@pytest.fixture(scope="module")
def boxes(tmp_path_factory):
    d = tmp_path_factory.mktemp("pef")
    return {name: util.load_generated(name, d) for name in SMALL}


@pytest.fixture(scope="module")
def solved(boxes):
    return {name: ref.solve(*boxes[name]) for name in SMALL}


def test_goldens_hold_the_anchors_of_the_reference():
    for name, want in ANCHORS.items():
        assert ref.golden(name)["polar"] == want, (name, ref.golden(name)["polar"], want)
    # polar_ewald changes nothing under the term: the static field is recip_term + real_term either way
    a, b = ref.golden("ion216_polar_nopbc_pef"), ref.golden("ion216_polar_pef")
    for k in ("total", "rd", "es", "polar"):
        assert a[k] == b[k], (k, a[k], b[k])
    for k in ("ef_static", "mu", "ef_induced"):
        assert np.array_equal(a[k], b[k]), k
    for name in gen_box.EWALD_FULL_FIXTURES:
        g = ref.golden(name)
        assert g["polar_iterations"] == 0 and g["dipole_rrms"] == 0 and g["iterator_failed"] == 0, name  # (the reference never writes them on this path)
        assert g["ef_static"].shape == (len(g["sample_atoms"]), 3), name
    assert len(ref.golden("ion4000_polar_pef")["sample_atoms"]) == 250


def test_es_and_rd_are_those_of_the_base_fixture():
    """the term touches the polarization energy alone: every other component of a _pef golden has the bits of its base box's golden (the
    bases that exist only here -- ion4000_polar, pol2_eq, pol2_gt -- have no golden of their own)"""
    seen = 0
    for name in gen_box.EWALD_FULL_FIXTURES:
        base = name.partition("_pef")[0]
        if not os.path.exists(os.path.join(util.GOLDEN, f"{base}.json")):
            assert base in ("ion4000_polar", "pol2_eq", "pol2_gt"), base
            continue
        g, b = ref.golden(name), util.golden(base)
        for k in ("rd", "es", "es_real", "es_recip", "es_self", "lj_pairs", "lrc_pair", "lrc_self", "n_lj_in_cutoff", "n_es_in_cutoff"):
            assert g[k] == b[k], (name, k, g[k], b[k])
        assert g["polar"] != b["polar"], name
        seen += 1
    assert seen == 11


def test_restatement_reproduces_every_golden(boxes, solved, capsys):
    lines = []
    for name in SMALL:
        g, r = ref.golden(name), solved[name]
        sample = np.asarray(g["sample_atoms"])
        dev = {k: float(np.abs(r[k][sample] - g[k]).max() / np.abs(g[k]).max()) for k in ("ef_static", "mu", "ef_induced")}
        d_u = abs(r["polarization_energy"] - g["polar"]) / abs(g["polar"])
        lines.append(f"{name:26s} passes {r['passes']:3d} pairs {r['n_real_pairs']:7d}  restatement vs reference: energy {d_u:.2e} "
                     f"ef_static {dev['ef_static']:.2e} mu {dev['mu']:.2e} ef_induced {dev['ef_induced']:.2e}")
        assert r["iterator_failed"] == 0, lines[-1]
        assert d_u <= 1e-9 and max(dev.values()) <= 1e-9, lines[-1]
        o = boxes[name][2]
        if not o.get("polar_precision"):
            assert r["passes"] == o["polar_max_iter"] + 1, lines[-1]
        if name in N_REAL_PAIRS:
            assert r["n_real_pairs"] == N_REAL_PAIRS[name], lines[-1]
    assert solved["ion216_polar_pef_prec"]["passes"] == 9  # (one pass more or fewer would move the dipoles by about the precision, 1e-7 of the largest: the parity above pins the count)
    assert solved["pol2_eq_pef"]["n_real_pairs"] == 1 and solved["pol2_gt_pef"]["n_real_pairs"] == 1
    with capsys.disabled():
        print("\n" + "\n".join(lines))


def test_vector_weight_moves_the_energy(boxes):
    """the intended weight k_p instead of the reference's k_z: the issue's figure for ion216_polar"""
    u = ref.solve(*boxes["ion216_polar_pef"], vector_weight=True)["polarization_energy"]
    assert abs(u - (-785.44)) < 0.005, u


def test_no_pair_sits_at_the_cutoff_except_in_pol2_eq(boxes):
    """a pair within 1e-9 relative of R could fall on either side of the predicate in another arithmetic: only pol2_eq has one, exactly at R"""
    for name, (atoms, basis, o) in boxes.items():
        bx = ref.Box(atoms, basis, o)
        r = bx.r[np.triu_indices(bx.n, 1)]
        near = np.abs(r - bx.cutoff) <= 1e-9 * bx.cutoff
        if name == "pol2_eq_pef":
            assert near.sum() == 1 and r[near][0] == bx.cutoff == 5.0
        else:
            assert not near.any(), (name, r[near])


def test_python_reader_takes_the_keyword(boxes, tmp_path):
    _, _, o = boxes["ion216_polar_pef"]
    assert o["polar_ewald_full"] == 1
    _, _, o = util.load_fixture("ion216_polar")  # an input that does not name it loads as before
    assert "polar_ewald_full" not in o
    assert "polar_ewald_full" not in pqr.UNSUPPORTED_ON
    inp, _ = gen_box.materialize("ion216_polar_pef", str(tmp_path))
    off = tmp_path / "off.in"
    off.write_text(open(inp).read().replace("polar_ewald_full on", "polar_ewald_full off"))
    assert pqr.read_input(str(off))["options"]["polar_ewald_full"] == 0


def build_check_program(tmp_path):
    lib = os.path.dirname(mbuild.LIB)
    mbuild.build_library()
    exe = str(tmp_path / "polar_ewald_full_check")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-I", os.path.join(util.ROOT, "include"),
                           os.path.join(util.ROOT, "tests", "cpp", "polar_ewald_full_check.cpp"), "-L", lib, "-lmpmc_energy", f"-Wl,-rpath,{lib}",
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_cpp_reader_and_drivers(tmp_path):
    """include/mpmc_io.hpp records the keyword in the facade and still sets the flag bit (the facade clears it when it calls the setter);
    the PI-NVT and Gibbs drivers refuse such a System with 4004 before any evaluation"""
    exe = build_check_program(tmp_path)
    inp, _ = gen_box.materialize("ion216_polar_pef", str(tmp_path))
    txt = open(inp).read()

    def run(text):
        p = tmp_path / "case.in"
        p.write_text(text)
        out = subprocess.run([exe, str(p)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        return out.stdout.split("\n")

    lines = run(txt)
    assert lines[0] == "read 1 0 1 0", lines
    assert lines[1:3] == ["pimc 4004", "gibbs 4004"], lines
    assert run(txt.replace("polar_ewald_full on", "polar_ewald_full off"))[0] == "read 0 0 0 0"
    assert run(txt.replace("polar_ewald_full on\n", ""))[0] == "read 0 0 0 0"
    assert run(txt + "polar_wolf_full on\n")[0] == f"read 1 0 1 {1 << 8}"


def test_header_keeps_abi_6_and_declares_the_entry_points():
    h = open(os.path.join(util.ROOT, "include", "mpmc_energy.h")).read()
    assert re.search(r"#define\s+MPMC_ABI_VERSION\s+6\b", h)
    assert re.search(r"#define\s+MPMC_K_COUNT\s+8\b", h)
    assert re.search(r"#define\s+MPMC_PEF_VECTOR_KWEIGHT\s+1\b", h)
    assert re.search(r"#define\s+MPMC_FLAG_POLAR_EWALD_FULL\s+\(1ull << 7\)", h)
    assert re.search(r"int\s+mpmc_set_polar_ewald_full\s*\(\s*mpmc_ctx\s*\*\s*ctx\s*,\s*int\s+enabled\s*,\s*int\s+flags\s*\)\s*;", h)
    assert re.search(r"typedef\s+struct\s+mpmc_ewald_full_info\s*\{[^}]*int32_t\s+passes;[^}]*int32_t\s+n_k;[^}]*int64_t\s+n_real_pairs;[^}]*int64_t\s+store_bytes;[^}]*\}\s*"
                     r"mpmc_ewald_full_info\s*;", h)
    assert re.search(r"int\s+mpmc_polar_ewald_full_info\s*\(\s*mpmc_ctx\s*\*\s*ctx\s*,\s*mpmc_ewald_full_info\s*\*\s*out\s*\)\s*;", h)


def test_kernels_compile_for_gfx950_and_the_library_exports_the_entry_points():
    assert "kernels_ewald_full.hip" in mbuild.SOURCES
    assert "--offload-arch=gfx950" in mbuild.CFLAGS
    mbuild.build_library()
    assert os.path.getmtime(mbuild.LIB) >= os.path.getmtime(os.path.join(mbuild.CSRC, "kernels_ewald_full.hip"))
    syms = subprocess.run(["nm", "-D", "--defined-only", mbuild.LIB], capture_output=True, text=True, check=True).stdout
    for s in ("mpmc_set_polar_ewald_full", "mpmc_polar_ewald_full_info"):
        assert re.search(r"\sT\s+" + s + r"\s", syms), s
    # the device code of the five kernels is in the library's gfx950 code object
    blob = open(mbuild.LIB, "rb").read()
    for k in (b"k_pef_fill", b"k_pef_phases", b"k_pef_contract", b"k_pef_sf", b"k_pef_finish"):
        assert k in blob, k
