"""CPU: `polar_wolf` (the Wolf static field) and `polar_palmo` (the Palmo-Krimm correction) through the readers, the facades and the
drivers, and the yardstick of the GPU tests.

The numpy restatement (tests/polar_wolf_ref.py) must reproduce every WOLF_FIXTURES golden that has a Wolf field, which the reference's own
object code computed.  Its distance from them is the margin of every test that uses the restatement as its oracle
(tests/test_gpu_polar_wolf.py: that margin plus the project's 1e-9); test_restatement_reproduces_every_golden prints the table that
profiles/polar_wolf_margin.txt records and holds every figure to MARGIN_LIMIT, so a regenerated golden cannot silently change it.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import util
import polar_wolf_ref as ref
from mpmcxx_amd import build as mbuild
from mpmcxx_amd import gen_box, pqr

MARGIN_LIMIT = 1e-11  # the restatement against the reference: a hundredth of the 1e-9 contract (measured: profiles/polar_wolf_margin.txt)
# the values of the issue's table (reference objects on the CPU), which regenerated goldens must give again
ANCHORS = {
    "ion216_polar_pw_jac": -726.3731974506533, "ion216_polar_pw_gs": -726.3735846332415, "ion216_polar_pw_gsp": -726.3731941823725,
    "ion216_polar_pw_direct": -726.3731942005356, "ion216_polar_pw_gspg": -726.3731941764188,
    "water64_polar_pw_jac": -90604.96377852632, "water64_polar_pw_gs": -89902.60616358115, "water64_polar_pw_gsp": -89907.24279939303,
    "water64_polar_pw_direct": -89907.26778089762, "water64_polar_pw_gspg": -89907.24101616343,
    "ion216_framework_pw_jac": -383.62344887358887, "ion216_framework_pw_gs": -383.623591655547, "ion216_framework_pw_gsp": -383.623446784191,
    "ion216_framework_pw_direct": -383.62344679588773, "ion216_framework_pw_gspg": -383.62344677976733,
    "ion216_triclinic_pw_jac": -2077.7175849741006, "ion216_triclinic_pw_gs": -2077.7116382722656, "ion216_triclinic_pw_gsp": -2077.7150796876504,
    "ion216_triclinic_pw_direct": -2077.7150836062833, "ion216_triclinic_pw_gspg": -2077.715079619494,
    "ion216_polar_pw0_jac": -671.1449134540435,
}


@pytest.fixture(scope="module")
def boxes(tmp_path_factory):
    d = tmp_path_factory.mktemp("wolf")
    return {name: util.load_generated(name, d) for name in gen_box.WOLF_FIXTURES}


def test_goldens_hold_the_anchors_of_the_reference():
    for name, want in ANCHORS.items():
        assert ref.golden(name)["polar"] == want, (name, ref.golden(name)["polar"], want)
    # Jacobi and the direct solve: palmo changes nothing, to the last bit; under polar_ewald the golden is the Ewald one plus palmo
    assert ref.golden("ion216_polar_pw_jacp")["polar"] == ref.golden("ion216_polar_pw_jac")["polar"]
    assert ref.golden("ion216_polar_pw_directp")["polar"] == ref.golden("ion216_polar_pw_direct")["polar"]
    g = ref.golden("ion216_polar_pw_gsp")
    assert g["ef_static"][0].tolist() == [-1.1749003375644862, 1.658605461393826, 0.06743218309108817]
    for b in gen_box.WOLF_BASES:  # sweeps to 1e-7 reach the direct answer
        a, d = ref.golden(f"{b}_pw_gspp"), ref.golden(f"{b}_pw_direct")
        assert abs(a["polar"] - d["polar"]) <= 1e-14 * abs(d["polar"]) and 6 <= a["polar_iterations"] <= 11, (b, a["polar"], d["polar"], a["polar_iterations"])


def test_python_reader_takes_the_keywords(boxes, tmp_path):
    atoms, basis, o = boxes["ion216_polar_pw_gsp"]
    assert o["polar_wolf"] == 1 and o["polar_palmo"] == 1 and o["polar_wolf_alpha"] == 0.13 and o["polar_ewald"] == 0
    _, _, o = boxes["ion216_polar_pw0_jac"]
    assert o["polar_wolf"] == 1 and o["polar_wolf_alpha"] == 0.0 and "polar_palmo" not in o
    _, _, o = util.load_fixture("ion216_polar")  # an input that names none of them loads as before
    assert not any(k.startswith("polar_wolf") or k == "polar_palmo" for k in o)
    inp, _ = gen_box.materialize("ion216_polar_pw_gsp", str(tmp_path))
    txt = open(inp).read()
    syn = tmp_path / "syn.in"
    syn.write_text(txt.replace("polar_wolf_alpha 0.13", "polar_wolf_damp 0.21"))
    assert pqr.read_input(str(syn))["options"]["polar_wolf_alpha"] == 0.21
    for extra in ("polar_wolf_full on", "polar_wolf_alpha_lookup on", "polar_gs_ranked on"):
        bad = tmp_path / "bad.in"
        bad.write_text(txt + extra + "\n")
        with pytest.raises(NotImplementedError):
            pqr.read_input(str(bad))
    ok = tmp_path / "ok.in"
    ok.write_text(txt + "polar_wolf_full off\npolar_wolf_alpha_lookup off\n")
    assert pqr.read_input(str(ok))["options"]["polar_wolf"] == 1
    assert "polar_wolf" not in pqr.UNSUPPORTED_ON and "polar_palmo" not in pqr.UNSUPPORTED_ON


def test_cpp_reader_and_drivers(tmp_path):
    """include/mpmc_io.hpp reads the keywords (and the synonym) without a refusal bit and keeps refusing polar_wolf_full and
    polar_wolf_alpha_lookup; the PI-NVT and Gibbs drivers refuse either option with 4004 before any evaluation"""
    lib = os.path.dirname(mbuild.LIB)
    mbuild.build_library()
    exe = str(tmp_path / "polar_wolf_check")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-I", os.path.join(util.ROOT, "include"),
                           os.path.join(util.ROOT, "tests", "cpp", "polar_wolf_check.cpp"), "-L", lib, "-lmpmc_energy", f"-Wl,-rpath,{lib}",
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    inp, _ = gen_box.materialize("ion216_polar_pw_gsp", str(tmp_path))
    txt = open(inp).read()

    def run(text):
        p = tmp_path / "case.in"
        p.write_text(text)
        out = subprocess.run([exe, str(p)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        return out.stdout.split("\n")

    lines = run(txt)
    assert lines[0] == "read 1 1 0.13 0", lines
    assert lines[1:5] == ["pimc 4004", "gibbs 4004", "pimc 4004", "gibbs 4004"], lines
    assert run(txt.replace("polar_wolf_alpha 0.13", "polar_wolf_damp 0.21"))[0] == "read 1 1 0.20999999999999999 0"
    h = open(os.path.join(util.ROOT, "include", "mpmc_energy.h")).read()
    bit = lambda name: 1 << int(re.search(r"#define\s+" + name + r"\s+\(1ull << (\d+)\)", h).group(1))
    assert (bit("MPMC_FLAG_POLAR_WOLF"), bit("MPMC_FLAG_POLAR_PALMO")) == (1 << 8, 1 << 9)
    assert run(txt + "polar_wolf_full on\n")[0] == f"read 1 1 0.13 {1 << 8}"
    assert run(txt + "polar_wolf_alpha_lookup on\n")[0] == f"read 1 1 0.13 {1 << 8}"
    assert run(txt + "polar_gs_ranked on\n")[0] == f"read 1 1 0.13 {1 << 10}"


def test_header_keeps_abi_6_and_declares_the_entry_points():
    h = open(os.path.join(util.ROOT, "include", "mpmc_energy.h")).read()
    assert re.search(r"#define\s+MPMC_ABI_VERSION\s+6\b", h)
    assert re.search(r"#define\s+MPMC_K_COUNT\s+8\b", h)
    assert re.search(r"int\s+mpmc_set_polar_wolf\s*\(\s*mpmc_ctx\s*\*\s*ctx\s*,\s*int\s+enabled\s*,\s*double\s+polar_wolf_alpha\s*\)\s*;", h)
    assert re.search(r"int\s+mpmc_set_polar_palmo\s*\(\s*mpmc_ctx\s*\*\s*ctx\s*,\s*int\s+enabled\s*\)\s*;", h)
    assert re.search(r"int\s+mpmc_polar_palmo_info\s*\(\s*mpmc_ctx\s*\*\s*ctx\s*,\s*double\s*\*\s*energy_correction\s*,\s*double\s*\*\s*ef_induced_change", h)
    assert "polar_wolf_full" in h and "polar_wolf_alpha_lookup" in h
    assert "kernels_wolf_field.hip" in mbuild.SOURCES
    mbuild.build_library()
    syms = subprocess.run(["nm", "-D", "--defined-only", mbuild.LIB], capture_output=True, text=True, check=True).stdout
    for s in ("mpmc_set_polar_wolf", "mpmc_set_polar_palmo", "mpmc_polar_palmo_info"):
        assert re.search(r"\sT\s+" + s + r"\s", syms), s
    src = util.csrc_text("kernels_pair.hip")  # the fast sweep's field part has no Wolf mode: its template parameters are what they were
    assert "wolf_field" not in src and "WolfFieldParams" not in src


def test_restatement_reproduces_every_golden(boxes, capsys):
    lines = []
    for name, (atoms, basis, o) in boxes.items():
        if o.get("polar_ewald") or np.asarray(atoms["pos"]).shape[0] > 1000:  # (the restatement has the Wolf field only; 4000 atoms: 12000^2 doubles)
            continue
        g = ref.golden(name)
        r = ref.solve(atoms, basis, o)
        sample = np.asarray(g.get("sample_atoms", np.arange(g["natoms"])))
        dev = {}
        # (the reference never writes ef_induced on the direct path: its golden holds zeros there)
        for k in ("ef_static", "mu") + (("ef_induced",) if o["polar_iterative"] else ()):
            want = np.asarray(g[k]).reshape(-1, 3)
            dev[k] = float(np.abs(r[k][sample] - want).max() / np.abs(want).max())
        d_u = abs(r["polarization_energy"] - g["polar"]) / abs(g["polar"])
        lines.append(f"{name:28s} iterations {r['polar_iterations']:3d} correction {r['correction']: .6e}  restatement vs reference: "
                     f"energy {d_u:.2e} ef_static {dev['ef_static']:.2e} mu {dev['mu']:.2e} ef_induced {dev.get('ef_induced', 0.0):.2e}")
        assert r["polar_iterations"] == g["polar_iterations"] and r["iterator_failed"] == g["iterator_failed"], lines[-1]
        assert d_u <= MARGIN_LIMIT and max(dev.values()) <= MARGIN_LIMIT, lines[-1]
        if not (o.get("polar_palmo") and o.get("polar_gs")):
            assert r["correction"] == 0.0 and not np.any(r["ef_induced_change"])
    for b in gen_box.WOLF_BASES:  # the correction itself: golden with palmo minus golden without
        atoms, basis, o = boxes[f"{b}_pw_gsp"]
        want = ref.golden(f"{b}_pw_gsp")["polar"] - ref.golden(f"{b}_pw_gs")["polar"]
        got = ref.solve(atoms, basis, o)["correction"]
        assert abs(got - want) <= 1e-9 * abs(ref.golden(f"{b}_pw_gs")["polar"]), (b, got, want)
    with capsys.disabled():
        print("\n" + "\n".join(lines))
