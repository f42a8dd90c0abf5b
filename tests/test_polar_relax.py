"""CPU: `polar_sor`, `polar_esor` and `polar_zodid` through the readers and the header, the host side of the blend, and the yardstick of
the GPU tests.

The numpy restatement (tests/polar_relax_ref.py) must reproduce every RELAX_FIXTURES golden, which the reference's own object code
computed: energy, iterations, failure flag, rrms, mu and ef_induced.  test_restatement_reproduces_every_golden prints how far it is from
each; WORST holds the largest deviation it reaches per quantity and the assertion allows ten times that.
"""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import util
import polar_relax_ref as ref
from mpmcxx_amd import build as mbuild
from mpmcxx_amd import gen_box, pqr

# the restatement against the reference over all 32 fixtures, as measured (relative to the largest component of each array; rrms relative
# to the golden's): ef_static 2.7e-15, mu 8.5e-14, ef_induced 7.0e-13 (both under polar_ewald_full: sums over 1400 k vectors in another
# order), energy 8.0e-14, rrms 2.3e-10 (water64_polar_rx_sorp: rrms = 2.2e-8 is a difference of consecutive iterates that agree to 2e-15)
WORST = {"ef_static": 2.7e-15, "mu": 8.5e-14, "ef_induced": 7.0e-13, "energy": 8.0e-14, "rrms": 2.3e-10}
# the values of the issue (reference objects on the CPU), which regenerated goldens must give again
ANCHORS = {"ion216_polar_rx_zodid": -789.1871449258084, "ion216_polar_rx_zodidg": -812.8627592735826}


@pytest.fixture(scope="module")
def boxes(tmp_path_factory):
    d = tmp_path_factory.mktemp("relax")
    return {name: util.load_generated(name, d) for name in gen_box.RELAX_FIXTURES}


def test_goldens_hold_the_anchors_of_the_reference():
    for name, want in ANCHORS.items():
        assert ref.golden(name)["polar"] == want, (name, ref.golden(name)["polar"], want)
    z = ref.golden("ion216_polar_rx_zodid")
    assert z["polar_iterations"] == 0 and z["dipole_rrms"] == 0.0 and z["iterator_failed"] == 0 and not np.any(z["ef_induced"])
    for v in ("zodidsor", "zodidpalmo"):  # no pre-scale under a scheme; Palmo-Krimm adds exactly 0
        g = ref.golden(f"ion216_polar_rx_{v}")
        assert g["polar"] == z["polar"] and np.array_equal(g["mu"], z["mu"]), v
    f = ref.golden("ion216_polar_rx_sorfail")  # diverges: 128 iterations, mu = alpha E0 without gamma
    assert f["polar_iterations"] == 128 and f["iterator_failed"] == 1 and f["polar"] == z["polar"] and 5.0 < f["dipole_rrms"] < 5.2
    # zodid changes nothing under ewald_full: the same bits as the ewald_full golden of the box
    from polar_ewald_full_ref import golden as pef_golden
    assert ref.golden("ion216_polar_rx_pefzodid")["polar"] == pef_golden("ion216_polar_pef")["polar"]
    # strong coupling: SOR and ESOR after 10 iterations differ by more than 1e-4 on the water box
    a, b = ref.golden("water64_polar_rx_sor08")["polar"], ref.golden("water64_polar_rx_esor06")["polar"]
    assert abs(a - b) > 1e-4 * abs(a)
    assert len(gen_box.RELAX_FIXTURES) == len(set(gen_box.RELAX_FIXTURES)) == 32


def test_restatement_reproduces_every_golden(boxes, capsys):
    lines, worst = [], {}
    for name, (atoms, basis, o) in boxes.items():
        g = ref.golden(name)
        r = ref.solve(atoms, basis, o)
        sample = np.asarray(g["sample_atoms"])
        dev = {}
        for k in ("ef_static", "mu", "ef_induced"):
            want = np.asarray(g[k]).reshape(-1, 3)
            scale = np.abs(want).max()
            dev[k] = float(np.abs(r[k][sample] - want).max() / scale) if scale > 0 else float(np.abs(r[k][sample]).max())
        dev["energy"] = abs(r["polarization_energy"] - g["polar"]) / abs(g["polar"])
        rr = g["dipole_rrms"]
        dev["rrms"] = abs(r["dipole_rrms"] - rr) / abs(rr) if rr else abs(r["dipole_rrms"])
        lines.append(f"{name:30s} iterations {r['polar_iterations']:3d} failed {r['iterator_failed']} restatement vs reference: "
                     + " ".join(f"{k} {v:.1e}" for k, v in dev.items()))
        assert r["polar_iterations"] == g["polar_iterations"] and r["iterator_failed"] == g["iterator_failed"], lines[-1]
        for k, v in dev.items():
            worst[k] = max(worst.get(k, 0.0), v)
            assert v <= 10.0 * WORST[k], lines[-1]
        if "zodid" in name and "pef" not in name:
            assert r["contractions"] == 0 and r["correction"] == 0.0
    with capsys.disabled():
        print("\n" + "\n".join(lines) + "\nworst: " + " ".join(f"{k} {v:.1e}" for k, v in worst.items()))


def test_sor_with_gamma_one_is_the_plain_solve(boxes):
    atoms, basis, o = boxes["ion216_polar_rx_sor08"]
    plain = {k: v for k, v in o.items() if k != "polar_sor"}
    a, b = ref.solve(atoms, basis, dict(o, polar_gamma=1.0)), ref.solve(atoms, basis, dict(plain, polar_gamma=1.0))
    assert a["polarization_energy"] == b["polarization_energy"] and np.array_equal(a["mu"], b["mu"])


def _compile_host(tmp_path, name, extra):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", "-I", os.path.join(util.ROOT, "mpmcxx_amd", "csrc"),
                           os.path.join(util.ROOT, "tests", "cpp", "polar_relax_host.cpp"), "-o", exe] + extra)
    return exe


def test_host_blend_and_weights_match_the_restatement(tmp_path):
    """the MPMC_HD blend and the host's weights, as the kernels get them, against the restatement's expressions: equal to the last bit
    (the library is built with -ffp-contract=off, and so is this program); once more under the address and undefined-behaviour sanitizers"""
    rng = np.random.default_rng(11)
    cases = [(s, g, it, float(nm), float(om)) for s in (0, 1, 2) for g in (0.0, 0.6, 0.8, 1.0, 1.2, 2.5) for it in (1, 2, 9, 127)
             for nm, om in rng.normal(size=(2, 2))]
    text = "".join(f"{s} {g!r} {it} {nm!r} {om!r}\n" for s, g, it, nm, om in cases)
    for name, extra in (("relax_host", []), ("relax_host_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])):
        out = subprocess.run([_compile_host(tmp_path, name, extra)], input=text, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and not out.stderr, out.stderr
        rows = [[float(x) for x in line.split()] for line in out.stdout.strip().split("\n")]
        assert len(rows) == len(cases)
        for (s, g, it, nm, om), (wn, wo, bl) in zip(cases, rows):
            o = {"polar_gamma": g, "polar_sor": s == 1, "polar_esor": s == 2}
            w = ref.weights(o, it)
            assert (wn, wo) == w and bl == ref.blend(w, nm, om), (s, g, it, nm, om, wn, wo, bl)
    assert ref.weights({"polar_gamma": 0.6, "polar_esor": 1}, 3) == (1.0 - math.exp(-0.6 * 3), math.exp(-0.6 * 3))


def test_python_reader_takes_the_keywords(boxes, tmp_path):
    _, _, o = boxes["ion216_polar_rx_esor06"]
    assert o["polar_esor"] == 1 and o["polar_gamma"] == 0.6 and "polar_sor" not in o and "polar_zodid" not in o
    _, _, o = boxes["ion216_polar_rx_zodidsor"]
    assert o["polar_sor"] == 1 and o["polar_zodid"] == 1 and o["polar_gamma"] == 1.03
    _, _, o = util.load_fixture("ion216_polar")  # an input that names none of them loads as before
    assert not any(k in o for k in ("polar_sor", "polar_esor", "polar_zodid"))
    assert not any(k in pqr.UNSUPPORTED_ON for k in ("polar_sor", "polar_esor", "polar_zodid")) and "polar_gs_ranked" in pqr.UNSUPPORTED_ON
    inp, _ = gen_box.materialize("ion216_polar_rx_sor08", str(tmp_path))
    txt = open(inp).read()
    both = tmp_path / "both.in"
    both.write_text(txt + "polar_esor on\n")
    with pytest.raises(ValueError):
        pqr.read_input(str(both))
    ranked = tmp_path / "ranked.in"
    ranked.write_text(txt + "polar_gs_ranked on\n")
    with pytest.raises(NotImplementedError):
        pqr.read_input(str(ranked))
    from mpmcxx_amd import energy
    assert energy.polar_relax_of({"polar_sor": 1}) == (1, False) and energy.polar_relax_of({"polar_esor": 1, "polar_zodid": 1}) == (2, True)
    with pytest.raises(ValueError):
        energy.polar_relax_of({"polar_sor": 1, "polar_esor": 1})


def test_cpp_reader_takes_the_keywords(tmp_path):
    """include/mpmc_io.hpp reads the keywords into fields with no refusal bit, refuses both schemes together and zodid with
    polar_iterative off (3000), and keeps the bit of polar_gs_ranked"""
    lib = os.path.dirname(mbuild.LIB)
    mbuild.build_library()
    exe = str(tmp_path / "polar_relax_check")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-I", os.path.join(util.ROOT, "include"),
                           os.path.join(util.ROOT, "tests", "cpp", "polar_relax_check.cpp"), "-L", lib, "-lmpmc_energy", f"-Wl,-rpath,{lib}",
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    inp, _ = gen_box.materialize("ion216_polar_rx_sor08", str(tmp_path))
    txt = open(inp).read()

    def run(text):
        p = tmp_path / "case.in"
        p.write_text(text)
        out = subprocess.run([exe, str(p)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        return out.stdout.strip()

    assert run(txt) == "read 1 0 0 0.80000000000000004 0"
    assert run(txt.replace("polar_sor on", "polar_esor on") + "polar_zodid on\n") == "read 0 1 1 0.80000000000000004 0"
    assert run(txt + "polar_esor on\n") == "read thrown 3000"
    assert run(txt.replace("polar_iterative on", "polar_iterative off") + "polar_zodid on\n") == "read thrown 3000"
    assert run(txt + "polar_gs_ranked on\n") == f"read 1 0 0 0.80000000000000004 {1 << 10}"


def test_header_keeps_abi_6_and_declares_the_entry_points():
    h = open(os.path.join(util.ROOT, "include", "mpmc_energy.h")).read()
    assert re.search(r"#define\s+MPMC_ABI_VERSION\s+6\b", h)
    assert re.search(r"#define\s+MPMC_K_COUNT\s+8\b", h)
    assert re.search(r"int\s+mpmc_set_polar_relax\s*\(\s*mpmc_ctx\s*\*\s*ctx\s*,\s*int\s+scheme\s*,\s*int\s+zodid\s*\)\s*;", h)
    assert re.search(r"int\s+mpmc_polar_relax_info\s*\(\s*mpmc_ctx\s*\*\s*ctx\s*,\s*mpmc_relax_info\s*\*\s*out\s*\)\s*;", h)
    for name, value in (("NONE", 0), ("SOR", 1), ("ESOR", 2)):
        assert re.search(r"#define\s+MPMC_POLAR_RELAX_" + name + r"\s+" + str(value) + r"\b", h)
    bit = lambda name: 1 << int(re.search(r"#define\s+" + name + r"\s+\(1ull << (\d+)\)", h).group(1))
    assert (bit("MPMC_FLAG_POLAR_SOR"), bit("MPMC_FLAG_POLAR_ZODID"), bit("MPMC_FLAG_POLAR_GS_RANKED")) == (1 << 11, 1 << 12, 1 << 10)
    assert "polar_gs_ranked" in h
    mbuild.build_library()
    syms = subprocess.run(["nm", "-D", "--defined-only", mbuild.LIB], capture_output=True, text=True, check=True).stdout
    for s in ("mpmc_set_polar_relax", "mpmc_polar_relax_info"):
        assert re.search(r"\sT\s+" + s + r"\s", syms), s


def test_library_holds_the_relaxed_kernel_instantiations():
    """the blend is a compile-time variant: kernels of their own next to the plain ones, which keep their names"""
    mbuild.build_library()
    blob = open(mbuild.LIB, "rb").read()
    for k in (b"k_dipole_update_relax", b"k_dipole_update_panel_relax", b"k_pef_finish_relax", b"k_gs_blend"):
        assert k in blob, k
    for k in (b"k_dipole_update", b"k_dipole_update_panel", b"k_pef_finish", b"k_gs_finish"):
        assert re.search(re.escape(k) + rb"(?![a-z_])", blob), k
