"""The Silvera-Goldman H2 potential off the GPU: the restatement tests/sg_ref.py against the goldens the reference itself made
(tests/golden/sg.json, gen_box.SG_FIXTURES through oracle/make_golden.py), and the readers."""
import os

import pytest

import sg_ref as R
import util
from mpmcxx_amd import gen_box, pqr

FIXTURES = gen_box.SG_FIXTURES


def golden(name):
    return gen_box.sg_golden(util.GOLDEN, name)


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_matches_reference(name):
    g, r = golden(name), R.restated(name)
    print(name, r, g["rd"], abs(r["rd"] - g["rd"]) / abs(g["rd"]), abs(r["rd"]) / r["mag"])
    assert util.close(r["rd"], g["rd"], util.REL_TOL), (name, r, g["rd"])
    assert g["total"] == g["rd"] and g["es"] == 0 and g["polar"] == 0 and g["lrc_pair"] == 0  # (:46, :115-116: sg() alone)
    # the relative bar is not hiding cancellation: the sum is no small remainder of its terms
    assert abs(r["rd"]) >= 1e-3 * r["mag"], (name, r)
    assert 0 < r["n_terms"] <= g["n_pairs"]


@pytest.mark.parametrize("name", ["h2_64_sg", "h2d2_64_sg_fh_a", "h2_216_sg_tri"])
def test_numpy_form_agrees_with_the_loop(name):
    atoms, basis, opts = R.load(name)
    a, b = R.restated(name), R.for_case(atoms, basis, opts, cutoff=golden(name)["cutoff"], fast=True)
    assert b["n_terms"] == a["n_terms"]
    assert abs(b["rd"] - a["rd"]) <= 1e-13 * a["mag"] and abs(b["mag"] - a["mag"]) <= 1e-13 * a["mag"], (a, b)


def test_ignored_and_skipped_settings_leave_the_reference_unchanged():
    base = golden("h2_64_sg")
    assert golden("h2_64_sg_lrc")["rd"] == base["rd"] and golden("h2_64_sg_polar")["total"] == base["total"]


def test_two_list_orders_differ_in_the_reference():
    a, b = golden("h2d2_64_sg_fh_a"), golden("h2d2_64_sg_fh_b")
    assert abs(a["rd"] - b["rd"]) > 1e-3 * abs(a["rd"]), (a["rd"], b["rd"])
    # ... and the restatement follows each order (the mass of the pair's first atom in the list)
    assert util.close(R.restated("h2d2_64_sg_fh_a")["rd"], a["rd"]) and util.close(R.restated("h2d2_64_sg_fh_b")["rd"], b["rd"])


def test_two_site_box_counts_intramolecular_pairs():
    atoms, _, _ = R.load("h2_2site_sg")
    assert len(util.molecules(atoms)) == 32 and golden("h2_2site_sg")["n_intra"] == 32
    assert golden("h2_2site_sg")["rd"] > 0  # (32 pairs at 2.4 A, on the repulsive wall, outweigh the wells)


def test_python_reader_carries_sg():
    assert "sg" not in pqr.UNSUPPORTED_ON
    for name in FIXTURES:
        _, _, opts = R.load(name)
        assert opts.get("sg"), (name, opts)


def test_python_reader_sg_off(tmp_path):
    inp, _ = gen_box.materialize("h2_64_sg", str(tmp_path))
    text = open(inp).read().replace("sg on", "sg off")
    assert "sg off" in text
    open(inp, "w").write(text)
    assert not pqr.load_case(inp)[2].get("sg")


def test_cpp_reader_carries_sg(tmp_path):
    """include/mpmc_io.hpp reads `sg` into a field of its own and raises no flag for it"""
    import shutil
    import subprocess

    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    inp, _ = gen_box.materialize("h2_64_sg", str(tmp_path))
    src = tmp_path / "reader.cpp"
    src.write_text('#include "mpmc_io.hpp"\n#include <cstdio>\nint main(int, char **v) { mpmc::System s; mpmc::read_input(v[1], s); '
                   'std::printf("%d %llu\\n", s.use_sg, (unsigned long long)(s.unsupported_flags & MPMC_FLAG_USE_SG)); return 0; }\n')
    exe = tmp_path / "reader"
    lib = os.path.join(util.ROOT, "mpmcxx_amd")
    subprocess.check_call([cxx, "-std=c++17", "-I", os.path.join(util.ROOT, "include"), str(src), "-o", str(exe), "-L", lib, "-lmpmc_energy",
                           f"-Wl,-rpath,{lib}"])
    assert subprocess.check_output([str(exe), inp], text=True).split() == ["1", "0"]
