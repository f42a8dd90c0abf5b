"""CPU side of `rd_crystal on` (the lattice-summed Lennard-Jones): the numpy restatement against the reference's goldens, the fixtures,
the readers, the header and the gfx950 code object of kernels_crystal.hip."""
import os
import re
import subprocess

import numpy as np
import pytest

import rd_crystal_ref as R
import util
from mpmcxx_amd import build as mbuild
from mpmcxx_amd import energy, gen_box, pqr
from test_cabi import _kernel_notes

EPS = np.finfo(float).eps
SMALL = [n for n in gen_box.RD_CRYSTAL_FIXTURES if not n.startswith("ion4000")]  # (the 4000-atom box is a golden for the GPU only)
# image-term counts of the two-atom boxes, orders 1 / 2 / 3 (at x = 5.0 and order 2 one image lies exactly at the cutoff 15 A and is kept)
AR2_TERMS = {"eq": (1, 19, 69), "gt": (0, 14, 64), "lt": (1, 15, 65)}


def golden(name):
    return gen_box.rd_crystal_golden(util.GOLDEN, name)


@pytest.mark.parametrize("name", SMALL)
def test_restatement_matches_reference_goldens(name):
    """rd within 1e-9 relative (the project's parity margin), lj_pairs within 1e-12 of the summed magnitudes of its terms (measured: 1.7e-13
    and 1.1e-14 at worst)"""
    g, r = golden(name), R.restated(name)
    assert abs(r["rd"] - g["rd"]) <= 1e-9 * abs(g["rd"]), (name, r["rd"], g["rd"])
    assert abs(r["lj_pairs"] - g["lj_pairs"]) <= 1e-12 * r["mag"], (name, r["lj_pairs"], g["lj_pairs"], r["mag"])
    assert abs(r["lrc_pair"] - g["lrc_pair"]) <= 1e-9 * abs(g["lrc_pair"]), (name, r["lrc_pair"], g["lrc_pair"])
    # the harness's own lrc_self is taken at the box cutoff: crystal_self + lrc_self against rd - lj_pairs - lrc_pair, good to the rounding
    # of those sums (n_pairs eps of the summed magnitudes, plus the subtraction's own)
    rest = g["rd"] - g["lj_pairs"] - g["lrc_pair"]
    bound = g["n_pairs"] * EPS * (r["mag"] + abs(g["lrc_pair"])) + 4 * EPS * (abs(g["rd"]) + abs(g["lj_pairs"]) + abs(g["lrc_pair"]))
    assert abs((r["crystal_self"] + r["lrc_self"]) - rest) <= max(1e-12 * abs(rest), bound), (name, r["crystal_self"], r["lrc_self"], rest, bound)
    o = R.order_of(R.load(name)[2])
    assert r["n_images"] == (2 * o - 1) ** 3 and r["cutoff"] == 2.0 * g["cutoff"] * (o - 0.5)


def test_two_atom_boxes_reproduce_the_recorded_values():
    """the reference's rd of the two Ar atoms in the 10 A cell, and the image-term counts of the restatement"""
    want = {"eq": (-115.6124102452959, -98.08007264059704, -96.92312821909265), "gt": (-72.5829438316864, -97.75229261448634, -96.9078333193216)}
    for tag, terms in AR2_TERMS.items():
        for o in (1, 2, 3):
            name = f"ar2_{tag}_rc{o}"
            if tag in want:
                assert golden(name)["rd"] == want[tag][o - 1], name
            assert R.restated(name)["n_image_terms"] == terms[o - 1], name


@pytest.mark.parametrize("name", SMALL)
def test_no_image_distance_sits_on_the_cutoff(name):
    """except in the deliberate exact-cutoff boxes no image distance lies within 1e-9 relative of the cutoff: the counts are meaningful"""
    gap = R.restated(name)["gap"]
    if name.startswith("ar2_eq"):  # (x = 5.0: an image at exactly 5, 15 and 25 A, the cutoffs of orders 1, 2 and 3)
        assert gap == 0.0, (name, gap)
    else:
        assert gap > 1e-9, (name, gap)


def test_shifted_box_is_the_wrapped_box_moved_by_lattice_vectors():
    a, basis, _ = R.load("water64_shift_rc2")
    b, _, _ = R.load("water64_polar_rc2")
    k = (a["pos"] - b["pos"]) / basis[0, 0]
    assert np.allclose(k, np.rint(k), atol=1e-6) and np.abs(np.rint(k)).max() == 1
    for lo, hi in util.molecules(a):
        assert np.all(np.rint(k[lo:hi]) == np.rint(k[lo])), lo
    # the term reads the raw positions: the reference's rd differs, its electrostatics only in the last digits
    gs, gw = golden("water64_shift_rc2"), golden("water64_polar_rc2")
    assert abs(gs["rd"] - gw["rd"]) > 1e-3 * abs(gw["rd"]) and abs(gs["es"] - gw["es"]) <= 1e-12 * abs(gw["es"])


@pytest.mark.parametrize("name", gen_box.RD_CRYSTAL_FIXTURES)
def test_regenerated_boxes_are_the_ones_the_reference_evaluated(name):
    g = golden(name)
    rows, basis, opts = gen_box.fixture(name)
    assert g["fixture"] == name and g["natoms"] == len(rows)
    assert np.array_equal(np.asarray(g["basis"], dtype=np.float64).reshape(3, 3), np.asarray(basis, dtype=np.float64))
    assert opts["rd_crystal"] == "on" and int(opts["rd_crystal_order"]) == int(name.rsplit("_rc", 1)[1])
    assert not os.path.exists(os.path.join(util.GOLDEN, name + ".pqr")) and not os.path.exists(os.path.join(util.GOLDEN, name + ".json"))
    assert not any(isinstance(v, list) and k not in ("basis", "reciprocal_basis") for k, v in g.items())  # scalars only


def test_terms_other_than_rd_are_the_plain_box_s():
    """es and polar of the reference are bit-identical with the term on and off"""
    for name, plain in (("water64_polar_rc2", "water64_polar"), ("ion216_triclinic_rc2", "ion216_triclinic"), ("ion1000_polar_rc2", "ion1000_polar"),
                        ("ion216_polar_rc1", "ion216_polar"), ("water64_fh2_rc2", "water64_fh2")):
        g, p = golden(name), util.golden(plain)
        for k in ("es", "polar", "es_real", "es_recip", "es_self", "n_lj_in_cutoff", "n_rd_excluded"):
            assert g[k] == p[k], (name, k)
        assert g["rd"] != p["rd"]


def test_readers_take_the_keywords(tmp_path):
    """pqr.read_input yields the two options, only when the input names them"""
    _, _, opts = R.load("water64_polar_rc3")
    assert opts["rd_crystal"] == 1 and opts["rd_crystal_order"] == 3
    _, _, o = util.load_fixture("ion216_polar")
    assert "rd_crystal" not in o and "rd_crystal_order" not in o
    assert "rd_crystal" not in pqr.UNSUPPORTED_ON and "cavity_autoreject" in pqr.UNSUPPORTED_ON
    inp, _ = gen_box.materialize("lj64_rc2", str(tmp_path))
    with open(inp, "a") as f:
        f.write("cavity_autoreject on\n")
    with pytest.raises(NotImplementedError):
        pqr.read_input(inp)


def test_cpp_reader_records_the_term_and_keeps_the_flag(tmp_path):
    """mpmc::read_input sets the facade's two fields and still sets MPMC_FLAG_RD_CRYSTAL for the keyword"""
    lib = os.path.dirname(mbuild.LIB)
    mbuild.build_library()
    exe = str(tmp_path / "rd_crystal_check")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-I", os.path.join(util.ROOT, "include"),
                           os.path.join(util.ROOT, "tests", "cpp", "rd_crystal_check.cpp"), "-L", lib, "-lmpmc_energy", f"-Wl,-rpath,{lib}",
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    inp, _ = gen_box.materialize("water64_polar_rc3", str(tmp_path))
    txt = open(inp).read()

    def run(text):
        p = tmp_path / "case.in"
        p.write_text(text)
        out = subprocess.run([exe, str(p)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        return out.stdout.split("\n")[0]

    assert run(txt) == "read 1 3 1 4"
    assert run(txt.replace("rd_crystal on", "rd_crystal off")) == "read 0 3 0 0"
    assert run(txt + "spectre on\n") == "read 1 3 1 12"
    plain, _ = gen_box.materialize("water64_polar", str(tmp_path))
    assert run(open(plain).read()) == "read 0 0 0 0"


def test_header_keeps_abi_6_and_declares_the_entry_points():
    h = open(os.path.join(util.ROOT, "include", "mpmc_energy.h")).read()
    assert "#define MPMC_ABI_VERSION 6" in h and "#define MPMC_RD_CRYSTAL_MAX_ORDER 8" in h
    assert re.search(r"int mpmc_set_rd_crystal\(mpmc_ctx \*ctx, int enabled, int order\);", h)
    assert re.search(r"int mpmc_rd_crystal_info\(mpmc_ctx \*ctx, struct mpmc_rd_crystal_info \*out\);", h)
    assert re.search(r"#define\s+MPMC_FLAG_RD_CRYSTAL\s+\(1ull << 2\)", h)
    assert "disp_expansion ignores rd_crystal" in h
    assert "#define MPMC_K_COUNT 8" in h and len(energy.Timings().ms) == 8
    L = energy.lib()
    assert hasattr(L, "mpmc_set_rd_crystal") and hasattr(L, "mpmc_rd_crystal_info")
    assert "kernels_crystal.hip" in mbuild.SOURCES


def test_rd_crystal_fixtures_stay_out_of_the_other_lists():
    others = set(gen_box.SMALL_FIXTURES + gen_box.LARGE_FIXTURES + gen_box.THREE_BODY_FIXTURES + gen_box.DISP_FIXTURES + gen_box.WOLF_FIXTURES
                 + gen_box.DIRECT_FIXTURES + util.SMALL)
    assert not set(gen_box.RD_CRYSTAL_FIXTURES) & others


def test_crystal_kernels_need_no_scratch():
    notes = _kernel_notes("kernels_crystal.hip.o")
    full = [k for k in notes if "k_pair_term_sum" in k and "CrystalTerm" in k]  # (the shared walks of pair_term_walk.h with this file's term)
    delta = [k for k in notes if "k_pair_term_delta" in k and "CrystalTerm" in k]
    assert len(full) == 2 and len(delta) == 2, list(notes)  # orthorhombic / skewed
    for name in full + delta:
        meta = notes[name]
        assert meta["vgpr_spill_count"] == 0 and meta["private_segment_fixed_size"] == 0, (name, meta)
        assert meta["vgpr_count"] <= 128, (name, meta)
