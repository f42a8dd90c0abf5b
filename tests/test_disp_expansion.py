"""CPU side of the disp-expansion term: the numpy restatement against the reference's goldens, the readers, the fixture generator, the
exported entry points and the gfx950 code object of kernels_disp.hip."""
import math
import os

import numpy as np
import pytest

import disp_expansion_ref as D
import util
from mpmcxx_amd import build as mbuild
from mpmcxx_amd import energy, gen_box, pqr
from test_cabi import _kernel_notes

EPS = np.finfo(float).eps
_CACHE = {}


def restated(name):
    if name not in _CACHE:
        atoms, basis, opts = D.load(name)
        _CACHE[name] = D.for_case(atoms, basis, opts)
    return _CACHE[name]


def sum_bound(g, mag):
    """what a sequential sum of the reference's pair terms can differ from any other order of the same terms by (n_pairs eps sum|terms|)"""
    return g["n_pairs"] * EPS * mag


@pytest.mark.parametrize("name", gen_box.DISP_FIXTURES)
def test_restatement_matches_reference_goldens(name):
    g = util.golden(name)
    r = restated(name)
    for k, kg in (("rd", "rd"), ("lj_pairs", "lj_pairs")):
        assert abs(r[k] - g[kg]) <= max(1e-12 * abs(g[kg]), 8 * EPS * r["mag"]), (name, k, r[k], g[kg])
    # the pair LRC is a sum of n (n - 1) / 2 terms of one sign in the reference's order
    lp_mag = abs(g["lrc_pair"])
    assert abs(r["lrc_pair"] - g["lrc_pair"]) <= max(1e-12 * lp_mag, sum_bound(g, lp_mag)), (name, r["lrc_pair"], g["lrc_pair"])
    # the harness prints no disp self LRC (its lrc_self field is lj_lrc_self): rd - lj_pairs - lrc_pair, good to the rounding of those sums
    ls = g["rd"] - g["lj_pairs"] - g["lrc_pair"]
    bound = sum_bound(g, r["mag"] + lp_mag) + 4 * EPS * (abs(g["rd"]) + abs(g["lj_pairs"]) + lp_mag)
    assert abs(r["lrc_self"] - ls) <= max(1e-12 * abs(ls), bound), (name, r["lrc_self"], ls, bound)


def test_two_atom_boxes_closed_form():
    """the 2-atom goldens against the pair formula written out by hand"""
    a, b = gen_box.DISP_SPECIES["A"], gen_box.DISP_SPECIES["B"]
    alpha = 2.0 * a[0] * b[0] / (a[0] + b[0])
    r0 = 0.5 * (a[1] + b[1])
    c = [np.sqrt(a[2 + k] * b[2 + k]) * f / D.UNIT for k, f in enumerate((0.021958709, 0.0061490647, 0.0017219135))]
    for name, r, damp in (("ar2_disp_32", 3.2, False), ("ar2_disp_38", 3.8, True), ("ar2_disp_60", 6.0, True)):
        x = alpha * r
        tt = [1.0 - np.exp(-x) * sum(x ** i / math.factorial(i) for i in range(n + 1)) if damp else 1.0 for n in (6, 8, 10)]
        e = D.REPULSION * np.exp(-alpha * (r - r0)) - sum(tt[k] * c[k] / r ** (6 + 2 * k) for k in range(3))
        g = util.golden(name)
        assert abs(g["lj_pairs"] - e) <= 1e-13 * abs(e), (name, g["lj_pairs"], e)


@pytest.mark.parametrize("name", gen_box.DISP_FIXTURES)
def test_regenerated_boxes_are_the_ones_the_reference_evaluated(name):
    """the goldens keep the reference's results only; the box text is regenerated (gen_box.keep_three_body_golden with DISP_FIXTURES)"""
    atoms, basis, opts = D.load(name)
    g = util.golden(name)
    assert g["fixture"] == name and g["natoms"] == atoms["pos"].shape[0]
    assert np.array_equal(np.asarray(g["basis"], dtype=np.float64).reshape(3, 3), basis)
    assert not os.path.exists(os.path.join(util.GOLDEN, name + ".pqr"))
    assert opts["disp_expansion"] == 1
    # every row carries all coefficient columns (the reference carries a previous row's c6 / c8 / c10 into rows that omit them)
    with open(os.path.join(D.box_dir(), name + ".pqr")) as f:
        rows = [ln.split() for ln in f if ln.startswith("ATOM")]
    assert all(len(t) == 20 for t in rows)
    assert int(g["n_lj_in_cutoff"]) > 0


def test_readers_take_the_keywords_and_columns(tmp_path):
    atoms, basis, opts = D.load("ion216_extrap_disp")
    assert opts["disp_expansion"] == 1 and opts["damp_dispersion"] == 1 and opts["extrapolate_disp_coeffs"] == 1
    assert "schmidt_ff" not in opts
    assert np.sum(atoms["c6"] == 0.0) == 216 // 7 and np.sum(atoms["c8"] == 0.0) == 216 // 11
    assert set(atoms["c10"].tolist()) == {49060.0, 155500.0}
    _, _, opts = D.load("ion216_schmidt_disp")
    assert opts["schmidt_ff"] == 1 and "damp_dispersion" not in opts
    atoms, _, _ = D.load("water64_disp")
    assert sorted(set(atoms["c6"].tolist())) == [0.0, 2.5, 15.0, 285.9]
    # disp_expansion_mbvdw needs vdw(): refused
    inp, _ = gen_box.materialize("ar2_disp_38", str(tmp_path))
    with open(inp, "a") as f:
        f.write("disp_expansion_mbvdw on\n")
    with pytest.raises(NotImplementedError):
        pqr.read_input(inp)
    assert "disp_expansion" not in pqr.UNSUPPORTED_ON and "disp_expansion_mbvdw" in pqr.UNSUPPORTED_ON


@pytest.mark.parametrize("name", util.SMALL)
def test_existing_fixtures_load_without_the_term(name):
    atoms, basis, opts = util.load_fixture(name)
    assert not any(k in opts for k in ("disp_expansion", "damp_dispersion", "extrapolate_disp_coeffs", "schmidt_ff"))
    assert np.all(atoms["c8"] == 0.0) and np.all(atoms["c10"] == 0.0)


def test_disp_fixtures_stay_out_of_the_other_lists():
    others = set(gen_box.SMALL_FIXTURES + gen_box.LARGE_FIXTURES + gen_box.THREE_BODY_FIXTURES + util.SMALL)
    assert not set(gen_box.DISP_FIXTURES) & others


def test_library_exports_the_entry_points():
    L = energy.lib()
    assert hasattr(L, "mpmc_set_disp_expansion") and hasattr(L, "mpmc_disp_expansion")
    hdr = open(os.path.join(os.path.dirname(mbuild.HERE), "include", "mpmc_energy.h")).read()
    assert "#define MPMC_ABI_VERSION 6" in hdr and "#define MPMC_DISP_DAMP 1" in hdr and "#define MPMC_DISP_SCHMIDT 4" in hdr
    assert "kernels_disp.hip" in mbuild.SOURCES


def test_disp_kernels_spill_nothing():
    notes = _kernel_notes("kernels_disp.hip.o")
    full = [k for k in notes if "k_pair_term_sum" in k and "DispTerm" in k]  # (the shared walks of pair_term_walk.h with this file's term)
    delta = [k for k in notes if "k_pair_term_delta" in k and "DispTerm" in k]
    assert len(full) == 4 and len(delta) == 4, list(notes)  # orthorhombic / skewed x damped / undamped
    for name in full + delta:
        meta = notes[name]
        assert meta["sgpr_spill_count"] == 0 and meta["vgpr_spill_count"] == 0 and meta["private_segment_fixed_size"] == 0, (name, meta)
        assert meta["vgpr_count"] <= 128, (name, meta)


def test_cpp_drivers_refuse_the_term(tmp_path):
    """the PI-NVT and Gibbs drivers (include/mpmc_pimc.hpp, mpmc_gibbs.hpp) refuse a System with the term with 4004, before any evaluation"""
    import subprocess

    lib = os.path.dirname(mbuild.LIB)
    mbuild.build_library()
    exe = str(tmp_path / "disp_refusal_check")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-I", os.path.join(util.ROOT, "include"),
                           os.path.join(util.ROOT, "tests", "cpp", "disp_refusal_check.cpp"), "-L", lib, "-lmpmc_energy", f"-Wl,-rpath,{lib}",
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.split("\n")[:2] == ["pimc 4004", "gibbs 4004"], out.stdout
