"""CPU side of the Axilrod-Teller three-body term: the numpy restatement against the reference's goldens, the readers, the fixture
generator, the exported entry points and the gfx950 code object of kernels_three_body.hip."""
import filecmp
import os

import numpy as np
import pytest

import three_body_ref as T
import util
from mpmcxx_amd import build as mbuild
from mpmcxx_amd import energy, gen_box, pqr
from test_cabi import _kernel_notes


def _ref_e3(g):
    return g["total"] - g["rd"] - g["es"] - g["polar"]


@pytest.mark.parametrize("name", gen_box.THREE_BODY_FIXTURES)
def test_restatement_matches_reference_goldens(name):
    atoms, basis, opts = T.load(name)
    g = util.golden(name)
    e3 = _ref_e3(g)
    # what the subtraction leaves: a few ulp of the four terms that were subtracted
    bound = 8 * np.finfo(float).eps * (abs(g["total"]) + abs(g["rd"]) + abs(g["es"]) + abs(g["polar"]))
    ours = T.for_case(atoms, basis, opts)
    assert abs(ours - e3) <= max(1e-12 * abs(e3), bound), (name, ours, e3)
    assert abs(e3) >= 1e-3 * abs(g["total"]), (name, e3, g["total"])  # the term is visible in the total


@pytest.mark.parametrize("name", gen_box.THREE_BODY_FIXTURES)
def test_regenerated_boxes_are_the_ones_the_reference_evaluated(name):
    """the goldens keep the reference's results only; the box text is regenerated (gen_box.keep_three_body_golden)"""
    atoms, basis, opts = T.load(name)
    g = util.golden(name)
    assert g["fixture"] == name and g["natoms"] == atoms["pos"].shape[0]
    assert np.array_equal(np.asarray(g["basis"], dtype=np.float64).reshape(3, 3), basis)
    assert not os.path.exists(os.path.join(util.GOLDEN, name + ".pqr"))


def test_equilateral_triangle_closed_form():
    atoms, basis, opts = T.load("ar3_at")
    closed = 518.3 * T.UNIT * (1.0 + 3.0 / 8.0) / 18.0 ** 4.5
    assert abs(T.for_case(atoms, basis, opts) - closed) <= 1e-13 * closed
    assert abs(_ref_e3(util.golden("ar3_at")) - closed) <= 1e-12 * closed


def test_readers_take_the_new_keywords_and_columns():
    atoms, basis, opts = T.load("ion216_mk_at")
    assert opts["axilrod_teller"] == 1 and opts["midzuno_kihara_approx"] == 1
    assert np.all(atoms["c6"] == 64.3) and np.all(atoms["c9"] == 0.0)
    atoms, basis, opts = T.load("water64_at")
    assert opts["axilrod_teller"] == 1 and "midzuno_kihara_approx" not in opts
    assert sorted(set(atoms["c9"].tolist())) == [25.0, 1200.0, 6000.0]
    assert np.all(atoms["c6"] == 0.0) and np.all(atoms["has_disp"] == 0)


@pytest.mark.parametrize("name", util.SMALL)
def test_existing_fixtures_load_as_before(name, tmp_path):
    atoms, basis, opts = util.load_fixture(name)
    assert "axilrod_teller" not in opts and "midzuno_kihara_approx" not in opts
    assert np.all(atoms["c6"] == 0.0) and np.all(atoms["c9"] == 0.0)
    # the generator prints the committed text byte for byte
    gen_box.materialize(name, str(tmp_path))
    for ext in (".pqr", ".in"):
        assert filecmp.cmp(str(tmp_path / (name + ext)), os.path.join(util.GOLDEN, name + ext), shallow=False), (name, ext)


def test_three_body_fixtures_stay_out_of_the_oracle_lists():
    assert not set(gen_box.THREE_BODY_FIXTURES) & set(gen_box.SMALL_FIXTURES + gen_box.LARGE_FIXTURES + util.SMALL)
    for name in gen_box.THREE_BODY_FIXTURES:
        gen_box.fixture(name)


def test_axilrod_teller_is_no_longer_refused_by_the_reader():
    assert "axilrod_teller" not in pqr.UNSUPPORTED_ON


def test_library_exports_the_entry_points():
    L = energy.lib()
    assert hasattr(L, "mpmc_set_axilrod_teller") and hasattr(L, "mpmc_axilrod_teller")
    hdr = open(os.path.join(os.path.dirname(mbuild.HERE), "include", "mpmc_energy.h")).read()
    assert "#define MPMC_K_THREE_BODY 6" in hdr and "#define MPMC_K_DIPOLE_FAR 6" in hdr and "#define MPMC_ABI_VERSION 6" in hdr


def test_three_body_kernels_spill_nothing():
    notes = _kernel_notes("kernels_three_body.hip.o")
    full = [k for k in notes if "k_three_body" in k and "delta" not in k and "sum" not in k and "mark" not in k]
    delta = [k for k in notes if "k_three_body_delta" in k]
    assert len(full) == 2 and len(delta) == 2, list(notes)  # orthorhombic and skewed
    for name in full + delta:
        meta = notes[name]
        assert meta["sgpr_spill_count"] == 0 and meta["vgpr_spill_count"] == 0 and meta["private_segment_fixed_size"] == 0, (name, meta)
        assert meta["vgpr_count"] <= 128, (name, meta)
