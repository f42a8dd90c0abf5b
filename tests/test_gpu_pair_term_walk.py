"""GPU (MI355X): the shapes at which the two walks that the pair-sum terms share (csrc/pair_term_walk.h) can go wrong -- atom counts at a
tile edge, both values of rd_crystal's jsplit, the rd model's skip by class on and off, trial moves inside one tile, across two and across
a tile boundary with moved-moved pairs in both list orders, and a table above the grid cap.  Every case is an rd_only gen_box lattice box
held to the numpy restatement of its term (disp_expansion_ref, rd_crystal_ref, rd_model_ref) within the bounds the term's own GPU test
file uses for that comparison: the pair sum to 1e-12 of the summed magnitudes of its terms, counts exactly.
"""
import os
import re

import numpy as np
import pytest

import disp_expansion_ref as D
import rd_crystal_ref as RC
import rd_model_ref as RM
import util
from mpmcxx_amd import build as mbuild
from mpmcxx_amd import energy, gen_box

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
RESULT_FIELDS = [f for f, _ in energy.Result._fields_]
TERMS = ("disp", "crystal", "rdm")
EDGE_COUNTS = [1, 63, 64, 65, 128, 129]
TRIAL_KEYS = util.TRIAL_KEYS + ["lrc_pair", "lrc_self"]
BIG = 11648  # 182 tiles, 16 653 tile pairs: above the 16 384-workgroup cap, so the grid stride takes a second pass


@pytest.fixture(scope="module", autouse=True)
def _need_device():
    if energy.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests need an MI355X")


def result_bits(r):
    return {k: r[k] for k in RESULT_FIELDS}


def box_length(n):
    return 40.0 * (max(n, 8) / 1000.0) ** (1.0 / 3.0)  # (the density of the terms' own rd_only boxes; 8 A at the smallest counts)


def case(term, n, L=None, rows=None, basis=None, order=2, shuffle=None):
    """(atoms, basis, opts) of an rd_only lattice box with the term on; shuffle: seed of a permutation of the rows, so that the list order
    says nothing about the place"""
    L = L or box_length(n)
    rows = rows if rows is not None else gen_box.lattice_box(n, L, 11, charged=False, alpha=0.0)
    if term == "disp":
        rows = gen_box._with_disp(rows)
    elif term == "rdm":
        rows = gen_box.rd_model_species(rows)
    if shuffle is not None:
        rows = [rows[k] for k in np.random.default_rng(shuffle).permutation(n)]
    atoms = {"pos": np.array([[r.x, r.y, r.z] for r in rows]), "charge": np.zeros(n), "polarizability": np.zeros(n),
             "epsilon": np.array([r.eps for r in rows]), "sigma": np.array([r.sigma for r in rows]), "mass": np.full(n, 39.948),
             "mol_id": np.arange(n, dtype=np.int32), "frozen": np.zeros(n, np.int32), "has_disp": np.zeros(n, np.int32)}
    if term == "disp":
        atoms.update(has_disp=np.ones(n, np.int32), c6=np.array([r.c6 for r in rows]), c8=np.array([r.c8 for r in rows]),
                     c10=np.array([r.c10 for r in rows]))
    opts = {"disp": {"rd_only": 1, "disp_expansion": 1, "damp_dispersion": 1}, "crystal": {"rd_only": 1, "rd_lrc": 1, "rd_crystal": 1, "rd_crystal_order": order},
            "rdm": {"rd_only": 1, "rd_lrc": 1, "waldmanhagler": 1}}[term]
    return atoms, (np.diag([L] * 3) if basis is None else np.asarray(basis, dtype=np.float64)), opts


def info_of(term, S):
    return {"disp": lambda: {}, "crystal": S.rd_crystal_info, "rdm": S.rd_model_info}[term]()


def restated(term, atoms, basis, opts):
    return {"disp": D.for_case, "crystal": RC.for_case, "rdm": RM.for_case}[term](atoms, basis, opts)


def terms_of(term, info):
    return {"disp": None, "crystal": info.get("n_image_terms"), "rdm": info.get("n_terms")}[term]


def check_sum(term, r, info, ref, label):
    print(label, r["lj_pairs"], ref["lj_pairs"], abs(r["lj_pairs"] - ref["lj_pairs"]) / max(ref["mag"], 1e-300), info)
    assert abs(r["lj_pairs"] - ref["lj_pairs"]) <= 1e-12 * ref["mag"], (label, r["lj_pairs"], ref)
    if term == "crystal":
        assert info["n_image_terms"] == ref["n_image_terms"], (label, info, ref["n_image_terms"])
    if term == "rdm":
        assert info["n_terms"] == ref["n_terms"] and r["n_lj_in_cutoff"] == ref["n_lj_in_cutoff"], (label, info, ref)


def crystal_jsplit(n_atoms):
    """crystal_jsplit (kernels_crystal.hip) with the constant of kernels.h: waves per tile pair of the rd_crystal sum"""
    hdr = open(os.path.join(mbuild.CSRC, "kernels.h")).read()
    min_items = int(re.search(r"constexpr int kCrystalMinItems = (\d+);", hdr).group(1))
    tiles = (n_atoms + 63) // 64
    pairs, s = tiles * (tiles + 1) // 2, 1
    while s < 16 and pairs * s < min_items:
        s *= 2
    return s


@pytest.mark.parametrize("n", EDGE_COUNTS)
@pytest.mark.parametrize("term", TERMS)
def test_atom_counts_at_a_tile_edge(term, n):
    """1, 63, 64, 65 (one atom alone in the second tile), 128, 129 (an equal-tile pair next to two unequal ones); rd_crystal at order 2, so the
    image loop runs, with every tile pair split over 16 waves"""
    atoms, basis, opts = case(term, n)
    if term == "crystal":
        assert crystal_jsplit(n) == 16
    S = energy.System(atoms, basis, opts)
    S.energy()
    r, info = result_bits(S.observables), info_of(term, S)
    check_sum(term, r, info, restated(term, atoms, basis, opts), (term, n))
    S.energy()
    assert result_bits(S.observables) == r and info_of(term, S) == info
    S.close()


def test_rd_crystal_with_one_wave_per_tile_pair():
    """4 160 atoms: 65 tiles, 2 145 tile pairs, jsplit = 1 (the edge counts above run with 16); order 1, cubic cell.  The restatement of this
    box takes about four seconds on the host."""
    n = 4160
    assert crystal_jsplit(n) == 1 and crystal_jsplit(129) == 16
    atoms, basis, opts = case("crystal", n, order=1)
    S = energy.System(atoms, basis, opts)
    S.energy()
    check_sum("crystal", result_bits(S.observables), S.rd_crystal_info(), RC.for_case(atoms, basis, opts), ("crystal", n))
    S.close()


def test_rd_model_skip_by_class_on_and_off():
    """a long orthorhombic cell: tile pairs further apart than the cutoff are skipped by class; the same atoms in a sheared cell: the skip
    is off.  Both against the restatement."""
    n, cell = 2197, np.diag([26.0, 26.0, 104.0])
    rows = gen_box.lattice_box_cell(n, cell.tolist(), 17, charge=0.0, alpha=0.0)
    for label, basis in (("orthorhombic", cell), ("triclinic", cell + np.array([[0.0, 0.0, 0.0], [1.5, 0.0, 0.0], [0.0, 2.5, 0.0]]))):
        atoms, basis, opts = case("rdm", n, rows=rows, basis=basis)  # (rd_model_species sets the same species again)
        S = energy.System(atoms, basis, opts)
        S.energy()
        r, info = result_bits(S.observables), S.rd_model_info()
        check_sum("rdm", r, info, RM.for_case(atoms, basis, opts), ("rdm", label))
        tiles = (n + 63) // 64
        assert info["n_tile_pairs"] == tiles * (tiles + 1) // 2
        if label == "orthorhombic":
            assert info["n_tile_pairs_skipped"] > 0, info
        else:
            assert info["n_tile_pairs_skipped"] == 0, info
        S.close()


def _trial(term, first, m, sort):
    atoms, basis, opts = case(term, 129, shuffle=5)
    energy.configure("spatial_sort", 1 if sort else 0)  # (0: for the contexts created from here on the tiles are the blocks of the list order)
    try:
        S = energy.System(atoms, basis, opts)
        S.energy()
        accepted, info0 = result_bits(S.observables), info_of(term, S)
        new = util.moved(atoms, first, m, seed=m + first)
        S.trial_energy(first, new)
        t, ti = dict(S.trial_observables), info_of(term, S)
        assert not S.last_trial_was_full()
        box = {"disp": D.Box, "crystal": RC.Box, "rdm": RM.Box}[term](atoms, basis, opts)
        out = box.delta(first, new)
        d, mag = out[0], out[1]
        print(term, first, m, (t["lj_pairs"] - accepted["lj_pairs"]) - d, mag)
        assert abs((t["lj_pairs"] - accepted["lj_pairs"]) - d) <= 1e-12 * mag + 4 * EPS * abs(accepted["lj_pairs"]), (term, first, m, t["lj_pairs"], d)
        if term != "disp":
            assert terms_of(term, ti) - terms_of(term, info0) == out[2]
        pos = atoms["pos"].copy()
        pos[first:first + m] = new
        F = energy.System(util.with_positions(atoms, pos), basis, opts)
        F.energy()
        ref, ref_info = dict(F.observables), info_of(term, F)
        F.close()
        assert terms_of(term, ti) == terms_of(term, ref_info)
        bad = util.component_errors(t, ref, [k for k in TRIAL_KEYS if ref[k] != 0.0 or t[k] != 0.0], 1e-11)
        assert not bad, bad
        S.reject()
        S.energy()
        assert result_bits(S.observables) == accepted and info_of(term, S) == info0
        S.close()
    finally:
        energy.configure("spatial_sort", 1)


@pytest.mark.parametrize("term", TERMS)
def test_trial_move_of_two_atoms_in_one_tile(term):
    _trial(term, 10, 2, sort=False)  # (list order = slot order: atoms 10 and 11 share tile 0)


@pytest.mark.parametrize("term", TERMS)
def test_trial_move_of_two_atoms_in_two_tiles(term):
    _trial(term, 63, 2, sort=False)  # (atom 63 closes tile 0, atom 64 opens tile 1)


@pytest.mark.parametrize("term", TERMS)
def test_trial_move_of_65_atoms_across_a_tile_boundary(term):
    """65 moved atoms cannot share one 64-atom tile; the rows are shuffled, so under the spatial sort their slots rise and fall along the
    move list: moved-moved pairs in both list orders"""
    _trial(term, 32, 65, sort=True)


def test_grid_stride_second_pass_against_the_restatement():
    """11 648 atoms, disp-expansion (every tile pair contributes: a lost pass cannot hide): the full sum against the restatement, as
    test_ten_thousand_atoms_against_the_restatement compares it.  (The 6.8e7 pair terms of the restatement are most of this test's time.)"""
    tiles = (BIG + 63) // 64
    assert tiles * (tiles + 1) // 2 > 16384
    atoms, basis, opts = case("disp", BIG, L=90.0)
    S = energy.System(atoms, basis, opts)
    S.energy()
    ref = D.for_case(atoms, basis, opts)
    r = S.observables
    print(BIG, r["lj_pairs"], ref["lj_pairs"], abs(r["lj_pairs"] - ref["lj_pairs"]) / ref["mag"])
    assert abs(r["lj_pairs"] - ref["lj_pairs"]) <= 1e-12 * ref["mag"], (r["lj_pairs"], ref)
    assert abs(r["lrc_pair"] - ref["lrc_pair"]) <= 1e-12 * abs(ref["lrc_pair"]) and abs(r["lrc_self"] - ref["lrc_self"]) <= 1e-12 * abs(ref["lrc_self"])
    S.close()
