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


# ---- the exact oracle (oracle/mpmc_oracle.c: orc_axilrod_teller_exact, orc_axilrod_teller_delta_exact) ---------------------------------
EPS = np.finfo(float).eps


def _oracle(atoms, basis, opts):
    from oracle import OracleSystem

    c9 = T.atom_c9(atoms["polarizability"], atoms["c6"], atoms["c9"], bool(opts.get("midzuno_kihara_approx")))
    return OracleSystem(atoms, basis, opts), c9


@pytest.mark.parametrize("name", gen_box.THREE_BODY_FIXTURES)
def test_exact_oracle_matches_restatement_and_goldens(name):
    atoms, basis, opts = T.load(name)
    O, c9 = _oracle(atoms, basis, opts)
    x = O.axilrod_teller_exact(c9)
    ours = T.for_case(atoms, basis, opts)
    # the restatement sums fp64 terms in numpy's pairwise order, rows one after the other: a few ulp of the sum of |term| apart
    assert abs(x["e3"] - ours) <= max(1e-12 * abs(x["e3"]), 8 * EPS * x["abs"]), (name, x, ours)
    assert x["abs"] >= abs(x["e3"]) and x["scale"] >= x["abs"] > 0 and x["count"] > 0, (name, x)
    # the goldens, with the bound of test_restatement_matches_reference_goldens
    g = util.golden(name)
    e3 = _ref_e3(g)
    bound = 8 * EPS * (abs(g["total"]) + abs(g["rd"]) + abs(g["es"]) + abs(g["polar"]))
    assert abs(x["e3"] - e3) <= max(1e-12 * abs(e3), bound), (name, x["e3"], e3)


def test_exact_oracle_counts_the_triples_of_the_contract():
    """water64_at: 64 three-site molecules whose H sites carry alpha = 0 (its atoms with a non-zero coefficient are the O and Xe sites,
    one per molecule at most): every triple of them, none excluded; ar3_at has its one triple"""
    atoms, basis, opts = T.load("water64_at")
    O, c9 = _oracle(atoms, basis, opts)
    on = (atoms["polarizability"] != 0) & (c9 != 0)
    k = int(on.sum())
    mol_on = np.bincount(atoms["mol_id"][on])
    same = sum(int(c) * (int(c) - 1) * (int(c) - 2) // 6 for c in mol_on)
    assert O.axilrod_teller_exact(c9)["count"] == k * (k - 1) * (k - 2) // 6 - same
    atoms, basis, opts = T.load("ar3_at")
    O, c9 = _oracle(atoms, basis, opts)
    assert O.axilrod_teller_exact(c9)["count"] == 1


def test_exact_oracle_is_independent_of_the_thread_count(tmp_path):
    """the rows are combined in atom order: the bits do not depend on OMP_NUM_THREADS (run in child processes, which read it at start)"""
    import subprocess
    import sys

    code = ("import sys; sys.path[:0] = [%r, %r]; import util, three_body_ref as T; from oracle import OracleSystem; "
            "a, b, o = T.load('ion216_triclinic_at'); c9 = T.atom_c9(a['polarizability'], a['c6'], a['c9'], False); "
            "x = OracleSystem(a, b, o).axilrod_teller_exact(c9); "
            "d = OracleSystem(a, b, o).axilrod_teller_delta_exact(c9, 40, a['pos'][40:45] + 0.2); "
            "print(float(x['e3']).hex(), float(d['delta']).hex())") % (os.path.join(util.ROOT, "tests"), util.ROOT)
    outs = set()
    for threads in ("1", "3", "8"):
        env = dict(os.environ, OMP_NUM_THREADS=threads)
        outs.add(subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True, timeout=300).stdout)
    assert len(outs) == 1, outs


# (fixture, first, m): cubic and triclinic cells; ranges inside one molecule, spanning several molecules, and over frozen atoms
DELTA_CASES = [("water64_at", 0, 1), ("water64_at", 31, 3), ("water64_at", 40, 65), ("ion216_triclinic_at", 7, 1), ("ion216_triclinic_at", 100, 3),
               ("ion216_triclinic_at", 150, 65), ("ion216_framework_at", 149, 3), ("ion216_framework_at", 120, 65), ("ion216_framework_at", 3, 1),
               ("ion216_mk_at", 151, 65)]


@pytest.mark.parametrize("name,first,m", DELTA_CASES)
def test_delta_oracle_is_the_difference_of_two_full_sums(name, first, m):
    from oracle import OracleSystem

    atoms, basis, opts = T.load(name)
    O, c9 = _oracle(atoms, basis, opts)
    new = util.moved(atoms, first, m, seed=first + m)
    if name == "ion216_triclinic_at" and m == 65:
        new = new + basis[1]  # (and out of the primary cell)
    d = O.axilrod_teller_delta_exact(c9, first, new)
    pos = atoms["pos"].copy()
    pos[first:first + m] = new
    old_x = O.axilrod_teller_exact(c9)
    new_x = OracleSystem(util.with_positions(atoms, pos), basis, opts).axilrod_teller_exact(c9)
    # the two totals are rounded to fp64 once each; everything else is long double (64-bit mantissa)
    bound = EPS * (abs(old_x["e3"]) + abs(new_x["e3"])) + 64 * 2.0 ** -63 * (old_x["abs"] + new_x["abs"])
    assert abs(d["delta"] - (new_x["e3"] - old_x["e3"])) <= bound, (name, first, m, d, new_x["e3"] - old_x["e3"], bound)
    assert d["delta"] != 0.0 and 0 < d["count"] <= old_x["count"] and d["abs"] <= old_x["abs"] + new_x["abs"], (d, old_x, new_x)


def test_delta_oracle_of_a_lattice_vector_move_is_rounding_only():
    """whole molecules moved by exactly one lattice vector: the same physics, the delta is the rounding of x + b alone"""
    atoms, basis, opts = T.load("ion216_triclinic_at")
    O, c9 = _oracle(atoms, basis, opts)
    d = O.axilrod_teller_delta_exact(c9, 20, atoms["pos"][20:29] + basis[2])
    assert abs(d["delta"]) <= 64 * EPS * d["scale"], d


def test_three_body_rungs_come_from_the_block_count():
    """test_gpu_three_body_ladder takes its grid-stride rungs from kThreeBodyBlocks (util.three_body_ladder): nt tiles fit one workgroup
    per tile triple (pair), nt + 1 do not"""
    blocks = util.ladder_constants()["kThreeBodyBlocks"]
    rungs = util.three_body_ladder()
    tri = lambda nt: nt * (nt + 1) * (nt + 2) // 6
    pairs = lambda nt: nt * (nt + 1) // 2
    assert tri(rungs["full"]) <= blocks < tri(rungs["full"] + 1), rungs
    assert pairs(rungs["delta"]) <= blocks < pairs(rungs["delta"] + 1), rungs


@pytest.mark.parametrize("cell", ["cubic", "triclinic"])
def test_sparse_tile_rung_catches_any_dropped_tile_triple(cell):
    """The "sparse_tiles" rung of test_gpu_three_body_ladder (10 000 atoms, spatial sort off, so tile T is atoms 64 T .. 64 T + 63) holds
    k_three_body to full_bound with PER_TILE^2 non-zero additions per tile triple.  Here, for every tile triple the grid-stride loop takes
    (index >= kThreeBodyBlocks), its own share of E3 is summed and must exceed that bound: a tile triple that tb_decode_triple or the
    stride skips or repeats moves the GPU result by more than the rung allows.  (The only tile triples without a triple that carries the
    term are those whose atoms of the subset are fewer than three, I = J = K, or all of one molecule; they contribute nothing at all.
    A handful of tile triples whose terms cancel are allowed, see below.)"""
    import test_gpu_three_body_ladder as G

    n = 10000
    atoms, basis = G.sparse_tiles_box(n, cell)
    O, c9 = G.oracle_of(atoms, basis)
    x = O.axilrod_teller_exact(c9)
    bound = G.full_bound(x, n, G.PER_TILE ** 2)
    act = np.nonzero((atoms["polarizability"] != 0) & (c9 != 0))[0]
    assert np.all(np.bincount(act // G.TILE, minlength=-(-n // G.TILE)) == G.PER_TILE)
    # every active triple's term (the restatement's arithmetic) and its tile triple t = K(K+1)(K+2)/6 + J(J+1)/2 + I
    from mpmcxx_amd import energy

    recip = energy.pbc_compute(basis)[0]
    pos, alpha, mol = atoms["pos"][act], atoms["polarizability"][act], atoms["mol_id"][act]
    a = alpha * T.A_SCALE
    inv_u = 1.0 / (c9[act] / a ** 3)
    D = T.min_image(basis, np.asarray(recip).reshape(3, 3), pos[:, None, :] - pos[None, :, :])
    R = np.sqrt(np.einsum("ijp,ijp->ij", D, D))
    tile = act // G.TILE
    nt = -(-n // G.TILE)
    n_triples = nt * (nt + 1) * (nt + 2) // 6
    share = np.zeros(n_triples)
    held = np.zeros(n_triples, dtype=bool)
    na = len(act)
    for i in range(na - 2):
        jj, kk = np.triu_indices(na - i - 1, 1)
        jj, kk = jj + i + 1, kk + i + 1
        ok = ~((mol[jj] == mol[i]) & (mol[kk] == mol[i]))
        jj, kk = jj[ok], kk[ok]
        ij, ik, jk = D[i, jj], D[i, kk], D[jj, kk]
        rij, rik, rjk = R[i, jj], R[i, kk], R[jj, kk]
        c = a[i] * a[jj] * a[kk] * 3.0 / (inv_u[i] + inv_u[jj] + inv_u[kk]) * T.UNIT
        cos3 = (np.einsum("tp,tp->t", ij, ik) / (rij * rik)) * (-np.einsum("tp,tp->t", ij, jk) / (rij * rjk)) * \
               (np.einsum("tp,tp->t", ik, jk) / (rik * rjk))
        e = c * (1.0 + 3.0 * cos3) / (rij * rik * rjk) ** 3
        I, J, K = tile[i], tile[jj], tile[kk]  # (act is ascending: I <= J <= K)
        t = K * (K + 1) * (K + 2) // 6 + J * (J + 1) // 2 + I
        np.add.at(share, t, e)
        held[t] = True
    assert abs(share.sum() - x["e3"]) <= 1e-12 * x["abs"], (share.sum(), x)
    strided = np.arange(n_triples) >= G.BLOCKS
    # the tile triples without a term: those whose atoms of the subset are all of one molecule (tiles inside the frozen framework)
    one_mol = np.full(nt, -1)
    for T_ in range(nt):
        m_ = set(mol[tile == T_].tolist())
        one_mol[T_] = m_.pop() if len(m_) == 1 else -1
    tet = lambda k: k * (k + 1) * (k + 2) // 6
    for t in np.nonzero(strided & ~held)[0]:
        K = max(k for k in range(nt) if tet(k) <= t)
        r = t - tet(K)
        J = max(j for j in range(K + 1) if j * (j + 1) // 2 <= r)
        I = r - J * (J + 1) // 2
        held_atoms = np.isin(tile, sorted({I, J, K}))
        assert held_atoms.sum() < 3 or len(set(mol[held_atoms].tolist())) == 1, (t, I, J, K)
    weak = np.nonzero(strided & held & ~(np.abs(share) > bound))[0]
    print(f"\n{cell}: {weak.size} strided tile triples at or below the bound")
    low = float(np.abs(share[strided & held]).min())
    print(f"\n{cell}: {int((strided & held).sum())} strided tile triples, the least |share| {low:.2e} = {low / bound:.1f} x the bound {bound:.2e}")
    # a few tile triples whose eight terms of both signs cancel to below the bound (3 of ~648 000 in either cell); every other skipped or
    # repeated tile triple fails the rung
    assert weak.size <= 5, (weak.size, weak[:10], share[weak[:10]], bound)
