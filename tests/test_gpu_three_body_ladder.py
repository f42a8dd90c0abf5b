"""GPU (MI355X): the Axilrod-Teller kernels (kernels_three_body.hip) against the exact oracle (orc_axilrod_teller_exact /
orc_axilrod_teller_delta_exact: long double terms from the contract's cosine form, Neumaier sums) on every launch path.

k_three_body starts min(tile triples, kThreeBodyBlocks) workgroups and strides over the rest; k_three_body_delta does the same over tile
pairs.  util.three_body_ladder() reads kThreeBodyBlocks out of kernels.h, so the rungs move with it: the full sum at the last tile count
with one workgroup per tile triple (35 full tiles) and one tile more holding a single atom, the delta at the last tile count with one
workgroup per tile pair (127 tiles) and one more.  Every rung runs in a cubic cell (k_three_body<true>, k_three_body_delta<true>) and a
triclinic one (<false>).  The boxes are heterogeneous: molecules of 1-4 sites, frozen molecules and one frozen framework molecule,
unwrapped coordinates, c9 from gen_box.AT_C9, a few atoms with alpha = 0 and a few with c9 = 0 (the two zero branches of
three_body_coefficients).  The sparse 10 000-atom boxes walk all 157 tiles (657 359 tile triples, 80 per workgroup) while only a
scattered ~14 % of the atoms carry the term, so that the oracle sums the triples of that subset alone.

Tolerances: no blanket bound.  Each comparison is held to the bound `full_bound` / `delta_bound` derives from the oracle's sum of term
scales S = sum |c9_ijk| (1 + 3 |cos A cos B cos C|) / (r_ij r_ik r_jk)^3 (>= the sum of |term|) and from the kernel's longest sequential
accumulation.  Run with -s for the measured deviation of every rung next to its bound."""
import math

import numpy as np
import pytest

import three_body_ref as T
import util
from mpmcxx_amd import energy, gen_box

pytestmark = pytest.mark.gpu

CONST = util.ladder_constants()
TILE, BLOCKS = CONST["kTile"], CONST["kThreeBodyBlocks"]
RUNGS = util.three_body_ladder()
EPS = np.finfo(float).eps
CELLS = ["cubic", "triclinic"]
OPTS = {"rd_only": 1, "rd_lrc": 1, "axilrod_teller": 1}

# One term of the kernel, (a_ab a_c) (d - 3P) / ((u_ab + u_c) d^2 sqrt(d)), against the oracle's cosine form from the same fp64 image
# vectors (min_image_sq rounds like orc_minimum_image): the three dot products (3 ulp each, absolute, of |u||v|), P and d (a product of
# three: 2 ulp more each, |P| <= d), d - 3P (absolute error ~45 ulp of d, which is what the cancellation of 1 + 3 cos cos cos costs), the
# denominator (~8 ulp) and the host's coefficients a = 6.7483345 alpha, u = 1 / (c9 / a^3) (~6 ulp each, three atoms): under 64 ulp of
# the term's scale |c9_ijk| (1 + 3 |cos cos cos|) / r^9.
K_TERM = 64
# after the lanes: wave_sum (6 levels), k_three_body_sum (ceil(grid / 256) strided adds per thread, wave_sum, four wave partials), the
# unit factor, and one rounding of the result
def tail(grid):
    return 6 + math.ceil(grid / 256) + 6 + 3 + 1 + 1


def full_bound(x, n, nonzero=TILE * TILE):
    """|GPU - oracle| of E3 for n atoms, oracle result x.  A lane adds (tile triples per workgroup) x 64 x 64 terms one after the other:
    the classical bound (k - 1) eps sum |x_i| of a sequential sum, each term's own error K_TERM eps of its scale, the tail.
    Adding an exact zero is exact (a masked triple adds 0.0, and a triple with an atom whose term vanishes carries a = 0, so its e is
    0 * finite / finite), so only the non-zero additions count: `nonzero` bounds them per lane and tile triple (the lane's own atom and
    the (i, j) pairs of the two other tiles that carry the term: k^2 where every tile holds k such atoms; 64 x 64 in general)."""
    nt = -(-n // TILE)
    triples = nt * (nt + 1) * (nt + 2) // 6
    grid = min(triples, BLOCKS)
    per_lane = -(-triples // grid) * nonzero
    return EPS * (K_TERM + per_lane + tail(grid)) * x["scale"]


def delta_bound(d, n, m, e3_acc, e3_trial):
    """|(trial - accepted) - oracle delta| for m moved atoms out of n.  A lane adds (tile pairs per workgroup) x m x 64 differences
    e_new - e_old (one rounding more per term); the trial total is accepted + delta rounded, and the test subtracts accepted again: eps
    of each total (what getting a delta from two totals costs)."""
    nt = -(-n // TILE)
    pairs = nt * (nt + 1) // 2
    grid = min(pairs, BLOCKS)
    per_lane = -(-pairs // grid) * m * TILE
    return EPS * (K_TERM + 1 + per_lane + tail(grid)) * d["scale"] + EPS * (abs(e3_acc) + abs(e3_trial))


DEVIATIONS = {}


@pytest.fixture(scope="module", autouse=True)
def _need_device_and_report():
    if energy.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests need an MI355X")
    import oracle as orc

    orc.lib()
    yield
    if DEVIATIONS:
        print("\nthree-body rungs: |GPU - exact oracle|, its bound, and the deviation relative to the oracle value:")
        for label, (dev, bound, ref) in DEVIATIONS.items():
            rel = dev / abs(ref) if ref else float("inf") if dev else 0.0
            print(f"  {label}: {dev:.2e} (bound {bound:.2e}, {dev / bound if bound else 0.0:.1e} of it; rel {rel:.1e})")


def check(label, got, ref, bound):
    DEVIATIONS[label] = (abs(got - ref), bound, ref)
    assert abs(got - ref) <= bound, (label, got, ref, abs(got - ref), bound)


# ---- boxes -----------------------------------------------------------------------------------------------------------------------------
def tb_box(n, cell, seed, active=None, single_molecule=False):
    """n atoms at ~45 A^3 each.  Molecule centres (and the sites of a frozen framework molecule of n // 8 sites, from 32 atoms on) on a
    jittered lattice of the cell's fractional coordinates; the sites of a molecule 1.2 A from its centre along orthogonal axes; every
    molecule shifted by a random whole cell vector; boxes of fewer than 8 atoms hold one-atom molecules.  `active`: the fraction of atoms, drawn independently, that carry the term; every
    other atom has alpha = 0 or c9 = 0.  Otherwise a few atoms of each of those kinds."""
    rng = np.random.default_rng(seed)
    L = (45.0 * n) ** (1.0 / 3.0)
    basis = np.diag([L, L, L]) if cell == "cubic" else L * np.array([[1.0, 0.0, 0.0], [0.17, 1.0, 0.0], [-0.12, 0.21, 1.0]])
    n_frame = n // 8 if n >= 32 and not single_molecule else 0
    sizes, left = [], n - n_frame
    while left > 0:
        s = n if single_molecule else 1 if n < 8 else min(left, int(rng.choice([1, 1, 1, 2, 3, 4])))  # (three atoms make a triple)
        sizes.append(s)
        left -= s
    frame = np.zeros(len(sizes) + (1 if n_frame else 0), dtype=bool)
    if n_frame:
        at = int(rng.integers(0, len(sizes) + 1))
        sizes.insert(at, n_frame)
        frame[at] = True
    sizes = np.array(sizes)
    n_mob = int((~frame).sum())
    g = math.ceil((n_mob + n_frame) ** (1.0 / 3.0))
    pts = rng.permutation(g ** 3)[:n_mob + n_frame]
    ijk = np.stack([pts // (g * g), (pts // g) % g, pts % g], axis=1).astype(np.float64)
    xyz = ((ijk + 0.5 + rng.uniform(-0.08, 0.08, size=ijk.shape)) / g) @ basis
    pos = np.zeros((n, 3))
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    k = 0
    for mi, (f, s) in enumerate(zip(first, sizes)):
        if frame[mi]:
            pos[f:f + s] = xyz[n_mob:]
            continue
        R = np.linalg.qr(rng.normal(size=(3, 3)))[0]
        pos[f] = xyz[k]
        for a in range(1, s):  # (single_molecule boxes have at most four sites)
            pos[f + a] = xyz[k] + 1.2 * R[:, a - 1]
        k += 1
    mol = np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)
    pos = pos + (rng.integers(-1, 2, size=(len(sizes), 3)) @ basis)[mol]
    types = rng.choice(sorted(gen_box.AT_C9), size=n)
    c9 = np.array([gen_box.AT_C9[t] for t in types])
    alpha = rng.uniform(0.2, 1.5, n)
    if active is not None:
        off = rng.random(n) >= active
        half = rng.random(n) < 0.5
        alpha[off & half] = 0.0
        c9[off & ~half] = 0.0
    elif n >= 8:
        z = rng.choice(n, size=max(2, n // 40), replace=False)
        alpha[z[0::2]] = 0.0
        c9[z[1::2]] = 0.0
    frozen = (rng.random(len(sizes)) < 0.15) | frame
    atoms = {"pos": pos, "charge": np.zeros(n), "polarizability": alpha, "epsilon": rng.uniform(5.0, 150.0, n), "sigma": rng.uniform(2.0, 3.4, n),
             "mol_id": mol, "frozen": frozen[mol].astype(np.int32), "has_disp": np.zeros(n, dtype=np.int32), "mass": rng.uniform(1.0, 40.0, n),
             "c6": np.zeros(n), "c9": c9}
    return atoms, basis


def tile_sparse(atoms, basis, per_tile, seed):
    """the term on for exactly `per_tile` atoms of every 64-atom block of the list order, off for all others (alpha = 0 or c9 = 0, half each).  With the spatial sort off the blocks are the kernel's tiles, so every
    tile triple holds triples that carry the term, and the list order scatters each tile over the box: far and near tile triples alike
    carry weight (test_three_body.test_sparse_tile_rung_catches_any_dropped_tile_triple)."""
    rng = np.random.default_rng(seed)
    n = len(atoms["pos"])
    mol = atoms["mol_id"]
    # candidates: atoms on a lattice point of tb_box (a molecule's first site, the framework's sites), at least 0.84 lattice spacings apart
    first = np.concatenate([[True], mol[1:] != mol[:-1]])
    lattice = first | (atoms["frozen"] != 0) & (np.bincount(mol)[mol] > 4)
    # greedy spread: each pick is the candidate of its tile farthest (minimum image) from the atoms picked so far, so the subset has no
    # close pairs and the terms of far tile triples stay within a few decades of the near ones (the r^-9 falloff over a 4-6x range)
    frac = atoms["pos"] @ np.linalg.inv(basis)
    keep = np.zeros(n, dtype=bool)
    picked = np.zeros((0, 3))
    for t0 in range(0, n, TILE):
        idx = rng.permutation(np.arange(t0, min(n, t0 + TILE)))
        idx = idx[lattice[idx]]
        for _ in range(per_tile):
            if len(picked):
                d = frac[idx][:, None, :] - picked[None, :, :]
                d = (d - np.rint(d)) @ basis
                i = idx[int(np.argmax(np.sqrt((d * d).sum(axis=2)).min(axis=1)))]
            else:
                i = idx[0]
            keep[i] = True
            picked = np.vstack([picked, frac[i]])
            idx = idx[idx != i]
    a = dict(atoms)
    alpha, c9 = atoms["polarizability"].copy(), atoms["c9"].copy()
    alpha[keep & (alpha == 0.0)] = 0.8
    c9[keep & (c9 == 0.0)] = gen_box.AT_C9["Ar"]
    half = rng.random(n) < 0.5
    alpha[~keep & half] = 0.0
    c9[~keep & ~half] = 0.0
    a["polarizability"], a["c9"] = alpha, c9
    return a


def oracle_of(atoms, basis, opts=OPTS):
    from oracle import OracleSystem

    c9 = T.atom_c9(atoms["polarizability"], atoms["c6"], atoms["c9"], bool(opts.get("midzuno_kihara_approx")))
    return OracleSystem(atoms, basis, opts), c9


def check_trial(S, O, c9, first, new, label):
    """one trial move of S against the delta oracle (O holds the accepted positions); the trial is rejected again"""
    n, m = S.n, len(new)
    acc = S.observables["three_body_energy"]
    S.trial_energy(first, new)
    assert not S.last_trial_was_full(), label
    t = S.trial_observables["three_body_energy"]
    d = O.axilrod_teller_delta_exact(c9, first, new)
    check(label, t - acc, d["delta"], delta_bound(d, n, m, acc, t))
    obs = dict(S.trial_observables)
    S.reject()
    return obs


# ---- full sums -------------------------------------------------------------------------------------------------------------------------
# "sparse": the production path (spatial sort on).  P(some tile holds no atom of the subset) <= 156 x (1 - f)^64 + (1 - f)^16 (156 full
# tiles and the last one of 16 atoms; the subset is drawn independently of the spatial order) = 0.0098 + 0.089 = 0.099 for f = 0.14.
# Its bound is the general one (64 x 64 non-zero additions per tile triple), and about half of its far tile triples weigh less.
# "sparse_tiles": the spatial sort off, PER_TILE atoms of every tile carry the term (tile_sparse): the bound counts PER_TILE^2 non-zero
# additions per tile triple, and all but 3 of the ~648 000 tile triples from kThreeBodyBlocks on (whose terms cancel) weigh more than it
# (checked on the CPU for every one: test_three_body.test_sparse_tile_rung_catches_any_dropped_tile_triple), so a tile triple that the
# stride drops or repeats fails here.
SPARSE = 0.14
PER_TILE = 2
EDGES = [1, 2, 3, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, 3 * TILE + 1]
FULL = [pytest.param("edge", n, cell, None, id=f"edge-{n}-{cell}") for n in EDGES for cell in CELLS] + \
       [pytest.param("stride", n, cell, None, id=f"stride-{n}-{cell}") for n in util.rung_sizes(RUNGS["full"]) for cell in CELLS] + \
       [pytest.param("sparse", 10000, cell, SPARSE, id=f"sparse-10000-{cell}") for cell in CELLS] + \
       [pytest.param("sparse_tiles", 10000, cell, None, id=f"sparse_tiles-10000-{cell}") for cell in CELLS]


def sparse_tiles_box(n, cell):
    atoms, basis = tb_box(n, cell, seed=11 * n + CELLS.index(cell))
    return tile_sparse(atoms, basis, PER_TILE, seed=n + CELLS.index(cell)), basis


@pytest.mark.parametrize("kind, n, cell, active", FULL)
def test_full_sum_against_exact_oracle(kind, n, cell, active):
    if kind == "sparse_tiles":
        atoms, basis = sparse_tiles_box(n, cell)
    else:
        atoms, basis = tb_box(n, cell, seed=7 * n + CELLS.index(cell), active=active)
    nt = -(-n // TILE)
    O, c9 = oracle_of(atoms, basis)
    x = O.axilrod_teller_exact(c9)
    if kind == "sparse_tiles":
        energy.configure("spatial_sort", 0)  # (for the contexts created from here on: the tiles are the blocks of the list order)
    try:
        S = energy.System(atoms, basis, OPTS)
    finally:
        energy.configure("spatial_sort", 1)
    try:
        S.energy()
        got = S.observables["three_body_energy"]
        label = f"full {kind} n={n} ({nt} tiles) {cell}"
        if n < 3:
            assert got == 0.0 and x["e3"] == 0.0, (label, got)
            return
        assert x["count"] > 0 and got != 0.0, (label, x)
        check(label, got, x["e3"], full_bound(x, n, PER_TILE ** 2 if kind == "sparse_tiles" else TILE * TILE))
        assert S.axilrod_teller() == got, label  # the component entry point: the same launches, the same bits
        # a trial move on the same box: the delta kernel's equal-tile mask at the tile edges, its strided grid on the sparse boxes
        moves = [(n // 2 - 1, 3)] if not kind.startswith("sparse") else [(1234, 64), (n - 300, 256)]
        for first, m in moves:
            first = max(0, min(first, n - m))
            new = util.moved(atoms, first, m, seed=n + m)
            check_trial(S, O, c9, first, new, f"trial {kind} n={n} m={m} {cell}")
    finally:
        S.close()


@pytest.mark.parametrize("cell", CELLS)
def test_one_molecule_gives_exactly_zero(cell):
    """every triple of a box that is a single molecule is excluded (and so is every triple of fewer than three atoms)"""
    for n in (1, 2, 3, 4):
        atoms, basis = tb_box(n, cell, seed=n, single_molecule=True)
        assert len(set(atoms["mol_id"].tolist())) == 1
        S = energy.System(atoms, basis, OPTS)
        try:
            S.energy()
            assert S.observables["three_body_energy"] == 0.0, (n, cell, S.observables["three_body_energy"])
            S.trial_energy(0, atoms["pos"][:1] + 0.7)
            assert S.trial_observables["three_body_energy"] == 0.0, (n, cell)
            S.reject()
        finally:
            S.close()


# ---- trial moves -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", util.rung_sizes(RUNGS["delta"]))
@pytest.mark.parametrize("cell", CELLS)
def test_delta_grid_stride_rung(n, cell):
    """8128 atoms: 8128 tile pairs, one workgroup each; 8129: 8256 tile pairs, the delta kernel strides"""
    atoms, basis = tb_box(n, cell, seed=3 * n + CELLS.index(cell))
    O, c9 = oracle_of(atoms, basis)
    S = energy.System(atoms, basis, OPTS)
    try:
        S.energy()
        for first, m in ((n // 3, 1), (17, 3), (n - 40, 17)):
            check_trial(S, O, c9, first, util.moved(atoms, first, m, seed=m), f"trial stride n={n} m={m} {cell}")
    finally:
        S.close()


FIXTURE_TRIALS = [(name, m) for name in ("ion216_triclinic_at", "ion216_mk_at", "ion216_framework_at") for m in (1, 9, 65)]


@pytest.mark.parametrize("name, m", FIXTURE_TRIALS)
def test_fixture_trials_against_delta_oracle(name, m):
    atoms, basis, opts = T.load(name)
    O, c9 = oracle_of(atoms, basis, opts)
    S = energy.System(atoms, basis, opts)
    try:
        S.energy()
        for first in (0, 140, len(atoms["pos"]) - m):  # (the framework of ion216_framework_at is atoms 0-149)
            check_trial(S, O, c9, first, util.moved(atoms, first, m, seed=first + m), f"trial {name} first={first} m={m}")
    finally:
        S.close()


def test_moves_out_of_the_cell_by_lattice_vectors_and_repeats():
    atoms, basis, opts = T.load("ion216_triclinic_at")
    O, c9 = oracle_of(atoms, basis, opts)
    S = energy.System(atoms, basis, opts)
    try:
        S.energy()
        # out of the primary cell: 1.5 cell vectors and some noise
        new = util.moved(atoms, 60, 9, seed=5) + 1.5 * basis[0] - basis[2]
        check_trial(S, O, c9, 60, new, "trial out of the cell (ion216_triclinic_at)")
        # whole (one-atom) molecules by exactly one lattice vector: the oracle's delta is rounding only, and so must the GPU's be
        for first, m, vec in ((20, 9, basis[2]), (100, 40, basis[1] - basis[0])):
            new = atoms["pos"][first:first + m] + vec
            d = O.axilrod_teller_delta_exact(c9, first, new)
            assert abs(d["delta"]) <= 64 * EPS * d["scale"], d
            # (on the GPU the delta is trial - accepted, so delta_bound's eps (|E3_acc| + |E3_trial|) of the two totals dominates here,
            # not the few-ulp scale bound the oracle is held to: that rounding is in the quantity compared, not in the kernel)
            check_trial(S, O, c9, first, new, f"trial lattice vector m={m} (ion216_triclinic_at)")
        # a repeated trial gives the same bits, every field
        new = util.moved(atoms, 30, 9, seed=9)
        first_obs = check_trial(S, O, c9, 30, new, "trial repeat (ion216_triclinic_at)")
        S.trial_energy(30, new)
        assert dict(S.trial_observables) == first_obs
        S.reject()
    finally:
        S.close()
    # water64_at: whole three-site molecules by one lattice vector
    atoms, basis, opts = T.load("water64_at")
    O, c9 = oracle_of(atoms, basis, opts)
    S = energy.System(atoms, basis, opts)
    try:
        S.energy()
        new = atoms["pos"][30:45] - basis[1]
        d = O.axilrod_teller_delta_exact(c9, 30, new)
        assert abs(d["delta"]) <= 64 * EPS * d["scale"], d
        check_trial(S, O, c9, 30, new, "trial lattice vector m=15 (water64_at)")
    finally:
        S.close()


# ---- the size guard of mpmc_set_axilrod_teller -----------------------------------------------------------------------------------------
def test_size_guard_boundary():
    """2343 tiles have 2 145 100 440 tile triples (<= INT_MAX): accepted; 2344 tiles (149 953 atoms) have 2 147 846 920: refused.  Neither
    box is evaluated (O(N^3))."""
    last = 1
    while (last + 1) * (last + 2) * (last + 3) // 6 <= 2 ** 31 - 1:
        last += 1
    assert last == 2343
    for n, ok in ((last * TILE, True), (last * TILE + 1, False)):
        g = math.ceil(n ** (1.0 / 3.0))
        idx = np.arange(n)
        L = 3.6 * g
        pos = 3.6 * np.stack([idx // (g * g), (idx // g) % g, idx % g], axis=1).astype(np.float64)
        atoms = {"pos": pos, "charge": np.zeros(n), "polarizability": np.full(n, 1.0), "epsilon": np.full(n, 50.0), "sigma": np.full(n, 3.0),
                 "mol_id": idx.astype(np.int32), "frozen": np.zeros(n, dtype=np.int32), "has_disp": np.zeros(n, dtype=np.int32), "mass": np.ones(n)}
        S = energy.System(atoms, np.diag([L, L, L]), {"rd_only": 1})
        try:
            if ok:
                S.set_axilrod_teller(True, c9=np.full(n, 518.3))
            else:
                with pytest.raises(energy.MpmcError, match="more tile triples"):
                    S.set_axilrod_teller(True, c9=np.full(n, 518.3))
        finally:
            S.close()


# ---- the path-integral loop ------------------------------------------------------------------------------------------------------------
def test_pi_loop_with_the_term_on():
    """PI_calculate_potential sums {rd, coulombic, polarization, vdw} over the beads (reference pi.cpp; include/mpmc_energy.h): the term
    fills each bead's three_body_energy and leaves those sums bit for bit as they are without it"""
    atoms, basis, opts = T.load("water64_at")
    off_opts = {k: v for k, v in opts.items() if k not in ("axilrod_teller", "midzuno_kihara_approx")}
    pos = [gen_box.bead_positions(atoms["pos"], b) for b in range(4)]
    on = [energy.System(util.with_positions(atoms, p), basis, opts) for p in pos]
    off = [energy.System(util.with_positions(atoms, p), basis, off_opts) for p in pos]
    lone = [energy.System(util.with_positions(atoms, p), basis, opts) for p in pos]
    try:
        s_on, per_on, f_on = energy.pi_potential_local(on)
        s_off, per_off, f_off = energy.pi_potential_local(off)
        assert not f_on and not f_off
        assert s_on.tobytes() == s_off.tobytes(), (s_on, s_off)
        for b in range(4):
            lone[b].energy()
            e3 = lone[b].observables["three_body_energy"]
            assert e3 != 0.0 and per_on[b]["three_body_energy"] == e3, (b, per_on[b]["three_body_energy"], e3)
            assert per_off[b]["three_body_energy"] == 0.0
            for k in ("rd_energy", "coulombic_energy", "polarization_energy", "vdw_energy"):
                assert per_on[b][k] == per_off[b][k], (b, k)
    finally:
        for S in on + off + lone:
            S.close()
