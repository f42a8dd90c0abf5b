"""Crystal lattices in orthorhombic, mildly and strongly skewed cells: thousands of pairs at a fractional separation of exactly +-0.5,
+-1.5, +-2.5 along a lattice direction, where the image the reference takes is decided by the last bit of its three-term sum
rint(((0 + R[0][p] d0) + R[1][p] d1) + R[2][p] d2), and cells in which that image is not the nearest one (60 and 120 degree angles,
the fcc primitive cell: plane spacing 0.866 L or less against a cutoff of half the shortest lattice vector).  Shared by
tests/test_lattice_tie_preconditions.py (what makes these inputs mean something, on the CPU) and tests/test_gpu_lattice_ties.py (the
device against the oracle).  Needs no device.

  cells     ortho        three unequal edges
            tri_mild     the basis of ion216_triclinic
            tri_general  tri_mild turned about z and then x: all nine entries non-zero
            hex60/120    a = (L, 0, 0), b = (+-L / 2, L sqrt(3) / 2, 0), c = (0, 0, 1.1 L)
            rhombo       the fcc primitive cell, all angles 60 degrees
            every cell has its lattice sites SPACING (4 A) or a little less apart along its lattice vectors; the nearest two sites of any
            cell are more than 2.3 A apart (asserted by the CPU file), the floor of the volume-trial preconditions
  sites     G x G x G points k / G of the fractional coordinates, G even, pos = (frac + whole cells) @ basis; OCCUPIED of them hold an atom
            (a seeded draw: no symmetry cancels the fields), a third of the atoms lie 1 or 2 cells away along each lattice vector (ties
            at 1.5 and 2.5: ties-to-even alternates), and up to 24 sorbate molecules of two or three sites sit in the voids, 2.3 A or
            more from every lattice site (vacant ones too) and from each other
  variants  crystal      every lattice atom its own mobile molecule
            framework    the lattice atoms are one frozen molecule (the ties reach the polarization and three-body terms only)
  sizes     G = 4 (two tiles), G = 6 (four tiles: the smallest box with a panel table) and G = 12 (about 1 440 atoms, 23 tiles)
            The large boxes and the slabs (SLABS: G x G x 3 G sites at G = 6 in a cell three times as long along c, listed layer by
            layer) are there for the tile-pair classes: their atoms lie whole cells away by REGION (by_region), not at random, so that
            tiles stay compact in the raw coordinates and share image indices, and their Thole damping is FAR_DAMP, so that the
            far-field walk starts at 5 A: with random shifts every tile spans whole cells in the raw coordinates and no tile pair
            has a common index, and at the usual damping of 2.1304 no two tiles of these boxes lie beyond the damping range
  layers    LAYERS: one fully occupied 8 x 8 lattice layer per tile of the list order, 24 layers along c: tile pairs whose extreme is
            a tie in the bounds themselves (margin_cases), for the 1e-9 margins of k_classify's uniform-image test
"""
import math

import numpy as np

E2R = 408.7816
SPACING = 4.0
OCCUPIED = 0.8
MIN_DIST = 2.3
CELLS = ("ortho", "tri_mild", "tri_general", "hex60", "hex120", "rhombo")
TRICLINIC = CELLS[1:]
SKEWED = ("hex60", "hex120", "rhombo")  # the reference's image is not the nearest one for pairs inside the cutoff
VARIANTS = ("crystal", "framework")
SLABS = ("tri_general_slab", "hex60_slab", "hex120_slab")  # G x G x 3 G sites in a cell three times as long along c: tile pairs beyond the cutoff
# Whole layers as tiles: G_LAYERS x G_LAYERS sites per layer, every one occupied, are one 64-atom tile of the list order; LAYER_COUNT
# layers along c, which is perpendicular to a and b in these cells, so that the raw fractional c of an atom is one product and the same
# double for a whole layer.  Two tiles half a cell apart along c are then a tile pair whose extreme IS a tie, in both bounds: what the
# 1e-9 margins of k_classify's uniform-image test are for (margin_cases).  LAYER_SCALE stretches c until the rounding falls so that some
# tile pair passes the test without the margin while its pairs round to the other image (test_lattice_tie_preconditions asserts it).
LAYERS = ("hex60_layers", "hex120_layers")
G_LAYERS, LAYER_COUNT = 8, 24
LAYER_SCALE = {"hex60_layers": 1.11, "hex120_layers": 1.11}  # (the first of 1.00, 1.01, ... with two such tile pairs)
MAX_ATOMS = 2000  # no box of these tests is larger


def _sizes():
    """G of the three sizes from the tile size of the kernels (util.ladder_constants): the largest even G that fits two tiles (no panel
    table below three), the smallest whose lattice alone fills more than two, the largest that stays under MAX_ATOMS (the pair sweep's own
    threshold, util.size_ladder()["sweep"], lies above that: the GPU file switches the sweep on)"""
    import util

    tile = util.ladder_constants()["kTile"]
    most = lambda G: OCCUPIED * G ** 3 + 3 * min(G ** 3 // 5, 24)  # lattice atoms and three-site sorbates
    even = range(2, 32, 2)
    return {"small": max(G for G in even if most(G) <= 2 * tile), "panel": min(G for G in even if OCCUPIED * G ** 3 > 2 * tile),
            "large": max(G for G in even if most(G) < MAX_ATOMS)}


SIZES = _sizes()  # 4, 6 and 12 at 64-atom tiles
# Thole damping of the large boxes and the slabs.  The far-field walk of the Jacobi contraction starts at 30 / polar_damp: 14.1 A at
# the usual 2.1304, which no two tiles of a 48 A cell with 23 tiles are apart.  At 6.0 it starts at 5 A, the pairs on a half-cell
# tie (24 A apart) are far-field pairs, and the oracle damps with the same constant.
FAR_DAMP = 6.0
# The G = 4 boxes have some 320 ties per direction, of which a fused sum would move 2 to 10 %; which ones depends on the last bits of the
# basis.  Where the edge of SPACING G left fewer than the 20 that test_lattice_tie_preconditions asks of every skewed box, the edge is
# scaled by the factor below (the first of 1.01, 1.02, ... that gave 20; in the two hexagonal cells only direction a has two non-zero
# products to fuse).  The lattice sites move apart, never closer.
SCALE = {("tri_mild", 4): 1.01, ("hex60", 4): 1.09, ("hex120", 4): 1.14}

OPTIONS = {"rd_only": 0, "rd_lrc": 1, "polarization": 1, "polar_iterative": 1, "polar_ewald": 1, "polar_max_iter": 4, "polar_gs": 0,
           "polar_rrms": 0, "ewald_kmax": 7, "polar_precision": 0.0, "polar_gamma": 1.0, "polar_damp": 2.1304, "damp_type": "exponential",
           "ewald_alpha": None, "polar_ewald_alpha": None, "wolf": 0, "feynman_hibbs": 0, "feynman_hibbs_order": 0, "temperature": 0.0}


def _rotation():
    """a fixed turn about z by 0.61 rad, then about x by 0.43 rad"""
    cz, sz, cx, sx = math.cos(0.61), math.sin(0.61), math.cos(0.43), math.sin(0.43)
    rz = np.array([[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]])
    rx = np.array([[1.0, 0.0, 0.0], [0.0, cx, -sx], [0.0, sx, cx]])
    return rx @ rz


def by_region(name, G):
    """the boxes with tile-pair classes: the large ones and the slabs"""
    return G == SIZES["large"] or name in SLABS + LAYERS


def cell(name, G):
    """basis [3, 3] (rows = lattice vectors) of cell `name` with G sites along each lattice vector (a slab: 3 G along c, three times as long)"""
    if name in SLABS:
        b = cell(name[:-len("_slab")], G)
        b[2] *= 3.0
        return b
    if name in LAYERS:
        b = cell(name[:-len("_layers")], G)
        b[2] *= LAYER_SCALE[name] * LAYER_COUNT / G
        return b
    L = SPACING * G * SCALE.get((name, G), 1.0)
    mild = np.array([[24.0, 0.0, 0.0], [3.0, 23.0, 0.0], [-2.0, 4.0, 22.0]]) * (L / 24.0)
    if name == "ortho":
        return np.diag([L, 0.9 * L, 1.1 * L])
    if name == "tri_mild":
        return mild
    if name == "tri_general":
        return mild @ _rotation().T
    if name in ("hex60", "hex120"):
        s = 0.5 if name == "hex60" else -0.5
        return np.array([[L, 0.0, 0.0], [s * L, L * math.sqrt(3.0) / 2.0, 0.0], [0.0, 0.0, 1.1 * L]])
    if name == "rhombo":
        a = L / math.sqrt(2.0)
        return np.array([[0.0, a, a], [a, 0.0, a], [a, a, 0.0]])
    raise KeyError(name)


def nearest_image_distances(d, basis):
    """|d + n B| minimised over n in {-1, 0, 1}^3 after the rint image: the true nearest image for the cells of this file"""
    f = d @ np.linalg.inv(basis)
    d0 = (f - np.rint(f)) @ basis
    best = np.full(d.shape[:-1], np.inf)
    for i in (-1, 0, 1):
        for j in (-1, 0, 1):
            for k in (-1, 0, 1):
                v = d0 + np.array([i, j, k], dtype=np.float64) @ basis
                best = np.minimum(best, np.sqrt((v * v).sum(axis=-1)))
    return best


_SORBATES = {2: (np.array([[-0.37, 0.0, 0.0], [0.37, 0.0, 0.0]]), np.array([0.25, -0.25]), np.array([0.6, 0.0])),
             3: (np.array([[0.0, 0.0, 0.0], [-1.16, 0.0, 0.0], [1.16, 0.0, 0.0]]), np.array([0.65, -0.325, -0.325]), np.array([1.1, 0.0, 0.0]))}


def _random_rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


_cache = {}


def box(name, G, variant="crystal"):
    """(atoms, basis, opts, info): info = {"n_lattice", "vacant": positions [v, 3] of the vacant lattice sites (in the home cell),
    "sorbates": [(first, end)] of the sorbate molecules, "lattice_mol": None or the framework's mol_id}"""
    key = (name, G, variant)
    if key in _cache:
        a, b, o, i = _cache[key]
        return {k: v.copy() for k, v in a.items()}, b.copy(), dict(o), i
    assert G % 2 == 0 and variant in VARIANTS
    rng = np.random.default_rng(1000 * (CELLS + SLABS + LAYERS).index(name) + G)  # (the variants share sites, charges and sorbates)
    basis = cell(name, G)
    dims = np.array([G, G, 3 * G if name in SLABS else LAYER_COUNT if name in LAYERS else G])
    ijk = np.stack(np.meshgrid(*[np.arange(d) for d in dims], indexing="ij"), axis=-1).reshape(-1, 3)
    if name in SLABS + LAYERS:  # layer by layer along c: in list order (spatial_sort = 0) the tiles are slices of the slab
        ijk = ijk[np.lexsort((ijk[:, 1], ijk[:, 0], ijk[:, 2]))]
    n_sites = len(ijk)
    taken = np.sort(rng.permutation(n_sites)[:int(round((1.0 if name in LAYERS else OCCUPIED) * n_sites))])
    vacant = np.setdiff1d(np.arange(n_sites), taken)
    nl = taken.size
    frac = ijk[taken] / dims
    if by_region(name, G):
        # the lower third of every lattice direction one cell down, the upper third one cell up (ties at 0.5 within a third, 1.5 against
        # the middle, 2.5 between the outer two): neighbours in space stay neighbours in the raw coordinates, so that a tile of the
        # spatial order has a common image index with most other tiles
        third = ijk[taken] * 3 // dims
        cells_away = third - 1
    else:
        far = rng.random(nl) < 1.0 / 3.0
        cells_away = np.where(far[:, None], rng.integers(-2, 3, size=(nl, 3)), 0)
    lat_pos = (frac + cells_away) @ basis
    all_sites = (ijk / dims) @ basis
    # sorbates in the voids
    n_sorb = min(G ** 3 // 5, 24)
    placed, kinds = [], []
    tries = 0
    while len(placed) < n_sorb:
        tries += 1
        assert tries < 20000, (name, G, len(placed))
        m = 2 if rng.random() < 0.5 else 3
        # near the middle of a random lattice cell, where the largest void is, in a random orientation
        centre = (rng.integers(0, dims) + 0.5 + rng.uniform(-0.12, 0.12, size=3)) / dims
        body = _SORBATES[m][0] @ _random_rotation(rng).T + centre @ basis
        others = np.concatenate([all_sites] + placed) if placed else all_sites
        if nearest_image_distances(body[:, None, :] - others[None, :, :], basis).min() >= MIN_DIST + 0.05:
            placed.append(body)
            kinds.append(m)
    n = nl + sum(kinds)
    pos = np.concatenate([lat_pos] + placed)
    sign = np.where(rng.random(nl) < 0.5, -1.0, 1.0)
    q = np.concatenate([0.4 * E2R * sign] + [_SORBATES[m][1] * E2R for m in kinds])
    alpha = np.concatenate([rng.uniform(0.6, 1.4, nl)] + [_SORBATES[m][2] for m in kinds])
    eps = np.concatenate([rng.uniform(30.0, 120.0, nl)] + [np.full(m, 36.7) if m == 2 else np.array([29.7, 80.5, 80.5]) for m in kinds])
    sig = np.concatenate([rng.uniform(2.4, 3.2, nl)] + [np.full(m, 2.958) if m == 2 else np.array([2.8, 3.05, 3.05]) for m in kinds])
    mass = np.concatenate([rng.uniform(12.0, 60.0, nl)] + [np.full(m, 1.008) if m == 2 else np.array([12.0, 16.0, 16.0]) for m in kinds])
    lattice_mol = None
    if variant == "crystal":
        mol = list(range(nl))
        frozen = np.zeros(n, dtype=np.int32)
    else:
        mol = [0] * nl
        frozen = np.concatenate([np.ones(nl, dtype=np.int32), np.zeros(n - nl, dtype=np.int32)])
        lattice_mol = 0
    sorbates, at, nxt = [], nl, (nl if variant == "crystal" else 1)
    for m in kinds:
        mol += [nxt] * m
        sorbates.append((at, at + m))
        at += m
        nxt += 1
    atoms = {"pos": pos, "charge": q, "polarizability": alpha, "epsilon": eps, "sigma": sig, "mol_id": np.asarray(mol, dtype=np.int32),
             "frozen": frozen, "has_disp": np.zeros(n, dtype=np.int32), "mass": mass}
    info = {"n_lattice": nl, "vacant": all_sites[vacant], "sorbates": sorbates, "lattice_mol": lattice_mol, "G": G}
    _cache[key] = atoms, basis, dict(OPTIONS, polar_damp=FAR_DAMP if by_region(name, G) else OPTIONS["polar_damp"]), info
    return box(name, G, variant)


def n_tiles(atoms, tile):
    return -(-len(atoms["charge"]) // tile)


# ---- what the preconditions count ------------------------------------------------------------------------------------------------------
def reference_image(d, R):
    """img [..., 3] = rint of the reference's sum, in its association order (numpy's elementwise products and sums are not fused)"""
    return np.stack([np.rint(((R[0, p] * d[..., 0]) + R[1, p] * d[..., 1]) + R[2, p] * d[..., 2]) for p in range(3)], axis=-1)


def reference_distance(d, basis, R):
    """|d - B^T img| as minimum_image forms it"""
    img = reference_image(d, R)
    di = np.stack([d[..., p] - (((basis[0, p] * img[..., 0]) + basis[1, p] * img[..., 1]) + basis[2, p] * img[..., 2]) for p in range(3)], axis=-1)
    return np.sqrt(((di[..., 0] * di[..., 0]) + di[..., 1] * di[..., 1]) + di[..., 2] * di[..., 2])


def pair_displacements(atoms):
    """(i, j, d = pos_i - pos_j) over the pairs i < j"""
    pos = atoms["pos"]
    i, j = np.triu_indices(len(pos), 1)
    return i, j, pos[i] - pos[j]


def tie_components(d, R, tol=1e-9):
    """per lattice direction p: (indices into d of the pairs whose fractional separation lies within tol of a half-integer, the k of each:
    |f| = k + 1/2)"""
    out = []
    for p in range(3):
        f = np.abs(((R[0, p] * d[:, 0]) + R[1, p] * d[:, 1]) + R[2, p] * d[:, 2])
        k = np.floor(f)
        hit = np.nonzero(np.abs(f - (k + 0.5)) < tol)[0]
        out.append((hit, k[hit].astype(int)))
    return out


def fused_index_differs(d, R, p):
    """for each displacement: whether rint(fma(R[2][p], d2, fma(R[1][p], d1, R[0][p] * d0))) -- every fma rounded once, from exact
    rationals -- is another integer than the reference's rint(((R[0][p] d0) + R[1][p] d1) + R[2][p] d2)"""
    from fractions import Fraction as Fr

    r0, r1, r2 = Fr(float(R[0, p])), Fr(float(R[1, p])), Fr(float(R[2, p]))
    ref = reference_image(d, R)[:, p]
    out = np.zeros(len(d), dtype=bool)
    for n, (x, y, z) in enumerate(d):
        t = float(R[0, p]) * float(x)  # one rounding
        t = float(r1 * Fr(float(y)) + Fr(t))  # fma: exact product and sum, one rounding
        t = float(r2 * Fr(float(z)) + Fr(t))
        out[n] = float(np.rint(t)) != ref[n]
    return out


def nearer_image_pairs(atoms, basis, R, cutoff):
    """pairs i < j whose nearest image lies inside the cutoff while the image the reference takes lies outside it"""
    _, _, d = pair_displacements(atoms)
    return int(((nearest_image_distances(d, basis) < cutoff) & (reference_distance(d, basis, R) > cutoff)).sum())


def restated_counts(atoms, basis, R, cutoff):
    """the oracle's pair counts from the rint image and the cutoff predicates alone (lj :934, coulombic_real :1490), in numpy"""
    i, j, d = pair_displacements(atoms)
    r = reference_distance(d, basis, R)
    mol, fr, q, eps, sig = (atoms[k] for k in ("mol_id", "frozen", "charge", "epsilon", "sigma"))
    intra = mol[i] == mol[j]
    frozen = (fr[i] != 0) & (fr[j] != 0)
    rd_excl = intra | (eps[i] == 0) | (eps[j] == 0) | (sig[i] == 0) | (sig[j] == 0)
    es_excl = intra | (q[i] == 0) | (q[j] == 0)
    return {"n_pairs": len(i), "n_intra": int(intra.sum()), "n_rd_excluded": int(rd_excl.sum()), "n_es_excluded": int(es_excl.sum()),
            "n_frozen": int(frozen.sum()), "n_lj_in_cutoff": int(((r - 1e-12 < cutoff) & ~rd_excl & ~frozen).sum()),
            "n_es_in_cutoff": int((~(r > cutoff) & ~es_excl & ~frozen).sum())}


_oracle = {}


def oracle(name, G, variant="crystal", **changes):
    """the oracle's energy() of a box under OPTIONS with `changes`, computed once per process; the caller leaves it unchanged"""
    from oracle import OracleSystem

    key = (name, G, variant, tuple(sorted(changes.items())))
    if key not in _oracle:
        atoms, basis, opts, _ = box(name, G, variant)
        _oracle[key] = OracleSystem(atoms, basis, dict(opts, **changes)).energy()
    return _oracle[key]


def margin_cases(atoms, R, tile, margin=1e-9):
    """The uniform-image test of k_classify restated for the tiles of the LIST order (spatial_sort = 0), in a skewed cell: per tile the
    range of the raw fractional coordinates fraw_p = ((R[0][p] x) + R[1][p] y) + R[2][p] z as k_tile_bounds forms them, per tile pair
    I < J and direction p the extreme differences lo = ilo - jhi, hi = ihi - jlo and m0 = rint(lo); the direction counts as common
    when lo - m0 > -0.5 + margin and hi - m0 < 0.5 - margin.  Returns [(I, J, p, m0, pairs)]: the cases that pass the test with margin 0
    but not with `margin`, in which `pairs` atom pairs' own sums round to another index than m0 -- what the margin is there for."""
    pos = atoms["pos"]
    n = len(pos)
    nt = -(-n // tile)
    fraw = np.stack([((R[0, p] * pos[:, 0]) + R[1, p] * pos[:, 1]) + R[2, p] * pos[:, 2] for p in range(3)], axis=1)
    lo_t = np.array([fraw[t * tile:(t + 1) * tile].min(axis=0) for t in range(nt)])
    hi_t = np.array([fraw[t * tile:(t + 1) * tile].max(axis=0) for t in range(nt)])
    out = []
    for I in range(nt):
        for J in range(I + 1, nt):
            for p in range(3):
                lo, hi = lo_t[I, p] - hi_t[J, p], hi_t[I, p] - lo_t[J, p]
                m0 = np.rint(lo)
                zero = (lo - m0 > -0.5) and (hi - m0 < 0.5)
                kept = (lo - m0 > -0.5 + margin) and (hi - m0 < 0.5 - margin)
                if zero and not kept:
                    d = pos[I * tile:(I + 1) * tile, None, :] - pos[None, J * tile:(J + 1) * tile, :]
                    other = int((reference_image(d, R)[..., p] != m0).sum())
                    if other:
                        out.append((I, J, p, float(m0), other))
    return out
