"""The boxes, configurations, moves and restatements of the trial-move matrix of polarizable boxes: the `polar_delta` branch of
mpmc_trial_energy_async (csrc/trial.cpp) under every solve configuration it serves, at the eight-tile limit of its restricted store pass
and across tile-pair class flips.  Shared by tests/test_polar_trial_preconditions.py (the conditions on these inputs, on the CPU) and
tests/test_gpu_polar_trial_matrix.py (the device against the restatements and the oracle).  Needs no device.

  boxes      polar_ragged_boxes.box: 257 atoms (five tiles, the last with one atom, orthorhombic, kmax 5), 512 (exactly eight, triclinic,
             kmax 3), 513 (nine, cubic, kmax 7) and the two 1089-atom slabs (18 tiles)
  configs    CONFIGS: the box's base options plus a few lines each, with the short iteration counts of polar_ragged_boxes.VARIANTS; every
             one of them takes the delta path (none has wolf electrostatics, the direct solve, polar_ewald_full or polar_gs_ranked)
  moves      by index ranges and seeds.  Whole molecules move rigidly (the ragged boxes have sites 0.1 A apart inside molecules: per-atom
             noise would change that chemistry); one seeded normal vector per molecule.
  references restated(): polar_relax_ref.solve (Jacobi, Gauss-Seidel, sor, esor, zodid) or polar_wolf_ref.solve (the Wolf field) on the
             static field of the configuration, kept per (box, configuration, positions); oracle(): the oracle's energy of the
             configurations it knows (ORACLE_KNOWS); others(): the oracle with polarization off, for the other components of the rest.

The slabs in list order: a tile is 64 consecutive atoms, 1.3 layers of the 7 x 7 x 23 lattice (spacing 3.6 A, 1089 of 1127 sites filled, so the
last 38 sites of the top layer are vacant).  k_tile_bounds wraps the fractional coordinates into [0, 1) counted from the origin of the
spatial sort, which is zero when nothing is sorted; the slab's raw fractional z runs from -0.479 to 0.479, so tiles 8 and 9, whose layers lie
on both sides of z = 0, span the whole period in wrapped z and have no far tile pair to lose.  The long jump therefore takes its mover from
tile 4 (JUMPER), whose wrapped z extent is compact and whose tile pairs with tiles 0, 16 and 17 lie beyond both thresholds.  Under the spatial
order (spatial_order(): the nested bisection, 3 slabs in x, 2 strips in y, 3 tiles in z) a tile spans a third of the period in z and the only
far tile pairs are the five of the lone atom of tile 17; JUMPER sits in tile 7 there, one of the five, and its jump takes that pair's class away.
"""
import hashlib
import re

import numpy as np

import util  # (first: it puts the oracle on the path, which the restatements import)
import polar_ragged_boxes as B
import polar_relax_ref as rx
import polar_wolf_ref as pw

TILE = B.TILE
SIGMA = 0.12            # A, rigid translations of whole molecules in the large moves
SIGMA_ONE = 0.3         # A, one-molecule and one-atom moves (util.moved's)
TRIAL_MAX = 256         # MPMC_TRIAL_MAX_ATOMS: longer moves are evaluated in full
LATTICE = (7, 7, 23)    # sites of the slab's lattice; spacing 3.6 A
SLAB_N = 1089

RAGGED = (257, 512, 513)
SLABS = B.SLABS

# ---- configurations: (options on top of the box's, System.configure pairs) -------------------------------------------------------------------
V = B.VARIANTS
CONFIGS = {
    "jac_mf": ({"solver": "matrix_free"}, ()),
    "jac_compact": ({"solver": "compact"}, ()),
    # the dense solve over the whole matrix, and the one that reads the upper block triangle only (the library's default)
    "jac_dense": ({"solver": "dense"}, (("dense_symmetric", 0),)),
    "jac_dense_sym": ({"solver": "dense"}, (("dense_symmetric", 1),)),
    "jac_gamma": ({"polar_gamma": 1.03}, ()),
    "jac_rrms": ({"polar_rrms": 1}, ()),
    "gs": ({"polar_gs": 1}, ()),
    "gs_nopbc": ({"polar_gs": 1, "polar_ewald": 0}, ()),
    "gs_sor": ({"polar_gs": 1, "polar_sor": 1, "polar_gamma": 0.8, "polar_max_iter": 5}, ()),
    "jac_sor": (V["jac_sor"], ()),
    "wolf_jac": (V["wolf_jac"], ()),
    "wolf_gsp": (V["wolf_gsp"], ()),
    "zodid": (V["zodid"], ()),
    # precision-terminated, on the slabs only (as in the ragged ladder)
    "jac_prec": ({"polar_precision": 1e-4}, ()),
    "gs_prec": ({"polar_gs": 1, "polar_precision": 1e-4}, ()),
    "jac_esor_prec": (V["jac_esor_prec"], ()),
}
FIXED = tuple(k for k in CONFIGS if not k.endswith("_prec"))
PRECISION = tuple(k for k in CONFIGS if k.endswith("_prec"))
ORACLE_KNOWS = ("jac_mf", "jac_compact", "jac_dense", "jac_dense_sym", "jac_gamma", "jac_rrms", "gs", "gs_nopbc", "jac_prec", "gs_prec")
RELAXED = ("gs_sor", "jac_sor", "zodid", "jac_esor_prec")  # polar_relax_info's counters apply
EIGHT_TILE_CONFIGS = ("jac_mf", "jac_compact", "jac_dense", "jac_dense_sym", "gs", "jac_sor", "wolf_jac")
FLIP_CONFIGS = ("jac_mf", "jac_compact", "jac_dense", "jac_dense_sym", "gs", "jac_sor", "wolf_jac", "jac_esor_prec")
TRICLINIC_SLAB_CONFIGS = ("jac_compact", "gs", "wolf_jac", "jac_esor_prec")


def family(cfg):
    return "wolf" if cfg.startswith("wolf") else "relax"


def reference_name(cfg):
    """the four solver settings of the plain Jacobi solve are one configuration to the references"""
    return "jac" if cfg in ("jac_mf", "jac_compact", "jac_dense", "jac_dense_sym") else cfg


def keeps_list_order(cfg):
    """Gauss-Seidel sweeps run in the atom order: such a context never sorts, whatever spatial_sort says"""
    return bool(CONFIGS[cfg][0].get("polar_gs"))


def options(rung, cfg):
    """what the System is created with"""
    return dict(B.box(rung)[2], **CONFIGS[cfg][0])


def reference_options(rung, cfg):
    """... and what the references read: `solver` chooses kernels, not numbers"""
    return {k: v for k, v in options(rung, cfg).items() if k != "solver"}


def sequence_configs(rung):
    if rung == 257:
        return FIXED
    return FIXED + PRECISION if rung == SLABS[0] else TRICLINIC_SLAB_CONFIGS


# ---- moves ---------------------------------------------------------------------------------------------------------------------------------
def whole_molecules(atoms, lo, hi, most=TRIAL_MAX):
    """[a, b): the longest run of whole molecules inside [lo, hi) that starts at the first molecule at or behind lo, at most `most` atoms"""
    mols = util.molecules(atoms)
    a = min(s for s, e in mols if s >= lo)
    b = max(e for s, e in mols if e <= hi and s >= a and e - a <= most)
    return a, b


def whole_molecules_of(atoms, lo, count):
    """[a, a + count): the first run of whole molecules of exactly `count` atoms that starts at or behind lo"""
    mols = util.molecules(atoms)
    ends = {e for _, e in mols}
    a = min(s for s, _ in mols if s >= lo and s + count in ends)
    return a, a + count


def molecule_at(atoms, i):
    return next((s, e) for s, e in util.molecules(atoms) if s <= i < e)


def rigid(atoms, pos, a, b, seed, sigma=SIGMA):
    """trial positions of atoms [a, b) of the configuration `pos`: every molecule translated by its own seeded normal vector"""
    rng = np.random.default_rng(seed)
    new = pos[a:b].copy()
    for s, e in util.molecules(atoms):
        if s >= a and e <= b:
            new[s - a:e - a] += rng.normal(scale=sigma, size=3)
    return new


def jitter(pos, i, seed, sigma=SIGMA_ONE):
    """one atom, util.moved's seeded normal noise"""
    return pos[i:i + 1] + np.random.default_rng(seed).normal(scale=sigma, size=(1, 3))


def applied(pos, first, new):
    out = pos.copy()
    out[first:first + len(new)] = new
    return out


def lone_movable_polarizable(atoms, i):
    """atom i is a molecule of its own, not frozen, polarizable and charged"""
    s, e = molecule_at(atoms, i)
    return e - s == 1 and not atoms["frozen"][i] and atoms["polarizability"][i] != 0.0


# (a) the sequence of every (configuration, box): [(label, first, new positions, accept)], each move made from the positions accepted so far
SEQUENCE = {  # rung: (molecule at or behind this index, rejected; ... accepted; first index of the 65-atom run; the frozen atom's molecule)
    257: (20, 193, 100),
    SLABS[0]: (100, 900, 400),
    SLABS[1]: (100, 900, 400),
}


def first_frozen(atoms):
    """a frozen atom: of a one-site molecule where the box has one, the first frozen atom otherwise"""
    fr = np.nonzero(np.asarray(atoms["frozen"]))[0]
    lone = [i for i in fr if molecule_at(atoms, i)[1] - molecule_at(atoms, i)[0] == 1]
    return int(lone[0] if lone else fr[0])


def sequence(rung):
    atoms = B.box(rung)[0]
    lo_rej, lo_acc, lo_65 = SEQUENCE[rung]
    pos = atoms["pos"].copy()
    steps = []
    a, b = molecule_at(atoms, min(s for s, _ in util.molecules(atoms) if s >= lo_rej))
    steps.append(("one molecule, rejected", a, rigid(atoms, pos, a, b, 41, SIGMA_ONE), False))
    a, b = molecule_at(atoms, min(s for s, _ in util.molecules(atoms) if s >= lo_acc))
    steps.append(("one molecule, accepted", a, rigid(atoms, pos, a, b, 42, SIGMA_ONE), True))
    pos = applied(pos, a, steps[-1][2])
    a, b = whole_molecules_of(atoms, lo_65, 65)
    steps.append(("65 atoms, accepted", a, rigid(atoms, pos, a, b, 43), True))
    pos = applied(pos, a, steps[-1][2])
    f = first_frozen(atoms)
    steps.append(("one frozen atom, rejected", f, jitter(pos, f, 44, SIGMA), False))
    return steps


# (b) the large moves of the boxes of exactly eight and of nine tiles: (bounds of the rejected move, bounds of the accepted one)
LARGE = {512: ((60, 262), (300, 512)), 513: ((60, 262), (320, 513))}
LARGE_EXPECTED = {512: ((63, 262), (300, 512)), 513: ((63, 261), (320, 513))}


def lone_atom_of_tile(atoms, tile):
    """the first movable polarizable one-site molecule of a tile of the list order"""
    return next(i for i in range(tile * TILE, (tile + 1) * TILE) if lone_movable_polarizable(atoms, i))


def large_moves(rung):
    """[(first, new positions, accept)]: the first large move rejected, the second accepted, then one atom of tile 0 accepted and one
    atom of tile 7 accepted (every tile pair of tile 7 but its own has it as the SECOND tile of the pair)"""
    atoms = B.box(rung)[0]
    pos = atoms["pos"].copy()
    (a1, b1), (a2, b2) = (whole_molecules(atoms, *r) for r in LARGE[rung])
    steps = [(a1, rigid(atoms, pos, a1, b1, 4), False), (a2, rigid(atoms, pos, a2, b2, 5), True)]
    pos = applied(pos, a2, steps[-1][1])
    for tile, seed in ((0, 6), (7, 7)):
        i = lone_atom_of_tile(atoms, tile)
        steps.append((i, jitter(pos, i, seed), True))
        pos = applied(pos, i, steps[-1][1])
    return steps


def tiles_of(a, b):
    return sorted({k // TILE for k in range(a, b)})


# (c) the slabs
JUMPER = 304      # tile 4 of the list order, tile 7 of the spatial order
BYSTANDER = 650   # tile 10: far from both ends of the jump
HOP_TILE = {2: 12, 0: 8}  # the hopper's tile: of the list order for a hop along the third cell vector, of the spatial order along the first


def vacancy(rung, exclude=()):
    """(position, clearance): the vacant lattice site of the top layer farthest from any atom (the atoms `exclude` apart)"""
    atoms, basis, _ = B.box(rung)
    pos = np.delete(atoms["pos"], list(exclude), axis=0)
    R = np.linalg.inv(basis)
    nx, ny, nz = LATTICE
    best = None
    for k in range(SLAB_N, nx * ny * nz):
        layer, rem = divmod(k, nx * ny)
        iy, ix = divmod(rem, nx)
        p = np.array([(ix + 0.5) / nx - 0.5, (iy + 0.5) / ny - 0.5, (layer + 0.5) / nz - 0.5]) @ basis
        d = (pos - p) @ R
        d -= np.rint(d)
        m = float(np.sqrt(((d @ basis) ** 2).sum(axis=1)).min())
        if best is None or m > best[1]:
            best = (p, m)
    return best


def hop_order(rung, axis):
    """(perm, origin) of the order the hop along `axis` is made for: hop_axis() sends the first cell vector to the contexts under the spatial
    order and the third to those in list order"""
    atoms, basis, _ = B.box(rung)
    return spatial_order(atoms["pos"], basis) if axis == 0 else (np.arange(len(atoms["pos"])), np.zeros(3))


def hopper(rung, axis):
    """the atom of tile HOP_TILE[axis] of that order with the largest raw fractional coordinate along `axis` among the tile's lone movable
    polarizable atoms"""
    atoms, basis, _ = B.box(rung)
    f = atoms["pos"] @ np.linalg.inv(basis)
    perm = hop_order(rung, axis)[0]
    ok = [int(i) for i in perm[HOP_TILE[axis] * TILE:(HOP_TILE[axis] + 1) * TILE] if lone_movable_polarizable(atoms, int(i))]
    return max(ok, key=lambda i: f[i, axis])


def flip_positions(rung):
    """the configurations of the class-flip scenario: {"start", "jumped" (the long jump from start), "nudged" (the bystander's jitter from
    start), "nudged_jumped" (the long jump from nudged)}, and the two single-atom moves as (first, new positions)"""
    atoms = B.box(rung)[0]
    p0 = atoms["pos"].copy()
    site = vacancy(rung)[0].reshape(1, 3)
    nudge = jitter(p0, BYSTANDER, 45)
    p1 = applied(p0, BYSTANDER, nudge)
    return {"start": p0, "jumped": applied(p0, JUMPER, site), "nudged": p1, "nudged_jumped": applied(p1, JUMPER, site)}, site, nudge


def hop_axis(cfg, sort):
    """the cell vector of the lattice hop.  Under the spatial order a tile is compact in every dimension and the hop goes along the first
    cell vector.  In list order a slab tile spans the cell in x and y (its raw x range, 21.7 A of 25.2, already has two images against
    every other tile), so a hop along x has no common image to take away: there it goes along the third."""
    return 0 if sort and not keeps_list_order(cfg) else 2


def hop_positions(rung, axis):
    """(atom, its position one cell vector `axis` further, the configuration with it, a one-molecule move behind it as (first, new))"""
    atoms, basis, _ = B.box(rung)
    p0 = atoms["pos"].copy()
    i = hopper(rung, axis)
    new = p0[i:i + 1] + basis[axis][None, :]
    ph = applied(p0, i, new)
    a, b = molecule_at(atoms, 100)
    return i, new, ph, (a, rigid(atoms, ph, a, b, 46, SIGMA_ONE))


# ---- the classes of the list order in an orthorhombic cell, as k_tile_bounds and k_classify form them ----------------------------------------
def thole_far_x():
    found = re.findall(r"\bkTholeFarX\s*=\s*([0-9.]+)\s*;", util.csrc_text("kernels.h"))
    assert len(found) == 1, found
    return float(found[0])


def wrapped_extents(pos, basis, perm=None, origin=0.0):
    """[tiles, 2, 3]: min and max per tile of the fractional coordinates wrapped into [0, 1) counted from `origin` (zero: nothing is
    sorted); perm: the order whose tiles are meant (the list order if None)"""
    f = pos @ np.linalg.inv(basis) - origin
    w = f - np.floor(f)
    w = w if perm is None else w[perm]
    nt = -(-len(pos) // TILE)
    return np.array([[w[t * TILE:(t + 1) * TILE].min(axis=0), w[t * TILE:(t + 1) * TILE].max(axis=0)] for t in range(nt)])


def raw_ranges(pos, basis, perm=None):
    """[tiles, 2, 3]: min and max per tile of the raw fractional coordinates; perm: the order whose tiles are meant (the list order if None)"""
    f = pos @ np.linalg.inv(basis)
    f = f if perm is None else f[perm]
    nt = -(-len(pos) // TILE)
    return np.array([[f[t * TILE:(t + 1) * TILE].min(axis=0), f[t * TILE:(t + 1) * TILE].max(axis=0)] for t in range(nt)])


def circle_gap(a0, a1, b0, b1):
    """distance of the intervals [a0, a1] and [b0, b1] on the unit circle (k_classify's, without its 1e-12 rounding guard)"""
    if a1 < b0:
        return min(b0 - a1, a0 + 1.0 - b1)
    if b1 < a0:
        return min(a0 - b1, b0 + 1.0 - a1)
    return 0.0


def tile_gaps(pos, basis, tile):
    """the lower bound of the distance of `tile` from every tile in an orthorhombic cell: sqrt(sum_d (L_d gap_d)^2)"""
    ext = wrapped_extents(pos, basis)
    L = np.abs(np.diag(basis))
    out = []
    for t in range(len(ext)):
        g = [circle_gap(ext[tile, 0, d], ext[tile, 1, d], ext[t, 0, d], ext[t, 1, d]) for d in range(3)]
        out.append(float(np.sqrt(sum((L[d] * g[d]) ** 2 for d in range(3)))))
    return np.array(out)


def class_counts(pos, basis, cutoff, damp):
    """(tile pairs beyond the Thole far range, tile pairs beyond the cutoff) of the list order in an orthorhombic cell"""
    nt = -(-len(pos) // TILE)
    far = beyond = 0
    for t in range(nt):
        g = tile_gaps(pos, basis, t)[t + 1:]
        far += int((g > thole_far_x() / damp).sum())
        beyond += int((g > cutoff).sum())
    return far, beyond


# ---- ... and of the spatial order of boxes below the aligned grid's size (compute_spatial_order's nested bisection, csrc/context.cpp) ---------
def spatial_order(pos, basis):
    """(perm, origin): slot k holds atom perm[k]; the fractional coordinates are counted from their minimum.  nx slabs in x, ny strips in
    y per slab, z order inside a strip, ties by index"""
    n = len(pos)
    f = pos @ np.linalg.inv(basis)
    origin = f.min(axis=0)
    w = f - origin
    w -= np.floor(w)
    T = -(-n // TILE)
    nx = max(1, int(np.floor(np.cbrt(T) + 0.5)))
    per_slab = -(-T // nx)
    ny = max(1, int(np.floor(np.sqrt(per_slab) + 0.5)))
    slab, strip = per_slab * TILE, -(-per_slab // ny) * TILE
    perm = sorted(range(n), key=lambda i: (w[i, 0], i))
    for s0 in range(0, n, slab):
        s1 = min(n, s0 + slab)
        perm[s0:s1] = sorted(perm[s0:s1], key=lambda i: (w[i, 1], i))
        for t0 in range(s0, s1, strip):
            t1 = min(s1, t0 + strip)
            perm[t0:t1] = sorted(perm[t0:t1], key=lambda i: (w[i, 2], i))
    return np.array(perm), origin


def ordered_class_counts(pos, basis, perm, origin, cutoff, damp):
    """(far, beyond) over the tile pairs of the order `perm`, any cell: k_classify's bound -- orthorhombic: sum_d (L_d gap_d)^2; otherwise
    max(max_d (gap_d / |R_d|)^2, lambda_min(B B^T) |gap|^2)"""
    n = len(pos)
    R = np.linalg.inv(basis)
    w = pos @ R - origin
    w = (w - np.floor(w))[perm]
    nt = -(-n // TILE)
    lo = np.array([w[t * TILE:(t + 1) * TILE].min(axis=0) for t in range(nt)])
    hi = np.array([w[t * TILE:(t + 1) * TILE].max(axis=0) for t in range(nt)])
    ortho = not np.any(basis - np.diag(np.diag(basis)))
    plane = 1.0 / np.sqrt((R * R).sum(axis=0))
    lam = float(np.linalg.eigvalsh(basis @ basis.T).min())
    far = beyond = 0
    for i in range(nt):
        for j in range(i + 1, nt):
            g = np.array([max(0.0, circle_gap(lo[i, d], hi[i, d], lo[j, d], hi[j, d]) - 1e-12) for d in range(3)])
            d2 = float(((np.abs(np.diag(basis)) * g) ** 2).sum()) if ortho else max(float((g * plane).max()) ** 2, lam * float((g * g).sum()))
            far += int(d2 > (thole_far_x() / damp) ** 2)
            beyond += int(d2 > cutoff * cutoff)
    return far, beyond


def cutoff_of(basis):
    from oracle import pbc_update

    return pbc_update(basis)[2]


def min_intermolecular(atoms, basis, pos):
    R = np.linalg.inv(basis)
    d = (pos[:, None, :] - pos[None, :, :]) @ R
    d -= np.rint(d)
    r = np.sqrt(((d @ basis) ** 2).sum(axis=-1))
    mol = np.asarray(atoms["mol_id"])
    return float(r[mol[:, None] != mol[None, :]].min())


# ---- references, each computed once per process ------------------------------------------------------------------------------------------------
_fields, _solved, _oracle, _others = {}, {}, {}, {}


def _key(pos):
    return hashlib.sha1(np.ascontiguousarray(pos, dtype=np.float64).tobytes()).hexdigest()


def field_of(rung, cfg, pos):
    atoms, basis, _ = B.box(rung)
    o = reference_options(rung, cfg)
    kind = "wolf" if o.get("polar_wolf") and not o["polar_ewald"] else ("ewald" if o["polar_ewald"] else "nopbc")
    k = (rung, kind, _key(pos))
    if k not in _fields:
        _fields[k] = rx.static_field(util.with_positions(atoms, pos), basis, o)
    return _fields[k]


def solve(rung, cfg, pos, E0):
    atoms, basis, _ = B.box(rung)
    fn = pw.solve if family(cfg) == "wolf" else rx.solve
    return fn(util.with_positions(atoms, pos), basis, reference_options(rung, cfg), E0=E0)


def restated(rung, cfg, pos):
    """the restatement's solve of the configuration `pos` of the box under cfg"""
    k = (rung, reference_name(cfg), _key(pos))
    if k not in _solved:
        _solved[k] = solve(rung, cfg, pos, field_of(rung, cfg, pos))
    return _solved[k]


def oracle(rung, cfg, pos):
    """the oracle's energy() of the configuration, with the per-atom arrays, for a configuration of ORACLE_KNOWS"""
    assert cfg in ORACLE_KNOWS, cfg
    k = (rung, reference_name(cfg), _key(pos))
    if k not in _oracle:
        atoms, basis, _ = B.box(rung)
        _oracle[k] = util.oracle_energy(util.with_positions(atoms, pos), basis, reference_options(rung, cfg))
    return _oracle[k]


def others(rung, cfg, pos):
    """the oracle with polarization off: every component but the polarization energy"""
    k = (rung, _key(pos))
    if k not in _others:
        atoms, basis, _ = B.box(rung)
        _others[k] = util.oracle_energy(util.with_positions(atoms, pos), basis, util.nonpolar(reference_options(rung, cfg)))
    return _others[k]


def compared_configurations(rung):
    """[(label, cfg, positions)]: every accepted and every trial configuration tests/test_gpu_polar_trial_matrix.py compares on this box"""
    atoms = B.box(rung)[0]
    out = []
    if rung in SEQUENCE:
        pos = atoms["pos"].copy()
        shapes = [("start", pos)]
        for label, first, new, accept in sequence(rung):
            trial = applied(pos, first, new)
            shapes.append((label, trial))
            pos = trial if accept else pos
        out += [(f"sequence: {label}", cfg, p) for cfg in sequence_configs(rung) for label, p in shapes]
    if rung in LARGE:
        pos = atoms["pos"].copy()
        shapes = []
        for k, (first, new, accept) in enumerate(large_moves(rung)):
            trial = applied(pos, first, new)
            shapes.append((f"large move {k}", trial))
            pos = trial if accept else pos
        out += [(label, cfg, p) for cfg in EIGHT_TILE_CONFIGS for label, p in shapes]
    if rung in SLABS:
        flips = flip_positions(rung)[0]
        for cfg in FLIP_CONFIGS:
            out += [(f"flip: {label}", cfg, p) for label, p in flips.items()]
            for axis in sorted({hop_axis(cfg, 0), hop_axis(cfg, 1)}):
                _, _, ph, (a, new) = hop_positions(rung, axis)
                out += [(f"hop along {axis}", cfg, ph), (f"one molecule behind the hop along {axis}", cfg, applied(ph, a, new))]
    return out
