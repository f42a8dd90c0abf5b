"""The boxes, scale factors and restatements of the volume-trial follow-ups: what a volume trial (mpmc_trial_volume_begin, csrc/trial.cpp)
leaves for the calls behind it.  Shared by tests/test_gpu_volume_trial.py (the move itself), tests/test_volume_trial_preconditions.py (the
conditions on these inputs, on the CPU) and tests/test_gpu_volume_trial_followups.py (the device).  Needs no device.

  restatement   host_scale(): System::volume_change in Python floats, the one restatement of the move in the suite
  lattice boxes sorted129 (129 atoms: three tiles, the last with one atom, one atom above the spatial sort's n > 2 kTile) and edge190 (190
                atoms, padded to 192; one 3-atom molecule more makes 193 atoms padded to 256): one- and three-atom molecules with unequal
                masses on a partly filled cubic lattice, LJ + Ewald.  The vacant sites are the insertion points.
  polarizable   polar_trial_cases.RAGGED rungs 257 and 513 under POLAR_CONFIGS, the ion fixture under jac_esor_prec, and EXTRA_SOLVES: the solves without an entry in
                polar_trial_cases.CONFIGS (polar_ewald_full, the direct solve, polar_gs_ranked), each on a committed fixture
  term boxes    TERM_FIXTURES (rd_crystal, an rd model, sg, Axilrod-Teller, disp-expansion, polar_ewald_full, Gauss-Seidel, the direct
                solve, Wolf); FROZEN: ion216_frozen and ion216_framework
  slab          polar_trial_cases.SLABS[0], the orthorhombic 1089-atom slab, at FLIP_SCALE

FLIP_SCALE is found by flip_search(): the first scale of 1 -/+ k / 200, k = 1 .. 20, at which the restated tile-pair class counts (far, beyond)
of the list order differ between the accepted and the scaled slab.  Under the spatial order of a fresh context NO scale of [0.9, 1.1]
changes the counts, and none can: the slab has 999 one-site molecules, whose fractional coordinates a volume move leaves alone, and the
cutoff scales with the cell, so the beyond-cutoff count is the accepted one at every scale; the Thole far range kTholeFarX / polar_damp =
14.08 A does not scale, but the five far tile pairs of that order (the lone atom of tile 17) lie further than 14.08 / 0.9 A apart and every
other pair within the cutoff of 12.6 A, 13.86 A at 1.1.  tests/test_volume_trial_preconditions.py asserts both halves.
DRIFT_SCALE moves some atom of the 513-atom box further than kResortDrift of context.cpp.
"""
import re
import tempfile

import numpy as np

import util
import polar_ragged_boxes as B
import polar_trial_cases as C

TERM_FIXTURES = ["lj64_rc2", "ion216_triclinic_rdm_ljwh", "h2_64_sg", "water64_at", "water64_disp", "water64_polar_pef", "ion216_gs",
                 "water64_polar_direct", "ion216_wolf"]
FROZEN = ("ion216_frozen", "ion216_framework")
POLAR_RUNGS = (257, 513)
POLAR_CONFIGS = ("jac_mf", "jac_dense_sym", "gs", "jac_sor", "wolf_jac")
# the precision-terminated relaxed solve does not converge on the ragged rungs at any scale, 1.0 included (128 iterations, iterator_failed, as
# polar_trial_cases says of its precision-terminated configurations: "on the slabs only"): it runs on the 216-atom ion fixture, where
# it converges in 5 or 6 iterations at every scale used
PRECISION_BOX, PRECISION_CONFIG = "ion216_polar", "jac_esor_prec"
POLAR_CASES = [(rung, cfg) for rung in POLAR_RUNGS for cfg in POLAR_CONFIGS] + [(PRECISION_BOX, PRECISION_CONFIG)]
# the solves no configuration of polar_trial_cases.CONFIGS reaches (none of them has a delta path): fixture, options on top of its own
EXTRA_SOLVES = {"pef": ("water64_polar_pef", {}), "direct": ("water64_polar_direct", {}), "gs_ranked": ("ion216_gs", {"polar_gs": 0, "polar_gs_ranked": 1})}
SLAB = C.SLABS[0]
REJECT_SCALE, SHRINK, GROW = 1.04, 0.97, 1.04  # case 1; case 2: SHRINK accepted, GROW on top of it
FAR = 2.5  # A: an insertion point is further than this from every atom


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def host_scale(atoms, basis, s):
    """System::volume_change in Python floats: per molecule mass += m_i, cm[p] += m_i * pos_i[p] in atom order, cm[p] /= mass,
    delta[p] = cm[p] * s - cm[p], pos_i[p] += delta[p]; every basis element times s"""
    pos, mass = np.asarray(atoms["pos"], dtype=np.float64), np.asarray(atoms["mass"], dtype=np.float64)
    new = pos.copy()
    for a, b in util.molecules(atoms):
        m, cm = 0.0, [0.0, 0.0, 0.0]
        for i in range(a, b):
            mi = float(mass[i])
            m += mi
            for p in range(3):
                cm[p] += mi * float(pos[i, p])
        for p in range(3):
            cm[p] /= m
            d = cm[p] * s - cm[p]
            for i in range(a, b):
                new[i, p] = float(pos[i, p]) + d
    return new, np.asarray(basis, dtype=np.float64) * s


def scaled(atoms, basis, s):
    """(the atom list at the scaled positions, the scaled basis)"""
    pos, b = host_scale(atoms, basis, s)
    return util.with_positions(atoms, pos), b


# ---- fixtures --------------------------------------------------------------------------------------------------------------------------------
_boxes = {}


def fixture(name):
    """(atoms, basis, options) of a committed or generated fixture, read once per process"""
    if name not in _boxes:
        if name in util.SMALL:
            atoms, basis, opts = util.load_fixture(name)
        else:
            with tempfile.TemporaryDirectory() as d:
                atoms, basis, opts = util.load_generated(name, d)
        _boxes[name] = atoms, np.asarray(basis, dtype=np.float64), opts
    return _boxes[name]


def extra_solve(name):
    fx, extra = EXTRA_SOLVES[name]
    atoms, basis, opts = fixture(fx)
    return atoms, basis, dict(opts, **extra)


def polar_box(key, cfg):
    """(atoms, basis, options) of a case of POLAR_CASES: a ragged rung, or the ion fixture with the configuration's lines on top"""
    if key in POLAR_RUNGS:
        atoms, basis, _ = B.box(key)
        return atoms, basis, C.options(key, cfg)
    atoms, basis, opts = fixture(key)
    return atoms, basis, dict(opts, **C.CONFIGS[cfg][0])


def reference_options(key, cfg):
    """... and what the references read: `solver` chooses kernels, not numbers"""
    return {k: v for k, v in polar_box(key, cfg)[2].items() if k != "solver"}


def is_polarizable(opts):
    """whether a context under these options solves dipoles (sg reads the options with rd_only on and polarization off)"""
    return bool(opts.get("polarization")) and not opts.get("rd_only") and not opts.get("sg")


def insertion_allowed(opts):
    """exchange trials are refused under Axilrod-Teller and disp-expansion coefficients (xch_begin_checks)"""
    return not (opts.get("axilrod_teller") or opts.get("disp_expansion"))


def candidates_allowed(opts):
    """mpmc_insert_candidates has the delta path only: no polarizable box, no rd_crystal, no rd model, no sg"""
    from mpmcxx_amd import energy

    return bool(insertion_allowed(opts) and not is_polarizable(opts) and not opts.get("rd_crystal") and not opts.get("sg") and
                tuple(energy.rd_model_of(opts)) == (0, 0))


# ---- displacement moves ------------------------------------------------------------------------------------------------------------------------
def displacement(atoms, basis, where=0.5, seed=7, sigma=0.3):
    """(first, new positions): the first movable molecule at or behind the fraction `where` of the molecule list, translated rigidly by a
    seeded normal vector -- the first of the seeds seed, seed + 1, ... that leaves its atoms no closer to another molecule than
    min(2.3 A, the closest intermolecular pair of the configuration)"""
    pos = np.asarray(atoms["pos"], dtype=np.float64)
    mols = util.molecules(atoms)
    a, b = next((s, e) for s, e in mols[int(where * len(mols)):] if not np.any(atoms["frozen"][s:e]))
    bound = min(2.3, C.min_intermolecular(atoms, basis, pos))
    R = np.linalg.inv(basis)
    other = np.asarray(atoms["mol_id"]) != atoms["mol_id"][a]
    for k in range(64):
        new = pos[a:b] + np.random.default_rng(seed + k).normal(scale=sigma, size=3)
        d = (pos[other][None, :, :] - new[:, None, :]) @ R
        if float(np.linalg.norm((d - np.rint(d)) @ basis, axis=-1).min()) >= bound:
            return a, new
    raise AssertionError("no seed keeps the mover clear of its neighbours")


def has_delta(opts):
    """whether a displacement trial of a polarizable box under these options takes the polar_delta branch of mpmc_trial_energy_async"""
    return not (opts.get("wolf") or not opts.get("polar_iterative") or opts.get("polar_ewald_full") or opts.get("polar_gs_ranked"))


# ---- the lattice boxes -------------------------------------------------------------------------------------------------------------------------
LATTICE = {"sorted129": (30, 39, 5, 19), "edge190": (60, 10, 6, 23)}  # three-atom molecules, one-atom molecules, sites per edge, seed
SPACING = 4.3     # A
ARM = 0.5         # A: the outer atoms of a three-atom molecule from its central one
REMOVED = 7       # the molecule the list-edit sequence removes (a three-atom one: the first n3 molecules are)


def lattice_box(name):
    """(atoms, basis, options, vacant sites): molecules on a random subset of a cubic lattice, jittered by up to 0.2 A per coordinate; the
    three-atom ones first, neutral (0.2, -0.1, -0.1), the one-atom ones alternating +-0.1 with the last one neutral where their number is
    odd; masses 1.0 + 3.3 (i mod 7)"""
    key = ("lattice", name)
    if key not in _boxes:
        n3, n1, side, seed = LATTICE[name]
        opts = fixture("ion64_es")[2]
        rng = np.random.default_rng(seed)
        sites = np.array([(i, j, k) for i in range(side) for j in range(side) for k in range(side)], dtype=np.float64)
        sites = (sites - (side - 1) / 2.0) * SPACING
        order = rng.permutation(len(sites))
        pos, q, mol = [], [], []
        for m in range(n3 + n1):
            centre = sites[order[m]] + rng.uniform(-0.2, 0.2, size=3)
            if m < n3:
                u = rng.normal(size=(2, 3))
                u /= np.linalg.norm(u, axis=1)[:, None]
                pos += [centre, centre + ARM * u[0], centre + ARM * u[1]]
                q += [0.2, -0.1, -0.1]
                mol += [m] * 3
            else:
                k = m - n3
                pos.append(centre)
                q.append(0.0 if (n1 % 2 and k == n1 - 1) else (0.1 if k % 2 == 0 else -0.1))
                mol.append(m)
        n = len(pos)
        atoms = {"pos": np.array(pos), "charge": np.array(q), "polarizability": np.zeros(n), "epsilon": np.full(n, 50.0), "sigma": np.full(n, 3.0),
                 "mol_id": np.array(mol, dtype=np.int32), "frozen": np.zeros(n, dtype=np.int32), "mass": 1.0 + (np.arange(n) % 7) * 3.3}
        _boxes[key] = atoms, np.eye(3) * side * SPACING, opts, sites[order[n3 + n1:]]
    return _boxes[key]


def new_molecule(atoms, at):
    """a three-atom molecule like the first of the list, its first atom at `at`, heavier than any other"""
    a0, a1 = util.molecules(atoms)[0]
    mol = {k: np.array(v[a0:a1]) for k, v in atoms.items()}
    mol["pos"] = mol["pos"] - mol["pos"][0] + np.asarray(at, dtype=np.float64)
    mol["mass"] = np.array([31.0, 2.5, 7.25])
    return mol


def appended(atoms, mol):
    """the list with `mol` behind its last atom, under a molecule id of its own"""
    out = {k: np.concatenate([atoms[k], mol[k]]) for k in atoms}
    out["mol_id"][len(atoms["mol_id"]):] = int(np.max(atoms["mol_id"])) + 1
    return out


def without(atoms, a, b):
    return {k: np.delete(v, np.s_[a:b], axis=0) for k, v in atoms.items()}


def clearance(atoms, basis, point):
    """the minimum-image distance of `point` from the nearest atom"""
    d = (np.asarray(atoms["pos"]) - point) @ np.linalg.inv(basis)
    return float(np.linalg.norm((d - np.rint(d)) @ basis, axis=1).min())


def far_point(atoms, basis, s, seed):
    """a seeded point further than FAR from every atom of the configuration and of the configuration scaled by s, in each's own cell"""
    rng = np.random.default_rng(seed)
    sc, sb = scaled(atoms, basis, s)
    for _ in range(100000):
        p = (0.5 - rng.random(3)) @ basis
        if clearance(atoms, basis, p) > FAR and clearance(sc, sb, p) > FAR:
            return p
    raise AssertionError("no point that far from every atom")


def list_edit_history(name):
    """The configurations of the list-edit sequence of a lattice box, in the order the device meets them:
    [(label, atoms, basis)]: start; grown (a molecule appended at the first vacant site); grown and scaled by GROW; that with molecule
    REMOVED gone; that scaled by SHRINK (rejected); the accepted one with a molecule appended at the second vacant site times GROW (rejected)"""
    atoms, basis, _, vacant = lattice_box(name)
    grown = appended(atoms, new_molecule(atoms, vacant[0]))
    big, bb = scaled(grown, basis, GROW)
    r0, r1 = util.molecules(big)[REMOVED]
    fewer = without(big, r0, r1)
    shrunk, sb = scaled(fewer, bb, SHRINK)
    again = appended(fewer, new_molecule(fewer, vacant[1] * GROW))
    return [("start", atoms, basis), ("grown", grown, basis), ("scaled", big, bb), ("fewer", fewer, bb), ("shrunk", shrunk, sb), ("again", again, bb)]


# ---- the slab: class counts under a scale -------------------------------------------------------------------------------------------------------
def slab_counts(s):
    """((far, beyond) in list order, (far, beyond) under the spatial order of the ACCEPTED configuration) of the slab scaled by s: the
    atoms keep their slots and the wrap origin through a volume trial"""
    atoms, basis, o = B.box(SLAB)
    perm, origin = C.spatial_order(atoms["pos"], basis)
    pos, b = host_scale(atoms, basis, s) if s != 1.0 else (atoms["pos"], basis)
    cut = C.cutoff_of(b)
    return C.class_counts(pos, b, cut, o["polar_damp"]), C.ordered_class_counts(pos, b, perm, origin, cut, o["polar_damp"])


FLIP_GRID = [1.0 + sign * k / 200.0 for k in range(1, 21) for sign in (-1, 1)]
_flip = []


def flip_search():
    """(FLIP_SCALE, counts at 1.0, counts at FLIP_SCALE): the first scale of FLIP_GRID whose list-order counts differ from the accepted ones"""
    if not _flip:
        start = slab_counts(1.0)
        for s in FLIP_GRID:
            got = slab_counts(s)
            if got[0] != start[0]:
                _flip.append((s, start, got))
                break
        assert _flip, "no scale of the grid changes a class count in list order"
    return _flip[0]


def flip_scale():
    return flip_search()[0]


# ---- drift ----------------------------------------------------------------------------------------------------------------------------------------
DRIFT_RUNG = 513
DRIFT_SCALE = 1.2


def resort_drift():
    """kResortDrift of context.cpp: how far an atom may stand from where it stood at the last sort before a bulk update sorts again"""
    found = re.findall(r"\bkResortDrift\s*=\s*([0-9.]+)\s*;", util.csrc_text("context.cpp"))
    assert len(found) == 1, found
    return float(found[0])


def cell_widths(basis):
    """the distances between opposite faces of the cell"""
    return 1.0 / np.sqrt((np.linalg.inv(basis) ** 2).sum(axis=0))


def nonpolar_rung(rung):
    atoms, basis, o = B.box(rung)
    return atoms, basis, util.nonpolar(o)


# ---- every scaled configuration the GPU file evaluates, for the distance and the conditioning conditions -----------------------------------------
def scaled_boxes():
    """[(label, atoms, basis, scale, scaled atoms, scaled basis)]"""
    out = []

    def add(label, atoms, basis, s):
        sa, sb = scaled(atoms, basis, s)
        out.append((f"{label} x {s}", atoms, basis, s, sa, sb))
        return sa, sb

    for name in TERM_FIXTURES:
        add(name, *fixture(name)[:2], REJECT_SCALE)
    for rung in POLAR_RUNGS + (PRECISION_BOX,):
        atoms, basis, _ = polar_box(rung, PRECISION_CONFIG)
        add(str(rung), atoms, basis, REJECT_SCALE)
        sa, sb = add(str(rung), atoms, basis, SHRINK)
        add(f"{rung} x {SHRINK}", sa, sb, GROW)
    for name in FROZEN:
        for s in (SHRINK, GROW):
            add(name, *fixture(name)[:2], s)
    add(SLAB, *B.box(SLAB)[:2], flip_scale())
    add(str(DRIFT_RUNG), *B.box(DRIFT_RUNG)[:2], DRIFT_SCALE)
    for name in LATTICE:
        for label, atoms, basis in list_edit_history(name):
            if label in ("grown", "fewer"):
                add(f"{name} {label}", atoms, basis, GROW if label == "grown" else SHRINK)
    return out
