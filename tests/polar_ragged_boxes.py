"""The boxes, the variants and the restatements of the ragged-size ladder of the dipole-solve variants: `polar_ewald_full`, the Wolf static
field, the relaxed Jacobi updates and `polar_zodid`.  Shared by tests/test_polar_ragged_preconditions.py (the conditions on these inputs,
on the CPU) and tests/test_gpu_polar_ragged_ladder.py (the device against the restatements).  Needs no device.

  ragged rungs   test_gpu_random.random_system at 1, 2, 63, 64, 65, 128, 129, 257, 512 and 513 atoms with one fixed seed each: 30 % of the
                 atoms with alpha = 0, 25 % without a charge, 15 % of the molecules frozen, molecules of 1 to 4 sites, unwrapped positions;
                 the cell cycles through cubic / orthorhombic / triclinic and ewald_kmax through 7 / 5 / 3 (709, 257 and 61 k vectors).  At
                 n <= 2 every atom is made polarizable: a lone non-polarizable atom tests nothing.  The seeds are chosen (and the choice is
                 asserted by the CPU file) so that the lone atom of the last tile is polarizable at 65 and 257 atoms and non-polarizable at
                 129 and 513: there, in list order, every tile pair with the last tile holds no pair of polarizable atoms.
  slab rungs     gen_box's slab1089_planted and slab1089_planted_tri: 25.2 x 25.2 x 82.8 A, cutoff 12.6 A, 18 tiles, the last with one atom

Every restatement is solved once per process and kept (restated); the static field of a box is kept too, so that the variants of one box
and the perturbed solves of the conditioning test share it.
"""
import tempfile

import numpy as np

import util  # (first: it puts the oracle on the path, which the restatements import)
import polar_ewald_full_ref as pef
import polar_relax_ref as rx
import polar_wolf_ref as pw
from test_gpu_random import random_system

RAGGED = (1, 2, 63, 64, 65, 128, 129, 257, 512, 513)
CELLS = ("cubic", "ortho", "triclinic")
KMAX = (7, 5, 3)
N_K = {7: 709, 5: 257, 3: 61}
SEEDS = {1: 5001, 2: 8002, 63: 5063, 64: 5064, 65: 5065, 128: 5128, 129: 7129, 257: 7257, 512: 5512, 513: 11513}
LONE_ATOM_POLARIZABLE = {65: True, 129: False, 257: True, 513: False}  # the one atom of the last tile
SLABS = ("slab1089_planted", "slab1089_planted_tri")
TILE = 64

BASE = {"rd_only": 0, "rd_lrc": 1, "polarization": 1, "polar_iterative": 1, "polar_ewald": 1, "polar_max_iter": 3, "polar_gs": 0, "polar_rrms": 0,
        "ewald_kmax": 7, "polar_precision": 0.0, "polar_gamma": 1.0, "polar_damp": 2.1304, "damp_type": "exponential", "ewald_alpha": None,
        "polar_ewald_alpha": None}
WOLF = {"polar_ewald": 0, "polar_wolf": 1, "polar_wolf_alpha": 0.13}  # (the polar_wolf_alpha of gen_box's WOLF_FIXTURES)
# the iteration counts are short on purpose: at this damping the random mix diverges under ten Jacobi iterations (max |mu| 5.7e5 at 513
# atoms in the restatement) and is well conditioned at three to six
VARIANTS = {
    "pef": {"polar_ewald_full": 1, "polar_max_iter": 3},  # four passes
    "pef_sor": {"polar_ewald_full": 1, "polar_sor": 1, "polar_gamma": 0.8, "polar_max_iter": 5},
    "jac_sor": {"polar_sor": 1, "polar_gamma": 0.8, "polar_max_iter": 6},
    "zodid": {"polar_zodid": 1, "polar_gamma": 1.03},
    "wolf_jac": dict(WOLF, polar_max_iter=3),
    "wolf_gsp": dict(WOLF, polar_gs=1, polar_palmo=1, polar_max_iter=3),
    # precision-terminated, on the slab rungs only
    "pef_prec": {"polar_ewald_full": 1, "polar_precision": 1e-4},
    "pef_esor_prec": {"polar_ewald_full": 1, "polar_esor": 1, "polar_gamma": 0.7, "polar_precision": 1e-4},
    "jac_esor_prec": {"polar_esor": 1, "polar_gamma": 0.6, "polar_precision": 1e-4, "polar_rrms": 1},
}
RAGGED_VARIANTS = ("pef", "pef_sor", "jac_sor", "zodid", "wolf_jac", "wolf_gsp")
SLAB_VARIANTS = ("pef", "pef_sor", "jac_sor", "zodid", "pef_prec", "pef_esor_prec", "jac_esor_prec")  # (the Gauss-Seidel ladder has the Wolf field there)
# whose restatement, and so whose bounds: polar_ewald_full_ref, polar_relax_ref, polar_wolf_ref
FAMILY = {"pef": "pef", "pef_sor": "relax", "jac_sor": "relax", "zodid": "relax", "wolf_jac": "wolf", "wolf_gsp": "wolf", "pef_prec": "pef",
          "pef_esor_prec": "relax", "jac_esor_prec": "relax"}
CASES = [(n, v) for n in RAGGED for v in RAGGED_VARIANTS] + [(s, v) for s in SLABS for v in SLAB_VARIANTS]

_boxes, _fields, _solved, _oracle = {}, {}, {}, {}


def box(rung):
    """(atoms, basis, base options) of a rung: an atom count of RAGGED or a name of SLABS"""
    if rung not in _boxes:
        if rung in SLABS:
            with tempfile.TemporaryDirectory() as d:  # (gen_box writes the reference's input files; the reader takes them whole)
                atoms, basis, o = util.load_generated(rung, d)
            assert o["polar_gs"] == 1 and o["polar_damp"] == BASE["polar_damp"] and len(atoms["charge"]) == 1089
            _boxes[rung] = atoms, np.asarray(basis, dtype=np.float64), dict(o, polar_gs=0, polar_max_iter=BASE["polar_max_iter"])
        else:
            k = RAGGED.index(rung)
            atoms, basis = random_system(np.random.default_rng(SEEDS[rung]), rung, CELLS[k % 3])
            if rung <= 2:
                atoms["polarizability"] = np.where(atoms["polarizability"] == 0.0, 0.8, atoms["polarizability"])
            _boxes[rung] = atoms, basis, dict(BASE, ewald_kmax=KMAX[k % 3])
    return _boxes[rung]


def options(rung, variant):
    return dict(box(rung)[2], **VARIANTS[variant])


def prefix(atoms, m):
    """the first m atoms of a list (random_system builds it molecule by molecule, so a prefix keeps its molecules contiguous)"""
    return {k: np.array(v[:m]) for k, v in atoms.items()}


def static_field(atoms, basis, o):
    return rx.static_field(atoms, basis, o)


def solve(variant, atoms, basis, o, E0):
    """the variant's restatement on the static field E0, with the pass count of the polar_ewald_full variants under "passes" whichever
    restatement solved them"""
    fam = FAMILY[variant]
    r = {"pef": pef.solve, "relax": rx.solve, "wolf": pw.solve}[fam](atoms, basis, o, E0=E0)
    if fam == "relax" and o.get("polar_ewald_full"):
        r["passes"] = r["contractions"]
    if fam == "pef":
        r["polar_iterations"] = 0
    return r


def field_of(rung, variant):
    """E0 of the rung under the variant's static field (Ewald or Wolf), computed once"""
    atoms, basis, _ = box(rung)
    o = options(rung, variant)
    key = (rung, "wolf" if o.get("polar_wolf") and not o["polar_ewald"] else "ewald")
    if key not in _fields:
        _fields[key] = static_field(atoms, basis, o)
    return _fields[key]


def restated(rung, variant):
    """the restatement's solve of (rung, variant), computed once per process"""
    if (rung, variant) not in _solved:
        atoms, basis, _ = box(rung)
        _solved[rung, variant] = solve(variant, atoms, basis, options(rung, variant), field_of(rung, variant))
    return _solved[rung, variant]


def oracle_without_polarization(rung):
    """the oracle's energy of the rung with polarization off: what every component but the polarization energy is held to"""
    if rung not in _oracle:
        atoms, basis, o = box(rung)
        _oracle[rung] = util.oracle_energy(atoms, basis, util.nonpolar(o))
    return _oracle[rung]


def predicate(atoms, basis, o):
    """[n, n] bool: the pairs inside the real-space predicate of polar_ewald_full (both polarizable, !(r > R)), as real_tensor states it"""
    bx = pef.Box(atoms, basis, o)
    pol = bx.alpha != 0.0
    return ~np.eye(bx.n, dtype=bool) & pol[:, None] & pol[None, :] & ~(bx.r > bx.cutoff)


def empty_tile_pairs(ok):
    """(tile pairs I <= J of the list order, those without a pair inside `ok`, those of them off the diagonal)"""
    n = ok.shape[0]
    nt = -(-n // TILE)
    empty = off = 0
    for i in range(nt):
        for j in range(i, nt):
            if not ok[i * TILE:(i + 1) * TILE, j * TILE:(j + 1) * TILE].any():
                empty += 1
                off += int(i != j)
    return nt * (nt + 1) // 2, empty, off
