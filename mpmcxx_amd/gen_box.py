"""Synthetic periodic boxes for the energy hot path -- TEST/BENCH INPUT GENERATOR.

Pure data generation (no physics): writes the reference's own on-disk formats so that the
reference harness (oracle/_ref/ref_harness) and our loaders (mpmcxx_amd/pqr.py) parse the SAME
text and therefore see bit-identical doubles.

PQR token grammar follows reference src/System.cpp:583-687
  ATOM atom_id atom_type molecule_type FLAG molecule_id x y z mass charge[e] alpha eps sigma omega gwp_alpha
Input-file grammar ("keyword value" per line) follows reference src/SimulationControl.cpp:204-267.

Generators (recipes from SURVEY.md Appendix A):
  lattice_box   : jittered simple-cubic lattice of single-site atoms, alternating +-0.1 e
  molecular_box : rigid 3-site molecules (exclusions, intramolecular erf term) + one neutral
                  polarizable atom (exercises the es_excluded "quirk 2")
"""
from __future__ import annotations

import math
import os
import random
import re
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence


@dataclass
class AtomRow:
    atom_id: int
    atomtype: str
    moltype: str
    flag: str  # M movable / F frozen
    mol_id: int
    x: float
    y: float
    z: float
    mass: float
    charge_e: float
    alpha: float
    eps: float
    sigma: float
    # dispersion coefficients (reference PQR columns 17-20, src/System.cpp:587): only rows that carry them print them
    c6: Optional[float] = None
    c8: Optional[float] = None
    c10: Optional[float] = None
    c9: Optional[float] = None

    def line(self) -> str:
        s = (
            f"ATOM {self.atom_id:6d} {self.atomtype:<4s} {self.moltype:<4s} {self.flag} {self.mol_id:6d} "
            f"{self.x:12.6f} {self.y:12.6f} {self.z:12.6f} {self.mass:9.5f} {self.charge_e:9.5f} "
            f"{self.alpha:8.5f} {self.eps:10.5f} {self.sigma:8.5f} 0.00000 0.00000"
        )
        coef = (self.c6, self.c8, self.c10, self.c9)
        if any(v is not None for v in coef):
            s += "".join(f" {(v or 0.0)!r}" for v in coef)
        return s


def lattice_box(
    n_atoms: int,
    L: float,
    seed: int,
    charged: bool = True,
    alpha: float = 1.6411,
    eps: float = 119.8,
    sigma: float = 3.405,
    charge: float = 0.1,
    frozen_every: int = 0,
) -> List[AtomRow]:
    """Jittered simple-cubic lattice, one atom per molecule, charges +q (odd id) / -q (even id)."""
    n = int(math.ceil(n_atoms ** (1.0 / 3.0) - 1e-9))
    a = L / n
    rng = random.Random(seed)
    rows: List[AtomRow] = []
    k = 0
    for ix in range(n):
        for iy in range(n):
            for iz in range(n):
                if k >= n_atoms:
                    break
                k += 1
                x = (ix + 0.5) * a - L / 2 + rng.uniform(-0.1 * a, 0.1 * a)
                y = (iy + 0.5) * a - L / 2 + rng.uniform(-0.1 * a, 0.1 * a)
                z = (iz + 0.5) * a - L / 2 + rng.uniform(-0.1 * a, 0.1 * a)
                q = (charge if (k % 2 == 1) else -charge) if charged else 0.0
                flag = "F" if (frozen_every and k % frozen_every == 0) else "M"
                rows.append(AtomRow(k, "Ar", "Ar", flag, k, x, y, z, 39.948, q, alpha, eps, sigma))
    return rows


def lattice_box_cell(n_atoms: int, basis, seed: int, charge: float = 0.1, alpha: float = 1.6411, eps: float = 119.8, sigma: float = 3.405) -> List[AtomRow]:
    """Jittered lattice in the FRACTIONAL coordinates of an arbitrary (triclinic) cell, one atom per molecule, charges +-q: atoms fill the
    cell evenly whatever its shape (lattice_box fills a cube, which a skewed cell of another volume wraps onto itself)."""
    n = int(math.ceil(n_atoms ** (1.0 / 3.0) - 1e-9))
    rng = random.Random(seed)
    rows: List[AtomRow] = []
    k = 0
    for ix in range(n):
        for iy in range(n):
            for iz in range(n):
                if k >= n_atoms:
                    break
                k += 1
                f = [(i + 0.5) / n - 0.5 + rng.uniform(-0.1 / n, 0.1 / n) for i in (ix, iy, iz)]
                x, y, z = (sum(f[q] * basis[q][p] for q in range(3)) for p in range(3))
                rows.append(AtomRow(k, "Ar", "Ar", "M", k, x, y, z, 39.948, charge if (k % 2 == 1) else -charge, alpha, eps, sigma))
    return rows


# ---- slab boxes: a long thin cell whose 64-atom tiles, in list order, are slabs about 5 A thick -----------------------------------------------
# 7 x 7 sites per layer, the layers stacked in z, z outermost in the list.  With Gauss-Seidel sweeps (no spatial sort) the tile-pair table of
# such a box has every class: the cutoff is 12.6 A, the Thole far distance 30 / 2.1304 = 14.1 A, and tiles more than half the cell apart
# share a non-zero periodic image in z.
SLAB_SPACING = 3.6
SLAB_SIDE = 7
SLAB_MIN_LAYERS = 23  # 25.2 x 25.2 x 82.8 A; a box of more than 23 layers is longer
SLAB_SKEW = [[1.0, 0.0, 0.0], [0.17, 1.0, 0.0], [-0.12, 0.21, 1.0]]  # the triclinic cell: row q of the orthorhombic basis times this
SLAB_PLANTED = (70, 200, 333, 520, 700, 845, 1000, 1088)  # list indices pulled to 2.0 A from their list predecessor
SLAB_PLANT_AT = (1.2, 1.6, 0.0)
SLAB_THIRD = (201, 200, (0.0, 0.0, 2.0))  # (atom, neighbour, displacement): a second atom 2.0 A from the planted atom 200
SLAB_SHIFTED = 700  # this planted atom (a molecule of its own) is listed one cell vector (the first) away from where it sits
SLAB_JITTER = {"planted": 0.014, "scrambled": 0.25 / SLAB_SPACING}  # in lattice spacings: +-0.05 A and +-0.25 A


def slab_basis(n_atoms: int, triclinic: bool = False):
    per = SLAB_SIDE * SLAB_SIDE
    layers = max(SLAB_MIN_LAYERS, (n_atoms + per - 1) // per)
    edge = [SLAB_SIDE * SLAB_SPACING, SLAB_SIDE * SLAB_SPACING, layers * SLAB_SPACING]
    skew = SLAB_SKEW if triclinic else [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    return [[edge[q] * skew[q][p] for p in range(3)] for q in range(3)], layers


def slab_box(n_atoms: int, variant: str, triclinic: bool = False) -> List[AtomRow]:
    """The first n_atoms sites of the slab lattice, from the same fractional coordinates whatever the cell.  Charges +-30 (reduced units) in
    alternation, about 10 % of the sites with alpha = 0, every 37th site the first of a three-site molecule, every sixth of those frozen.
      planted    jitter +-0.05 A; the atoms SLAB_PLANTED sit 2.0 A (Cartesian SLAB_PLANT_AT) from their list predecessors and SLAB_THIRD
                 2.0 A from one of them: rmin = 2.0, the threshold of the rank pass 3.0 is clear of every lattice distance, and only the
                 planted atoms and their neighbours have a rank.  SLAB_SHIFTED is listed a whole cell vector away: the pair has the image
                 distance 2.0 and, by the unwrapped distance, no rank.
      scrambled  jitter +-0.25 A: rmin about 2.9, nearly every atom has a rank, the ranked order scatters the list over the cell."""
    basis, layers = slab_basis(n_atoms, triclinic)
    jit = SLAB_JITTER[variant]
    rng, pick = random.Random(41), random.Random(43)
    planted = [k for k in SLAB_PLANTED if k < n_atoms] if variant == "planted" else []
    third = SLAB_THIRD if (planted and SLAB_THIRD[0] < n_atoms) else None
    keep_alpha = set(planted) | {k - 1 for k in planted} | ({third[0]} if third else set())
    per = SLAB_SIDE * SLAB_SIDE
    rows: List[AtomRow] = []
    mol = 0
    for k in range(n_atoms):
        iz, rem = divmod(k, per)
        iy, ix = divmod(rem, SLAB_SIDE)
        f = [(ix + 0.5 + rng.uniform(-jit, jit)) / SLAB_SIDE - 0.5, (iy + 0.5 + rng.uniform(-jit, jit)) / SLAB_SIDE - 0.5,
             (iz + 0.5 + rng.uniform(-jit, jit)) / layers - 0.5]
        x, y, z = (sum(f[q] * basis[q][p] for q in range(3)) for p in range(3))
        start = k - k % 37
        in_triple = k - start < 3 and start + 2 < n_atoms
        if not (in_triple and k > start):
            mol += 1
        frozen = in_triple and (start // 37) % 6 == 1
        dark = pick.random() < 0.1 and k not in keep_alpha
        q = (30.0 if k % 2 == 0 else -30.0) / 408.7816
        rows.append(AtomRow(k + 1, "Ar", "Tri" if in_triple else "Ar", "F" if frozen else "M", mol, x, y, z, 39.948, q, 0.0 if dark else 1.6411, 119.8, 3.405))
    for k in planted:
        rows[k].x, rows[k].y, rows[k].z = (getattr(rows[k - 1], c) + d for c, d in zip("xyz", SLAB_PLANT_AT))
    if third:
        rows[third[0]].x, rows[third[0]].y, rows[third[0]].z = (getattr(rows[third[1]], c) + d for c, d in zip("xyz", third[2]))
    if SLAB_SHIFTED in planted:
        r = rows[SLAB_SHIFTED]
        r.x, r.y, r.z = r.x + basis[0][0], r.y + basis[0][1], r.z + basis[0][2]
    return rows


SLAB_NAME = r"slab(\d+)_(planted|scrambled)(_tri)?"


def _slab_fixture(name: str):
    """slab<N>_<variant>[_tri]: N atoms, Gauss-Seidel sweeps in atom order (the GS_RANKED_FIXTURES swap in the ranked order)"""
    n, variant, tri = re.fullmatch(SLAB_NAME, name).groups()
    o = dict(POLAR_OPTS, polar_gs="on", polar_max_iter=3)
    return slab_box(int(n), variant, bool(tri)), slab_basis(int(n), bool(tri))[0], o


def _rot(rng: random.Random):
    """random rotation matrix from a uniformly drawn unit quaternion."""
    while True:
        q = [rng.gauss(0, 1) for _ in range(4)]
        nrm = math.sqrt(sum(c * c for c in q))
        if nrm > 1e-6:
            break
    w, x, y, z = (c / nrm for c in q)
    return [
        [1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
        [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
        [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)],
    ]


def molecular_box(n_mol: int, L: float, seed: int, extra_neutral: bool = True) -> List[AtomRow]:
    """n_mol rigid bent 3-site molecules on a jittered lattice + (optionally) one neutral polarizable atom.

    Site parameters: O  q=-0.8 e, alpha 1.45, eps 78, sigma 3.15 ; H q=+0.4 e, eps=sigma=0,
    the first H carries alpha 0.30, the second none.  O-H 0.9572 A, HOH 104.52 deg.
    """
    n = int(math.ceil((n_mol + (1 if extra_neutral else 0)) ** (1.0 / 3.0) - 1e-9))
    a = L / n
    rng = random.Random(seed)
    rows: List[AtomRow] = []
    half = math.radians(104.52) / 2
    local = [
        (0.0, 0.0, 0.0),
        (0.9572 * math.sin(half), 0.9572 * math.cos(half), 0.0),
        (-0.9572 * math.sin(half), 0.9572 * math.cos(half), 0.0),
    ]
    sites = [("O", -0.8, 1.45, 78.0, 3.15, 15.9994), ("H", 0.4, 0.30, 0.0, 0.0, 1.00794), ("H", 0.4, 0.0, 0.0, 0.0, 1.00794)]
    aid = 0
    mid = 0
    cells = [(ix, iy, iz) for ix in range(n) for iy in range(n) for iz in range(n)]
    for (ix, iy, iz) in cells[:n_mol]:
        mid += 1
        cx = (ix + 0.5) * a - L / 2 + rng.uniform(-0.1 * a, 0.1 * a)
        cy = (iy + 0.5) * a - L / 2 + rng.uniform(-0.1 * a, 0.1 * a)
        cz = (iz + 0.5) * a - L / 2 + rng.uniform(-0.1 * a, 0.1 * a)
        R = _rot(rng)
        for (name, q, al, ep, sg, mass), (lx, ly, lz) in zip(sites, local):
            aid += 1
            x = cx + R[0][0] * lx + R[0][1] * ly + R[0][2] * lz
            y = cy + R[1][0] * lx + R[1][1] * ly + R[1][2] * lz
            z = cz + R[2][0] * lx + R[2][1] * ly + R[2][2] * lz
            rows.append(AtomRow(aid, name, "H2O", "M", mid, x, y, z, mass, q, al, ep, sg))
    if extra_neutral:
        ix, iy, iz = cells[n_mol]
        mid += 1
        aid += 1
        rows.append(
            AtomRow(aid, "Xe", "Xe", "M", mid, (ix + 0.5) * a - L / 2, (iy + 0.5) * a - L / 2, (iz + 0.5) * a - L / 2,
                    131.293, 0.0, 4.044, 221.0, 4.1)
        )
    return rows


def write_pqr(path: str, rows: Sequence[AtomRow]) -> None:
    with open(path, "w") as f:
        for r in rows:
            f.write(r.line() + "\n")
        f.write("END\n")


DEFAULT_OPTS: Dict[str, object] = {
    "job_name": "t",
    "ensemble": "nvt",
    "temperature": 100.0,
    "numsteps": 1,
    "corrtime": 1,
    "seed": 1,
    "move_factor": 0.01,
    "rot_factor": 0.01,
}

QUIET = {
    "pop_histogram": "off",
    "traj_output": "off",
    "pqr_restart": "off",
    "pqr_output": "off",
    "energy_output": "off",
    "dipole_output": "off",
    "field_output": "off",
}


def write_input(path: str, pqr_name: str, basis: Sequence[Sequence[float]], opts: Dict[str, object]) -> None:
    """opts: hot-path keywords (rd_only, polarization, polar_*, ewald_*) with reference spelling."""
    lines: List[str] = []
    merged: Dict[str, object] = dict(DEFAULT_OPTS)
    merged.update(opts)
    for k, v in merged.items():
        lines.append(f"{k} {_fmt(v)}")
    for i, b in enumerate(basis):
        lines.append(f"basis{i + 1} {b[0]!r} {b[1]!r} {b[2]!r}")
    lines.append(f"pqr_input {pqr_name}")
    for k, v in QUIET.items():
        lines.append(f"{k} {v}")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def _fmt(v: object) -> str:
    if isinstance(v, bool):
        return "on" if v else "off"
    if isinstance(v, float):
        return repr(v)
    return str(v)


def cubic(L: float):
    return [[L, 0.0, 0.0], [0.0, L, 0.0], [0.0, 0.0, L]]


POLAR_OPTS = {
    "polarization": "on",
    "polar_damp_type": "exponential",
    "polar_damp": 2.1304,
    "polar_iterative": "on",
    "polar_max_iter": 10,
    "polar_ewald": "on",
    "ewald_kmax": 7,
}

# named fixtures: (rows builder, basis, options).  Sizes/seeds follow SURVEY.md Appendix A / §8d.
def fixture(name: str):
    if name == "ar2":  # Ar2 at exactly 4 A in a 10^4 A box (pi001 geometry), LJ only
        rows = [
            AtomRow(1, "Ar", "Ar", "M", 1, 0.0, 0.0, -2.0, 39.948, 0.0, 0.0, 119.8, 3.405),
            AtomRow(2, "Ar", "Ar", "M", 2, 0.0, 0.0, 2.0, 39.948, 0.0, 0.0, 119.8, 3.405),
        ]
        return rows, cubic(10000.0), {"rd_only": "on"}
    if name == "lj64":
        return lattice_box(64, 16.0, 3, charged=False, alpha=0.0), cubic(16.0), {"rd_only": "on"}
    if name == "ion64_es":  # LJ + Ewald, no polarization
        return lattice_box(64, 16.0, 3), cubic(16.0), {"ewald_kmax": 7}
    if name == "ion216_polar":  # SURVEY §4 anchor: rd -107838.41890820718 ...
        return lattice_box(216, 24.0, 7), cubic(24.0), dict(POLAR_OPTS)
    if name == "ion216_polar_nopbc":  # static field without Ewald (thole_field_nopbc)
        o = dict(POLAR_OPTS)
        o["polar_ewald"] = "off"
        return lattice_box(216, 24.0, 7), cubic(24.0), o
    if name == "ion216_triclinic":
        basis = [[24.0, 0.0, 0.0], [3.0, 23.0, 0.0], [-2.0, 4.0, 22.0]]
        return lattice_box(216, 24.0, 7), basis, dict(POLAR_OPTS)
    if name == "ion1000_triclinic":  # 16 tiles in a skewed cell: tile classes, uniform images and panels for a non-orthorhombic basis
        basis = [[40.0, 0.0, 0.0], [5.0, 38.0, 0.0], [-4.0, 6.0, 37.0]]
        return lattice_box_cell(1000, basis, 21), basis, dict(POLAR_OPTS)
    if name == "ion8000_triclinic":  # 125 tiles: far-field, beyond-cutoff and common-image tile pairs in a skewed cell (large fixture: regenerated, not stored)
        basis = [[79.8, 0.0, 0.0], [9.0, 77.0, 0.0], [-6.0, 11.0, 75.0]]
        return lattice_box_cell(8000, basis, 22), basis, dict(POLAR_OPTS)
    if name == "ion216_frozen":  # every 5th atom frozen (quirk 4: frozen handling differs per term)
        return lattice_box(216, 24.0, 7, frozen_every=5), cubic(24.0), dict(POLAR_OPTS)
    if name == "ion216_framework":  # the usual MPMC layout: ONE frozen molecule (150 sites spanning three 64-atom tiles) + 66 mobile atoms
        rows = lattice_box(216, 24.0, 7)
        for r in rows[:150]:
            r.flag, r.mol_id, r.moltype = "F", 1, "MOF"
        for k, r in enumerate(rows[150:]):
            r.mol_id = 2 + k
        return rows, cubic(24.0), dict(POLAR_OPTS)
    if name == "ion216_precision":  # precision-terminated solve
        o = dict(POLAR_OPTS)
        del o["polar_max_iter"]
        o["polar_precision"] = 1e-7
        return lattice_box(216, 24.0, 7), cubic(24.0), o
    if name == "ion216_gamma":  # polar_gamma pre-scaling, 3 iterations
        o = dict(POLAR_OPTS)
        o["polar_max_iter"] = 3
        o["polar_gamma"] = 1.03
        return lattice_box(216, 24.0, 7), cubic(24.0), o
    if name == "ion216_alpha":  # user-set ewald_alpha / polar_ewald_alpha (differ from 3.5/rc)
        o = dict(POLAR_OPTS)
        o["ewald_alpha"] = 0.31
        o["polar_ewald_alpha"] = 0.27
        o["ewald_kmax"] = 5
        return lattice_box(216, 24.0, 7), cubic(24.0), o
    if name == "water64_polar":  # SURVEY §4 molecular fixture: exclusions, intramolecular erf, quirk 2
        return molecular_box(64, 14.0, 5), cubic(14.0), dict(POLAR_OPTS)
    if name == "ion216_wolf":  # Wolf electrostatics instead of Ewald (coulombic_wolf)
        return lattice_box(216, 24.0, 7), cubic(24.0), {"wolf": "on"}
    if name == "water64_fh2":  # Feynman-Hibbs second-order corrections to LJ and real-space Coulomb
        return molecular_box(64, 14.0, 5), cubic(14.0), {"feynman_hibbs": "on", "feynman_hibbs_order": 2, "temperature": 77.0}
    if name == "water64_fh4":
        return molecular_box(64, 14.0, 5), cubic(14.0), {"feynman_hibbs": "on", "feynman_hibbs_order": 4, "temperature": 40.0}
    if name == "ion216_fh4_polar":
        o = dict(POLAR_OPTS)
        o.update({"feynman_hibbs": "on", "feynman_hibbs_order": 4, "temperature": 30.0})
        return lattice_box(216, 24.0, 7), cubic(24.0), o
    if name == "ion216_gs":  # Gauss-Seidel sweeps (polar_gs): in-place dipole updates in atom order
        o = dict(POLAR_OPTS)
        o["polar_gs"] = "on"
        o["polar_max_iter"] = 6
        return lattice_box(216, 24.0, 7), cubic(24.0), o
    if name == "water64_gs_precision":  # Gauss-Seidel, precision-terminated, molecular box (non-polarizable sites, exclusions)
        o = dict(POLAR_OPTS)
        del o["polar_max_iter"]
        o["polar_gs"] = "on"
        o["polar_precision"] = 1e-8
        o["polar_rrms"] = "on"
        return molecular_box(64, 14.0, 5), cubic(14.0), o
    if name == "ion1000_gs":  # 16 tiles: the blocked sweep crosses many tile boundaries
        o = dict(POLAR_OPTS)
        o["polar_gs"] = "on"
        o["polar_max_iter"] = 4
        return lattice_box(1000, 40.0, 11), cubic(40.0), o
    if name == "lj1000":  # BASELINE config 2
        return lattice_box(1000, 40.0, 11, charged=False, alpha=0.0), cubic(40.0), {"rd_only": "on"}
    if name == "ion1000_polar":
        return lattice_box(1000, 40.0, 11), cubic(40.0), dict(POLAR_OPTS)
    if name == "ion10k_es":  # BASELINE config 3
        return lattice_box(10000, 86.0, 13), cubic(86.0), {"ewald_kmax": 7}
    if name == "ion10k_polar":  # BASELINE config 4
        return lattice_box(10000, 86.0, 13), cubic(86.0), dict(POLAR_OPTS)
    if name.startswith("ion10k_polar_bead"):  # BASELINE config 5: image `b` of the 32-bead ensemble of the config-4 box
        rows = lattice_box(10000, 86.0, 13)
        pos = bead_positions([(r.x, r.y, r.z) for r in rows], int(name[len("ion10k_polar_bead"):]))
        for r, (x, y, z) in zip(rows, pos):
            r.x, r.y, r.z = float(x), float(y), float(z)
        return rows, cubic(86.0), dict(POLAR_OPTS)
    if name in DIRECT_FIXTURES:  # the same boxes with the dipoles by matrix inversion (the reference's default, `polar_iterative off`)
        rows, basis, o = fixture(name[:-len("_direct")])
        return rows, basis, dict(o, polar_iterative="off")
    if name in WOLF_FIXTURES:
        return _wolf_fixture(name)
    if name in THREE_BODY_FIXTURES:
        return _three_body_fixture(name)
    if name in DISP_FIXTURES:
        return _disp_fixture(name)
    if name in RD_CRYSTAL_FIXTURES:
        return _rd_crystal_fixture(name)
    if name in EWALD_FULL_FIXTURES:
        return _ewald_full_fixture(name)
    if name in RD_MODEL_FIXTURES:
        return _rd_model_fixture(name)
    if name in SG_FIXTURES:
        return _sg_fixture(name)
    if name in RELAX_FIXTURES:
        return _relax_fixture(name)
    if name in GS_RANKED_FIXTURES:
        return _gs_ranked_fixture(name)
    if re.fullmatch(SLAB_NAME, name):
        return _slab_fixture(name)
    raise KeyError(name)


# ---- dispersion-expansion repulsion/dispersion (`disp_expansion on`, reference src/System.Energy.cpp:1939-2080) -----------------------------
# per species: alpha (1/A) and r0 (A) in the PQR's epsilon / sigma columns, c6 / c8 / c10 in atomic units.  Repulsion and dispersion partly
# cancel at contact (two A atoms at 3.8 A: +124 K of repulsion against -262 K of undamped dispersion).  Lattice rows alternate A / B (the
# mixing rules see two species); in the molecular box the first H has alpha = 0 but c6 != 0 and the second H is a null site.
DISP_SPECIES = {
    "A": (3.10, 3.45, 64.3, 1623.0, 49060.0),
    "B": (2.85, 3.70, 129.6, 4187.0, 155500.0),
    "O": (3.60, 3.20, 15.0, 250.0, 5000.0),
    "H1": (0.0, 0.0, 2.5, 0.0, 0.0),
    "H2": (0.0, 0.0, 0.0, 0.0, 0.0),
    "Xe": (2.60, 4.30, 285.9, 11000.0, 500000.0),
}
DISP_OPTS = {"disp_expansion": "on"}


def _with_disp(rows: List[AtomRow], zero_c6_every: int = 0, zero_c8_every: int = 0) -> List[AtomRow]:
    """every row gets its species' parameters and all four coefficient columns (c9 = 0)"""
    prev = None
    for r in rows:
        if r.atomtype == "H":
            sp = "H1" if prev == "O" else "H2"
        elif r.atomtype in ("O", "Xe"):
            sp = r.atomtype
        else:
            sp = "A" if r.atom_id % 2 == 1 else "B"
        prev = r.atomtype
        r.eps, r.sigma, r.c6, r.c8, r.c10 = DISP_SPECIES[sp]
        r.c9 = 0.0
        if zero_c6_every and r.atom_id % zero_c6_every == 0:
            r.c6 = 0.0
        if zero_c8_every and r.atom_id % zero_c8_every == 0:
            r.c8 = 0.0
    return rows


def _disp_fixture(name: str):
    d = dict(DISP_OPTS)
    damped = dict(d, damp_dispersion="on")
    if name.startswith("ar2_disp_"):  # two atoms (species A and B) at 3.2, 3.8 or 6.0 A in a 10^4 A box
        r = {"ar2_disp_32": 3.2, "ar2_disp_38": 3.8, "ar2_disp_60": 6.0}[name]
        rows = [AtomRow(1, "Ar", "Ar", "M", 1, 0.0, 0.0, -r / 2, 39.948, 0.0, 0.0, 0.0, 0.0),
                AtomRow(2, "Ar", "Ar", "M", 2, 0.0, 0.0, r / 2, 39.948, 0.0, 0.0, 0.0, 0.0)]
        return _with_disp(rows), cubic(10000.0), dict(d if name == "ar2_disp_32" else damped, rd_only="on")
    if name == "ar216_disp":  # noble-gas lattice, rd_only, damped
        return _with_disp(lattice_box(216, 24.0, 7, charged=False, alpha=0.0)), cubic(24.0), dict(damped, rd_only="on")
    if name == "ion216_disp":  # Ewald, undamped
        return _with_disp(lattice_box(216, 24.0, 7)), cubic(24.0), dict(d, ewald_kmax=7)
    if name == "ion216_polar_disp":
        return _with_disp(lattice_box(216, 24.0, 7)), cubic(24.0), dict(POLAR_OPTS, **damped)
    if name == "water64_disp":  # 3-site molecules, an alpha = 0 site with c6, a null site, a neutral Xe; undamped
        return _with_disp(molecular_box(64, 14.0, 5)), cubic(14.0), dict(d, ewald_kmax=7)
    if name == "ion216_framework_disp":  # one frozen 150-site molecule + 66 mobile atoms
        rows, basis, o = fixture("ion216_framework")
        return _with_disp(rows), basis, dict(o, **damped)
    if name == "ion216_triclinic_disp":
        rows, basis, o = fixture("ion216_triclinic")
        return _with_disp(rows), basis, dict(o, **damped)
    if name == "ion216_extrap_disp":  # extrapolated c10, with atoms whose c6 or c8 is 0
        return (_with_disp(lattice_box(216, 24.0, 7), zero_c6_every=7, zero_c8_every=11), cubic(24.0),
                dict(damped, extrapolate_disp_coeffs="on", ewald_kmax=7))
    if name == "ion216_schmidt_disp":
        return _with_disp(lattice_box(216, 24.0, 7)), cubic(24.0), dict(d, schmidt_ff="on", ewald_kmax=7)
    if name == "ion216_nolrc_disp":
        return _with_disp(lattice_box(216, 24.0, 7)), cubic(24.0), dict(damped, rd_lrc="off", ewald_kmax=7)
    if name == "ion4000_polar_disp":  # 63 tiles: beyond the single-launch size, Ewald + polarization
        return _with_disp(lattice_box(4000, 64.0, 17)), cubic(64.0), dict(POLAR_OPTS, **damped)
    raise KeyError(name)


# ---- Axilrod-Teller three-body dispersion (`axilrod_teller on`, reference src/System.Energy.cpp:1653-1770) ----------------------------------
# per-site c9 in hartree bohr^9 (the PQR's last column); c6 for the Midzuno-Kihara form (c9 = 3/4 alpha 6.7483345 c6)
AT_C9 = {"Ar": 518.3, "O": 1200.0, "H": 25.0, "Xe": 6000.0}
AT_C6 = {"Ar": 64.3}
AT_OPTS = {"axilrod_teller": "on"}


def _with_c9(rows: List[AtomRow], c9: Optional[Dict[str, float]] = None, c6: Optional[Dict[str, float]] = None) -> List[AtomRow]:
    for r in rows:
        r.c6, r.c8, r.c10 = (c6 or {}).get(r.atomtype, 0.0), 0.0, 0.0
        r.c9 = (c9 or {}).get(r.atomtype, 0.0)
    return rows


def _three_body_fixture(name: str):
    at = dict(AT_OPTS)
    if name == "ar3_at":  # equilateral triangle (3,0,0) (0,3,0) (0,0,3), side sqrt(18) A, in a 10^4 A box: cos A cos B cos C = 1/8, LJ only
        rows = [AtomRow(k + 1, "Ar", "Ar", "M", k + 1, *xyz, 39.948, 0.0, 1.6411, 119.8, 3.405)
                for k, xyz in enumerate([(3.0, 0.0, 0.0), (0.0, 3.0, 0.0), (0.0, 0.0, 3.0)])]
        return _with_c9(rows, AT_C9), cubic(10000.0), dict(at, rd_only="on")
    if name == "ion216_at":  # single-site atoms, LJ + Ewald
        return _with_c9(lattice_box(216, 24.0, 7), AT_C9), cubic(24.0), dict(at, ewald_kmax=7)
    if name == "ion216_polar_at":
        return _with_c9(lattice_box(216, 24.0, 7), AT_C9), cubic(24.0), dict(POLAR_OPTS, **at)
    if name == "water64_at":  # 3-site molecules (same-molecule triples excluded), an alpha = 0 site, a neutral Xe
        return _with_c9(molecular_box(64, 14.0, 5), AT_C9), cubic(14.0), dict(at, ewald_kmax=7)
    if name == "ion216_framework_at":  # one frozen 150-site molecule + 66 mobile atoms
        rows, basis, o = fixture("ion216_framework")
        return _with_c9(rows, AT_C9), basis, dict(o, **at)
    if name == "ion216_triclinic_at":
        rows, basis, o = fixture("ion216_triclinic")
        return _with_c9(rows, AT_C9), basis, dict(o, **at)
    if name == "ion216_mk_at":  # Midzuno-Kihara c9 from the c6 column; the c9 column is 0 and must be ignored
        return (_with_c9(lattice_box(216, 24.0, 7), None, AT_C6), cubic(24.0),
                dict(at, ewald_kmax=7, midzuno_kihara_approx="on"))
    if name == "grid_at":  # integer grid, spacing 2 in an 8 A box: every separation of 4 A is an exact half-box image tie
        rows = []
        for ix in range(4):
            for iy in range(4):
                for iz in range(4):
                    k = len(rows) + 1
                    rows.append(AtomRow(k, "Ar", "Ar", "M", k, 2.0 * ix - 4.0, 2.0 * iy - 4.0, 2.0 * iz - 4.0, 39.948, 0.0, 1.0, 50.0, 1.2))
        return _with_c9(rows, {"Ar": 100.0}), cubic(8.0), dict(at, rd_only="on")
    if name == "ion512_at":
        return _with_c9(lattice_box(512, 32.0, 9), AT_C9), cubic(32.0), dict(at, ewald_kmax=7)
    raise KeyError(name)


def bead_positions(base_pos, bead: int, sigma: float = 0.05):
    """Image `bead` of a path-integral ensemble: base positions + Gaussian displacement (sigma in A), numpy default_rng([17, bead])
    (SURVEY §8d config 5), QUANTISED to the 6 decimals of a PQR coordinate column: what bench.py evaluates on the GPU is then, double
    for double, what the reference reads from `ion10k_polar_beadB.pqr` (tests/golden/ion10k_polar_bead{0,1}.json)."""
    import numpy as np

    # the PQR text the base positions came from has 6 decimals too: go through the same text -> double conversion
    base = np.array(np.char.mod("%.6f", np.asarray(base_pos, dtype=np.float64)), dtype=np.float64)
    rng = np.random.default_rng([17, bead])
    moved = base + rng.normal(scale=sigma, size=base.shape)
    return np.array(np.char.mod("%.6f", moved), dtype=np.float64)


SMALL_FIXTURES = [
    "ar2", "lj64", "ion64_es", "ion216_polar", "ion216_polar_nopbc", "ion216_triclinic", "ion216_frozen",
    "ion216_precision", "ion216_gamma", "ion216_alpha", "water64_polar", "lj1000", "ion1000_polar",
    "ion216_wolf", "water64_fh2", "water64_fh4", "ion216_fh4_polar", "ion216_gs", "water64_gs_precision", "ion1000_gs", "ion216_framework",
    "ion1000_triclinic",
]
# boxes with the Axilrod-Teller term: the C oracle (oracle/) has no three-body term, so they are kept apart from SMALL_FIXTURES
THREE_BODY_FIXTURES = ["ar3_at", "ion216_at", "ion216_polar_at", "water64_at", "ion216_framework_at", "ion216_triclinic_at", "ion216_mk_at",
                       "grid_at", "ion512_at"]
LARGE_FIXTURES = ["ion10k_es", "ion10k_polar", "ion10k_polar_bead0", "ion10k_polar_bead1", "ion8000_triclinic"]
# boxes with the disp-expansion term (the C oracle has no such term): kept apart like THREE_BODY_FIXTURES
DISP_FIXTURES = ["ar2_disp_32", "ar2_disp_38", "ar2_disp_60", "ar216_disp", "ion216_disp", "ion216_polar_disp", "water64_disp",
                 "ion216_framework_disp", "ion216_triclinic_disp", "ion216_extrap_disp", "ion216_schmidt_disp", "ion216_nolrc_disp",
                 "ion4000_polar_disp"]


# boxes whose dipoles the reference solves by matrix inversion (thole_bmatrix): the direct solve of the library
DIRECT_FIXTURES = ["ion216_polar_direct", "ion216_polar_nopbc_direct", "water64_polar_direct", "ion216_triclinic_direct",
                   "ion216_framework_direct", "ion1000_polar_direct"]
DIRECT_SAMPLE_EVERY = 16  # ion1000_polar_direct keeps the per-atom results of every 16th atom (63 atoms)


def keep_direct_golden(golden_dir: str) -> None:
    """After `python oracle/make_golden.py <DIRECT_FIXTURES>`: the box text is dropped (the tests regenerate it with `materialize`, which
    writes the same bytes the reference read); the 1000-atom box keeps its scalars and the per-atom rows of every DIRECT_SAMPLE_EVERY-th
    atom (`sample_atoms` lists them), the small boxes keep everything."""
    import json

    for name in DIRECT_FIXTURES:
        path = os.path.join(golden_dir, f"{name}.json")
        with open(path) as f:
            res = json.load(f)
        n = res["natoms"]
        if n > 500 and "sample_atoms" not in res:
            idx = list(range(0, n, DIRECT_SAMPLE_EVERY))
            for k, v in list(res.items()):
                if k in ("ef_static", "mu", "ef_induced"):  # flat [n][3]
                    res[k] = [v[3 * i + p] for i in idx for p in range(3)]
                elif isinstance(v, list) and len(v) > 64:
                    del res[k]
            res["sample_atoms"] = idx
        with open(path, "w") as f:
            json.dump(res, f, separators=(",", ":"))
            f.write("\n")
        for ext in (".in", ".pqr"):
            if os.path.exists(os.path.join(golden_dir, name + ext)):
                os.remove(os.path.join(golden_dir, name + ext))


# ---- `polar_wolf` / `polar_palmo` (reference src/System.Energy.cpp:3337-3396, 3602-3627) ------------------------------------------------------
# NAME = BASE_pw_VARIANT: the box BASE with polar_ewald off and the Wolf static field (polar_wolf_alpha 0.13), solved as VARIANT says
WOLF_VARIANTS = {
    "jac": {},                                                                            # Jacobi, 10 iterations
    "gs": {"polar_gs": "on", "polar_max_iter": 4},                                        # Gauss-Seidel, 4 sweeps
    "gsp": {"polar_gs": "on", "polar_max_iter": 4, "polar_palmo": "on"},                  # ... + Palmo-Krimm
    "gspg": {"polar_gs": "on", "polar_max_iter": 4, "polar_palmo": "on", "polar_gamma": 1.03},
    "direct": {"polar_iterative": "off"},                                                 # matrix inversion
    "gspp": {"polar_gs": "on", "polar_palmo": "on", "polar_precision": 1e-7, "polar_max_iter": None},  # sweeps until converged
    "jacp": {"polar_palmo": "on"},                                                        # Jacobi + Palmo-Krimm: the correction is zero to the bit
    "directp": {"polar_iterative": "off", "polar_palmo": "on"},                           # likewise under matrix inversion
}
WOLF_BASES = ["ion216_polar", "water64_polar", "ion216_framework", "ion216_triclinic"]
WOLF_FIXTURES = [f"{b}_pw_{v}" for b in WOLF_BASES for v in ("jac", "gs", "gsp", "gspg", "direct", "gspp")] + [
    "ion216_polar_pw_jacp", "ion216_polar_pw_directp",
    "ion216_polar_pw0_jac",    # polar_wolf_alpha 0: the undamped branch (:3379-3382)
    "ion216_polar_pw0_gsp",
    "ion216_polar_pwewald_gsp",  # polar_ewald on as well: Ewald wins (:3289-3294), Palmo-Krimm on an Ewald field
    "ion216_frozen_pw_gsp",
    "ion1000_gs_pw_gsp",       # 16 tiles: the blocked sweep, then the contraction
    "ion4000_pw1_gsp",         # polar_wolf_alpha 1 at a cutoff of 32 A: a R = 32, erfc and the Gaussian underflow for most pairs
]
WOLF_SAMPLE_EVERY = 16  # boxes of more than 216 atoms keep the per-atom results of every 16th atom


def _wolf_fixture(name: str):
    base, variant = name.rsplit("_", 1)
    o_extra = dict(WOLF_VARIANTS[variant])
    if base == "ion4000_pw1":
        rows, basis, o = lattice_box(4000, 64.0, 17), cubic(64.0), dict(POLAR_OPTS)
        kind = "pw1"
    else:
        box, kind = base.rsplit("_", 1)
        rows, basis, o = fixture(box)
        o = dict(o)
    o["polar_gs"] = "off"  # (ion1000_gs brings its own; the variant decides)
    o["polar_max_iter"] = 10
    o["polar_ewald"] = "on" if kind == "pwewald" else "off"
    o["polar_wolf"] = "on"
    o["polar_wolf_alpha"] = {"pw": 0.13, "pwewald": 0.13, "pw0": 0.0, "pw1": 1.0}[kind]
    for k, v in o_extra.items():
        if v is None:
            o.pop(k, None)
        else:
            o[k] = v
    return rows, basis, o


WOLF_GOLDEN = ("polar_wolf.json", "polar_wolf_atoms.npz")  # under tests/golden/: every fixture's scalars; the per-atom arrays, each once


def keep_wolf_golden(golden_dir: str, names: Optional[List[str]] = None) -> None:
    """After `python oracle/make_golden.py <WOLF_FIXTURES>`: the per-fixture files are folded into WOLF_GOLDEN and removed, the box text
    too (the tests regenerate it with `materialize`, which writes the same bytes the reference read).  polar_wolf.json holds every
    fixture's scalars and cell; polar_wolf_atoms.npz holds ef_static, mu and ef_induced as float64 -- of every atom for boxes of up to
    216 atoms, of every WOLF_SAMPLE_EVERY-th atom for larger ones -- with nothing lost (the harness prints %.17g) and each distinct
    array stored once: the variants of one box share its static field, and Palmo-Krimm leaves the dipoles alone.  A fixture's "arrays"
    entry names the key of each of its arrays; an ef_induced of zeros (the direct path never writes it) is left out."""
    import json

    import numpy as np

    scalars, arrays, by_bytes = {}, {}, {}
    for name in (names or WOLF_FIXTURES):
        with open(os.path.join(golden_dir, f"{name}.json")) as f:
            res = json.load(f)
        n = res["natoms"]
        every = WOLF_SAMPLE_EVERY if n > 216 else 1
        out = {k: v for k, v in res.items() if not isinstance(v, list) or k in ("basis", "reciprocal_basis")}
        out["sample_every"] = every
        out["arrays"] = {}
        for k in ("ef_static", "mu", "ef_induced"):
            a = np.asarray(res[k], dtype=np.float64).reshape(-1, 3)
            a = a[::every] if a.shape[0] == n else a  # (a file that an earlier pass has already cut down to the sample)
            if k == "ef_induced" and not a.any():
                continue
            key = by_bytes.setdefault(a.tobytes(), f"{name}.{k}")
            arrays.setdefault(key, a)
            out["arrays"][k] = key
        scalars[name] = out
    with open(os.path.join(golden_dir, WOLF_GOLDEN[0]), "w") as f:
        json.dump(scalars, f, indent=0, separators=(",", ":"))
        f.write("\n")
    np.savez_compressed(os.path.join(golden_dir, WOLF_GOLDEN[1]), **arrays)
    for name in (names or WOLF_FIXTURES):
        for ext in (".json", ".in", ".pqr"):
            if os.path.exists(os.path.join(golden_dir, name + ext)):
                os.remove(os.path.join(golden_dir, name + ext))


def wolf_golden(golden_dir: str, name: str) -> Dict[str, object]:
    """one fixture of WOLF_GOLDEN as make_golden wrote it: scalars, `sample_atoms`, and ef_static / mu / ef_induced as [k, 3] arrays"""
    import json

    import numpy as np

    with open(os.path.join(golden_dir, WOLF_GOLDEN[0])) as f:
        g = json.load(f)[name]
    with np.load(os.path.join(golden_dir, WOLF_GOLDEN[1])) as z:
        for k, key in g.pop("arrays").items():
            g[k] = z[key]
    g["sample_atoms"] = list(range(0, g["natoms"], g.pop("sample_every")))
    return g


# ---- `rd_crystal on` (reference src/System.Energy.cpp:916-963, 1017-1022, 1152-1208) ----------------------------------------------------------
# NAME = BASE_rcO: the box BASE with the lattice-summed Lennard-Jones of order O.  Bases that exist only here:
#   ar2_eq / ar2_gt / ar2_lt  two Ar atoms in a cubic 10 A cell at x = 0 and x = 5.0 / 5.000001 / 4.999999, rd_only: at x = 5.0 and order 2 one
#                             image lies exactly at the cutoff 15 A (kept: the reference drops r > cutoff only)
#   water64_shift             water64_polar with every molecule moved by a whole lattice vector (the term reads the raw positions)
#   ion216_nolrc              ion216_polar with rd_lrc off
#   ion4000_polar             63 tiles, Ewald + polarization (golden only: the tests of the large sizes regenerate it)
RD_CRYSTAL_FIXTURES = [f"ar2_{t}_rc{o}" for t in ("eq", "gt", "lt") for o in (1, 2, 3)] + [
    "lj64_rc2", "water64_polar_rc1", "water64_polar_rc2", "water64_polar_rc3", "water64_shift_rc1", "water64_shift_rc2",
    "ion216_triclinic_rc2", "ion216_framework_rc2", "water64_fh2_rc2", "water64_fh4_rc2", "ion216_nolrc_rc2", "ion216_polar_rc1",
    "ion1000_polar_rc2", "ion4000_polar_rc2"]
RD_CRYSTAL_AR2_X = {"eq": 5.0, "gt": 5.000001, "lt": 4.999999}
RD_CRYSTAL_GOLDEN = "rd_crystal.json"  # under tests/golden/: every fixture's scalars


def _rd_crystal_fixture(name: str):
    base, order = name.rsplit("_rc", 1)
    if base.startswith("ar2_"):
        x = RD_CRYSTAL_AR2_X[base[4:]]
        rows = [AtomRow(1, "Ar", "Ar", "M", 1, 0.0, 0.0, 0.0, 39.948, 0.0, 0.0, 119.8, 3.405),
                AtomRow(2, "Ar", "Ar", "M", 2, x, 0.0, 0.0, 39.948, 0.0, 0.0, 119.8, 3.405)]
        basis, o = cubic(10.0), {"rd_only": "on"}
    elif base == "water64_shift":
        rows, basis, o = fixture("water64_polar")
        L = basis[0][0]
        for r in rows:  # molecule m by (m % 3 - 1, m // 3 % 3 - 1, m // 9 % 3 - 1) cells
            m = r.mol_id
            r.x += (m % 3 - 1) * L
            r.y += (m // 3 % 3 - 1) * L
            r.z += (m // 9 % 3 - 1) * L
    elif base == "ion216_nolrc":
        rows, basis, o = fixture("ion216_polar")
        o = dict(o, rd_lrc="off")
    elif base == "ion4000_polar":
        rows, basis, o = lattice_box(4000, 64.0, 17), cubic(64.0), dict(POLAR_OPTS)
    else:
        rows, basis, o = fixture(base)
    return rows, basis, dict(o, rd_crystal="on", rd_crystal_order=int(order))


def keep_rd_crystal_golden(golden_dir: str, names: Optional[List[str]] = None) -> None:
    """After `python oracle/make_golden.py <RD_CRYSTAL_FIXTURES>`: the per-fixture files are folded into RD_CRYSTAL_GOLDEN (scalars and
    cell only) and removed, the box text too (the tests regenerate it with `materialize`, which writes the same bytes the reference read)."""
    import json

    out = {}
    for name in (names or RD_CRYSTAL_FIXTURES):
        with open(os.path.join(golden_dir, f"{name}.json")) as f:
            res = json.load(f)
        out[name] = {k: v for k, v in res.items() if not isinstance(v, list) or k in ("basis", "reciprocal_basis")}
    with open(os.path.join(golden_dir, RD_CRYSTAL_GOLDEN), "w") as f:
        json.dump(out, f, indent=0, separators=(",", ":"))
        f.write("\n")
    for name in (names or RD_CRYSTAL_FIXTURES):
        for ext in (".json", ".in", ".pqr"):
            if os.path.exists(os.path.join(golden_dir, name + ext)):
                os.remove(os.path.join(golden_dir, name + ext))


def rd_crystal_golden(golden_dir: str, name: str) -> Dict[str, object]:
    import json

    with open(os.path.join(golden_dir, RD_CRYSTAL_GOLDEN)) as f:
        return json.load(f)[name]


# ---- the rd model: `waldmanhagler` / `halgren_mixing` / `c6_mixing`, `lj_buffered_14_7` / `dreiding` (reference src/System.cpp:1069-1177,
# src/System.Energy.cpp:897-1032, 1212-1248, 2098-2215) ------------------------------------------------------------------------------------------
# NAME = BASE_rdm_<form><rule>: the box BASE with three species on its non-H rows (by atom_id % 5: 1 and 3 -> B, 4 -> C, else A; with one
# species every mixing rule gives the atom's own parameters back), form lj | b147 | drd, rule lb | wh | hal | c6.  In the water64 boxes the
# first H of every molecule also carries a dispersion coefficient: its pairs are not excluded, and their mixed sigma is 0.  Bases that exist
# only here:
#   arkr_eq / arkr_gt / arkr_lt   species A and B alone in a cubic 10 A cell at (0, 0, 0) and (3, 4 | 4.000001 | 3.999999, 0), rd_only: at
#                                 (3, 4, 0) the pair sits exactly at the cutoff 5 A and every form keeps it
#   arkr_contact                  the same two atoms 0.9 A apart: below 0.4 sigma_ij DREIDING's exponential term is MAXVALUE
#   ion216_nolrc                  ion216_polar with rd_lrc off
#   ion4000_polar                 63 tiles, cutoff 32 A: many tile pairs lie wholly beyond it
RD_MODEL_SPECIES = {"A": (119.8, 3.405), "B": (36.7, 2.958), "C": (10.22, 2.28)}  # (epsilon K, sigma A)
RD_MODEL_FORMS = {"lj": {}, "b147": {"lj_buffered_14_7": "on"}, "drd": {"dreiding": "on"}}
RD_MODEL_RULES = {"lb": {}, "wh": {"waldmanhagler": "on"}, "hal": {"halgren_mixing": "on"}, "c6": {"c6_mixing": "on"}}
RD_MODEL_COMBOS = [f + r for f in RD_MODEL_FORMS for r in RD_MODEL_RULES if (f, r) != ("lj", "lb")]
RD_MODEL_ARKR_Y = {"eq": 4.0, "gt": 4.000001, "lt": 3.999999}
RD_MODEL_FIXTURES = [f"ion216_polar_rdm_{m}" for m in RD_MODEL_COMBOS] + [
    "water64_polar_rdm_b147hal", "water64_polar_rdm_drdwh", "water64_polar_rdm_ljwh", "ion216_framework_rdm_b147hal", "ion216_framework_rdm_ljc6",
    "ion216_triclinic_rdm_ljwh", "ion216_triclinic_rdm_drdlb", "ion216_fh4_polar_rdm_ljwh", "ion216_nolrc_rdm_ljhal",
    "ion4000_polar_rdm_b147hal", "ion4000_polar_rdm_ljwh"] + [
    f"arkr_{t}_rdm_{m}" for t in ("eq", "gt", "lt") for m in ("ljwh", "b147lb", "drdlb")] + ["arkr_contact_rdm_drdlb"]
RD_MODEL_GOLDEN = "rd_model.json"  # under tests/golden/: every fixture's scalars


def rd_model_species(rows: List[AtomRow]) -> List[AtomRow]:
    """the three species on every non-H row, by atom_id % 5"""
    for r in rows:
        if r.atomtype == "H":
            continue
        sp = {1: "B", 3: "B", 4: "C"}.get(r.atom_id % 5, "A")
        r.eps, r.sigma = RD_MODEL_SPECIES[sp]
    return rows


def rd_model_combo(tag: str):
    """'b147hal' -> ('b147', 'hal')"""
    for f in sorted(RD_MODEL_FORMS, key=len, reverse=True):
        if tag.startswith(f) and tag[len(f):] in RD_MODEL_RULES:
            return f, tag[len(f):]
    raise KeyError(tag)


def _rd_model_fixture(name: str):
    base, tag = name.rsplit("_rdm_", 1)
    form, rule = rd_model_combo(tag)
    if base.startswith("arkr_"):
        (ea, sa), (eb, sb) = RD_MODEL_SPECIES["A"], RD_MODEL_SPECIES["B"]
        at = (0.9, 0.0) if base == "arkr_contact" else (3.0, RD_MODEL_ARKR_Y[base[5:]])
        rows = [AtomRow(1, "Ar", "Ar", "M", 1, 0.0, 0.0, 0.0, 39.948, 0.0, 0.0, ea, sa),
                AtomRow(2, "Kr", "Kr", "M", 2, at[0], at[1], 0.0, 83.798, 0.0, 0.0, eb, sb)]
        basis, o = cubic(10.0), {"rd_only": "on"}
    elif base == "ion216_nolrc":
        rows, basis, o = fixture("ion216_polar")
        o = dict(o, rd_lrc="off")
    elif base == "ion4000_polar":
        rows, basis, o = lattice_box(4000, 64.0, 17), cubic(64.0), dict(POLAR_OPTS)
    else:
        rows, basis, o = fixture(base)
    if not base.startswith("arkr_"):
        rows = rd_model_species(rows)
    if base.startswith("water64"):
        for r in rows:  # (every row prints its coefficient columns: the reference's reader carries a row's values on to rows without them)
            r.c6 = 1.0 if (r.atomtype == "H" and r.alpha != 0.0) else 0.0
    return rows, basis, dict(o, **RD_MODEL_FORMS[form], **RD_MODEL_RULES[rule])


def keep_rd_model_golden(golden_dir: str, names: Optional[List[str]] = None) -> None:
    """After `python oracle/make_golden.py <RD_MODEL_FIXTURES>`: the per-fixture files are folded into RD_MODEL_GOLDEN (scalars and cell
    only) and removed, the box text too (the tests regenerate it with `materialize`, which writes the same bytes the reference read)."""
    import json

    out = {}
    for name in (names or RD_MODEL_FIXTURES):
        with open(os.path.join(golden_dir, f"{name}.json")) as f:
            res = json.load(f)
        out[name] = {k: v for k, v in res.items() if not isinstance(v, list) or k in ("basis", "reciprocal_basis")}
    with open(os.path.join(golden_dir, RD_MODEL_GOLDEN), "w") as f:
        json.dump(out, f, indent=0, separators=(",", ":"))
        f.write("\n")
    for name in (names or RD_MODEL_FIXTURES):
        for ext in (".json", ".in", ".pqr"):
            if os.path.exists(os.path.join(golden_dir, name + ext)):
                os.remove(os.path.join(golden_dir, name + ext))


def rd_model_golden(golden_dir: str, name: str) -> Dict[str, object]:
    import json

    with open(os.path.join(golden_dir, RD_MODEL_GOLDEN)) as f:
        return json.load(f)[name]


# ---- `sg on`: the Silvera-Goldman H2 potential (reference src/System.Energy.cpp:1763-1867) ------------------------------------------------------
# Hydrogen at about the liquid's density (3.75 A between lattice sites, +-10 % jitter): the cutoff, half the shortest cell edge, lies beyond
# RM = 8.321 bohr = 4.40 A, so every box has pairs on both sides of the switch of the damping function.  sigma, epsilon and the charge play
# no part in sg(); the rows carry hydrogen's usual values.
#   h2_64_sg, h2_216_sg        single-site molecules in cubic cells of 15 and 22.5 A
#   h2_64_sg_ortho             64 sites in a 14 x 16 x 18 A cell;  h2_216_sg_tri: 216 sites in a skewed cell
#   h2_2site_sg                32 molecules of two sites 2.4 A apart: sg() counts the pairs inside a molecule
#   h2d2_64_sg_fh_a / _b       H2 and D2 alternating, feynman_hibbs on at 30 K: the correction takes the mass of the molecule of the pair's
#                              FIRST atom in the list; _b lists the same atoms in reverse order
#   h2_64_sg_lrc               rd_lrc on and rd_crystal on (order 2): sg() ignores both
#   h2_64_sg_polar             charges, polarizabilities and polarization on: energy() skips electrostatics and polarization under sg
SG_MASS = {"H2": 2.016, "D2": 4.028}
SG_FIXTURES = ["h2_64_sg", "h2_216_sg", "h2_64_sg_ortho", "h2_216_sg_tri", "h2_2site_sg", "h2d2_64_sg_fh_a", "h2d2_64_sg_fh_b", "h2_64_sg_lrc",
               "h2_64_sg_polar"]
SG_GOLDEN = "sg.json"  # under tests/golden/: every fixture's scalars
SG_TRI_BASIS = [[22.5, 0.0, 0.0], [3.0, 22.0, 0.0], [-2.0, 4.0, 21.5]]


def _h2_rows(rows: List[AtomRow], charged: bool = False) -> List[AtomRow]:
    for r in rows:
        r.atomtype, r.moltype, r.mass, r.eps, r.sigma = "H2G", "H2", SG_MASS["H2"], 34.2, 2.96
        if not charged:
            r.charge_e, r.alpha = 0.0, 0.0
    return rows


def _sg_fixture(name: str):
    o = {"sg": "on"}
    if name == "h2_216_sg":
        return _h2_rows(lattice_box(216, 22.5, 31)), cubic(22.5), o
    if name == "h2_64_sg_ortho":
        basis = [[14.0, 0.0, 0.0], [0.0, 16.0, 0.0], [0.0, 0.0, 18.0]]
        return _h2_rows(lattice_box_cell(64, basis, 32)), basis, o
    if name == "h2_216_sg_tri":
        return _h2_rows(lattice_box_cell(216, SG_TRI_BASIS, 33)), SG_TRI_BASIS, o
    if name == "h2_2site_sg":  # the second site 2.4 A from the first, in a seeded direction
        rng = random.Random(34)
        rows = []
        for k, r in enumerate(_h2_rows(lattice_box(32, 15.0, 35))):
            ux, uy, uz = _rot(rng)[0]
            rows.append(AtomRow(2 * k + 1, "H2G", "H2", "M", k + 1, r.x, r.y, r.z, 1.008, 0.0, 0.0, 34.2, 2.96))
            rows.append(AtomRow(2 * k + 2, "H2E", "H2", "M", k + 1, r.x + 2.4 * ux, r.y + 2.4 * uy, r.z + 2.4 * uz, 1.008, 0.0, 0.0, 0.0, 0.0))
        return rows, cubic(15.0), o
    if name.startswith("h2d2_64_sg_fh_"):
        rows = _h2_rows(lattice_box(64, 15.0, 36))
        for r in rows[1::2]:
            r.atomtype, r.moltype, r.mass = "D2G", "D2", SG_MASS["D2"]
        if name.endswith("_b"):
            rows = rows[::-1]
            for k, r in enumerate(rows):
                r.atom_id = r.mol_id = k + 1
        return rows, cubic(15.0), dict(o, feynman_hibbs="on", temperature=30.0)
    if name == "h2_64_sg_lrc":
        return _h2_rows(lattice_box(64, 15.0, 30)), cubic(15.0), dict(o, rd_lrc="on", rd_crystal="on", rd_crystal_order=2)
    if name == "h2_64_sg_polar":
        rows = _h2_rows(lattice_box(64, 15.0, 30, alpha=0.8), charged=True)
        return rows, cubic(15.0), dict(POLAR_OPTS, **o)
    return _h2_rows(lattice_box(64, 15.0, 30)), cubic(15.0), o  # h2_64_sg


def keep_sg_golden(golden_dir: str, names: Optional[List[str]] = None) -> None:
    """After `python oracle/make_golden.py <SG_FIXTURES>`: the per-fixture files are folded into SG_GOLDEN (scalars and cell only) and
    removed, the box text too (the tests regenerate it with `materialize`, which writes the same bytes the reference read)."""
    import json

    out = {}
    for name in (names or SG_FIXTURES):
        with open(os.path.join(golden_dir, f"{name}.json")) as f:
            res = json.load(f)
        out[name] = {k: v for k, v in res.items() if not isinstance(v, list) or k in ("basis", "reciprocal_basis")}
    with open(os.path.join(golden_dir, SG_GOLDEN), "w") as f:
        json.dump(out, f, indent=0, separators=(",", ":"))
        f.write("\n")
    for name in (names or SG_FIXTURES):
        for ext in (".json", ".in", ".pqr"):
            if os.path.exists(os.path.join(golden_dir, name + ext)):
                os.remove(os.path.join(golden_dir, name + ext))


def sg_golden(golden_dir: str, name: str) -> Dict[str, object]:
    import json

    with open(os.path.join(golden_dir, SG_GOLDEN)) as f:
        return json.load(f)[name]


# ---- `polar_ewald_full on` (reference src/System.Energy.cpp:2785-2830, 2944-3143) -------------------------------------------------------------
# NAME = BASE_pef[_VARIANT]: the box BASE with the fully periodic dipole solve.  Variants: it3 = polar_max_iter 3 (4 passes); prec =
# polar_precision 1e-8 and no polar_max_iter.  Bases that exist only here:
#   ion4000_polar       63 tiles, cutoff 32 A: many tile pairs lie wholly beyond it (golden sample only)
#   pol2_eq / pol2_gt   two charged polarizable atoms in a cubic 10 A cell at x = 0 and x = 5.0 / 5.000001: at 5.0 the pair sits exactly at
#                       the cutoff and is kept (the reference drops rimg > cutoff only); polar_ewald_alpha EWALD_FULL_POL2_ALPHA
EWALD_FULL_FIXTURES = [
    "ion216_polar_pef", "ion216_polar_pef_it3", "ion216_polar_pef_prec", "ion216_polar_nopbc_pef", "ion216_alpha_pef", "water64_polar_pef",
    "ion216_framework_pef", "ion216_frozen_pef", "ion216_triclinic_pef", "ion1000_polar_pef", "ion1000_triclinic_pef", "ion4000_polar_pef",
    "pol2_eq_pef", "pol2_gt_pef"]
EWALD_FULL_POL2_X = {"eq": 5.0, "gt": 5.000001}
EWALD_FULL_POL2_ALPHA = 0.7  # 3.5 / cutoff: the reference's iteration contracts at it (10 against 40 passes agree to 2e-5, iterator_failed 0)
EWALD_FULL_SAMPLE_EVERY = 16  # boxes of more than 216 atoms keep the per-atom results of every 16th atom
EWALD_FULL_GOLDEN = ("polar_ewald_full.json", "polar_ewald_full_atoms.npz")  # under tests/golden/: every fixture's scalars; the per-atom arrays


def _ewald_full_fixture(name: str):
    base, _, variant = name.partition("_pef")
    if base.startswith("pol2_"):
        x = EWALD_FULL_POL2_X[base[5:]]
        rows = [AtomRow(1, "Ar", "Ar", "M", 1, 0.0, 0.0, 0.0, 39.948, 0.1, 1.6411, 119.8, 3.405),
                AtomRow(2, "Ar", "Ar", "M", 2, x, 0.0, 0.0, 39.948, -0.1, 1.6411, 119.8, 3.405)]
        basis, o = cubic(10.0), dict(POLAR_OPTS, polar_ewald_alpha=EWALD_FULL_POL2_ALPHA)
    elif base == "ion4000_polar":
        rows, basis, o = lattice_box(4000, 64.0, 17), cubic(64.0), dict(POLAR_OPTS)
    else:
        rows, basis, o = fixture(base)
        o = dict(o)
    if variant == "_it3":
        o["polar_max_iter"] = 3
    elif variant == "_prec":
        o.pop("polar_max_iter", None)
        o["polar_precision"] = 1e-8
    elif variant:
        raise KeyError(name)
    return rows, basis, dict(o, polar_ewald_full="on")


def keep_ewald_full_golden(golden_dir: str, names: Optional[List[str]] = None) -> None:
    """After `python oracle/make_golden.py <EWALD_FULL_FIXTURES>`: the per-fixture files are folded into EWALD_FULL_GOLDEN and removed, the
    box text too (the tests regenerate it with `materialize`, which writes the same bytes the reference read).  The json holds every
    fixture's scalars and cell; the npz holds ef_static, mu and ef_induced as float64 -- of every atom for boxes of up to 216 atoms, of
    every EWALD_FULL_SAMPLE_EVERY-th atom for larger ones (whatever sample the harness printed is cut down to those) -- each distinct
    array stored once."""
    import json

    import numpy as np

    scalars, arrays, by_bytes = {}, {}, {}
    for name in (names or EWALD_FULL_FIXTURES):
        with open(os.path.join(golden_dir, f"{name}.json")) as f:
            res = json.load(f)
        n = res["natoms"]
        every = EWALD_FULL_SAMPLE_EVERY if n > 216 else 1
        out = {k: v for k, v in res.items() if not isinstance(v, list) or k in ("basis", "reciprocal_basis")}
        out["sample_every"] = every
        out["arrays"] = {}
        for k in ("ef_static", "mu", "ef_induced"):
            a = np.asarray(res[k], dtype=np.float64).reshape(-1, 3)
            assert a.shape[0] == n, (name, k, a.shape)
            a = a[::every]
            key = by_bytes.setdefault(a.tobytes(), f"{name}.{k}")
            arrays.setdefault(key, a)
            out["arrays"][k] = key
        scalars[name] = out
    with open(os.path.join(golden_dir, EWALD_FULL_GOLDEN[0]), "w") as f:
        json.dump(scalars, f, indent=0, separators=(",", ":"))
        f.write("\n")
    np.savez_compressed(os.path.join(golden_dir, EWALD_FULL_GOLDEN[1]), **arrays)
    for name in (names or EWALD_FULL_FIXTURES):
        for ext in (".json", ".in", ".pqr"):
            if os.path.exists(os.path.join(golden_dir, name + ext)):
                os.remove(os.path.join(golden_dir, name + ext))


def ewald_full_golden(golden_dir: str, name: str) -> Dict[str, object]:
    """one fixture of EWALD_FULL_GOLDEN: scalars, `sample_atoms`, and ef_static / mu / ef_induced as [k, 3] arrays"""
    import json

    import numpy as np

    with open(os.path.join(golden_dir, EWALD_FULL_GOLDEN[0])) as f:
        g = json.load(f)[name]
    with np.load(os.path.join(golden_dir, EWALD_FULL_GOLDEN[1])) as z:
        for k, key in g.pop("arrays").items():
            g[k] = z[key]
    g["sample_atoms"] = list(range(0, g["natoms"], g.pop("sample_every")))
    return g


# ---- `polar_sor` / `polar_esor` / `polar_zodid` (reference src/System.Energy.cpp:3450-3560, 3181-3211) ---------------------------------------
# NAME = BASE_rx_VARIANT: the box BASE with a relaxed dipole update or zeroth-order dipoles.  None = the keyword is taken out.
RELAX_VARIANTS = {
    "sor08": {"polar_sor": "on", "polar_gamma": 0.8},                                      # Jacobi, 10 iterations
    "sor12": {"polar_sor": "on", "polar_gamma": 1.2},                                      # over-relaxed
    "esor06": {"polar_esor": "on", "polar_gamma": 0.6},
    "sorp": {"polar_sor": "on", "polar_gamma": 0.8, "polar_precision": 1e-7, "polar_rrms": "on", "polar_max_iter": None},
    "esorp": {"polar_esor": "on", "polar_gamma": 0.6, "polar_precision": 1e-7, "polar_rrms": "on", "polar_max_iter": None},
    "sorfail": {"polar_sor": "on", "polar_gamma": 2.5, "polar_precision": 1e-7, "polar_max_iter": None},  # diverges: 128 iterations, iterator_failed
    "gssor": {"polar_gs": "on", "polar_sor": "on", "polar_gamma": 0.9, "polar_max_iter": 6},   # Gauss-Seidel sweeps, blended behind each
    "gsesorp": {"polar_gs": "on", "polar_esor": "on", "polar_gamma": 0.7, "polar_max_iter": 6, "polar_palmo": "on"},  # ... + Palmo-Krimm
    "gsesor4": {"polar_gs": "on", "polar_esor": "on", "polar_gamma": 0.7, "polar_max_iter": 4},
    "zodid": {"polar_zodid": "on"},
    "zodidg": {"polar_zodid": "on", "polar_gamma": 1.03},                                  # the start vector carries polar_gamma
    "zodidsor": {"polar_zodid": "on", "polar_gamma": 1.03, "polar_sor": "on"},             # ... but not under a scheme
    "zodidpalmo": {"polar_zodid": "on", "polar_palmo": "on"},                              # the correction is exactly 0
    "zodidwolf": {"polar_zodid": "on", "polar_ewald": "off", "polar_wolf": "on", "polar_wolf_alpha": 0.13},
    "pefsor": {"polar_ewald_full": "on", "polar_sor": "on", "polar_gamma": 0.8},
    "pefesor": {"polar_ewald_full": "on", "polar_esor": "on", "polar_gamma": 0.6},
    "pefsorp": {"polar_ewald_full": "on", "polar_sor": "on", "polar_gamma": 0.8, "polar_precision": 1e-7, "polar_max_iter": None},
    "pefzodid": {"polar_ewald_full": "on", "polar_zodid": "on"},                           # zodid changes nothing under ewald_full
}
RELAX_FIXTURES = [f"ion216_polar_rx_{v}" for v in RELAX_VARIANTS if v != "gsesor4"] + [
    f"{b}_rx_{v}" for b in ("ion216_polar_nopbc", "ion216_triclinic", "water64_polar") for v in ("sor08", "esor06", "gssor", "zodid")] + [
    "water64_polar_rx_sorp", "water64_polar_rx_gsesorp",  # non-polarizable sites, exclusions, strong coupling
    "ion1000_gs_rx_gsesor4"]                              # 16 tiles: the blocked sweep, blended
RELAX_SAMPLE_EVERY = 16  # boxes of more than 216 atoms keep the per-atom results of every 16th atom
RELAX_GOLDEN = ("polar_relax.json", "polar_relax_atoms.npz")  # under tests/golden/: every fixture's scalars; the per-atom arrays


def _relax_fixture(name: str):
    base, variant = name.rsplit("_rx_", 1)
    rows, basis, o = fixture(base)
    o = dict(o, polar_gs="off", polar_max_iter=10)  # (ion1000_gs brings its own; the variant decides)
    for k, v in RELAX_VARIANTS[variant].items():
        if v is None:
            o.pop(k, None)
        else:
            o[k] = v
    return rows, basis, o


def keep_relax_golden(golden_dir: str, names: Optional[List[str]] = None) -> None:
    """After `python oracle/make_golden.py <RELAX_FIXTURES>`: the per-fixture files are folded into RELAX_GOLDEN and removed, the box text
    too (the tests regenerate it with `materialize`), the way keep_ewald_full_golden keeps its family."""
    import json

    import numpy as np

    scalars, arrays, by_bytes = {}, {}, {}
    for name in (names or RELAX_FIXTURES):
        with open(os.path.join(golden_dir, f"{name}.json")) as f:
            res = json.load(f)
        n = res["natoms"]
        every = RELAX_SAMPLE_EVERY if n > 216 else 1
        out = {k: v for k, v in res.items() if not isinstance(v, list) or k in ("basis", "reciprocal_basis")}
        out["sample_every"] = every
        out["arrays"] = {}
        for k in ("ef_static", "mu", "ef_induced"):
            a = np.asarray(res[k], dtype=np.float64).reshape(-1, 3)
            assert a.shape[0] == n, (name, k, a.shape)
            a = a[::every]
            key = by_bytes.setdefault(a.tobytes(), f"{name}.{k}")
            arrays.setdefault(key, a)
            out["arrays"][k] = key
        scalars[name] = out
    with open(os.path.join(golden_dir, RELAX_GOLDEN[0]), "w") as f:
        json.dump(scalars, f, indent=0, separators=(",", ":"))
        f.write("\n")
    np.savez_compressed(os.path.join(golden_dir, RELAX_GOLDEN[1]), **arrays)
    for name in (names or RELAX_FIXTURES):
        for ext in (".json", ".in", ".pqr"):
            if os.path.exists(os.path.join(golden_dir, name + ext)):
                os.remove(os.path.join(golden_dir, name + ext))


def relax_golden(golden_dir: str, name: str) -> Dict[str, object]:
    """one fixture of RELAX_GOLDEN: scalars, `sample_atoms`, and ef_static / mu / ef_induced as [k, 3] arrays"""
    import json

    import numpy as np

    with open(os.path.join(golden_dir, RELAX_GOLDEN[0])) as f:
        g = json.load(f)[name]
    with np.load(os.path.join(golden_dir, RELAX_GOLDEN[1])) as z:
        for k, key in g.pop("arrays").items():
            g[k] = z[key]
    g["sample_atoms"] = list(range(0, g["natoms"], g.pop("sample_every")))
    return g


# ---- `polar_gs_ranked` (reference src/System.cpp:1001-1029, src/System.Energy.cpp:3450-3543, 3631-3656) -------------------------------------
# NAME = BASE_gr_VARIANT: the box BASE with Gauss-Seidel sweeps in ranked order.  None = the keyword is taken out.
GS_RANKED_VARIANTS = {
    "it1": {"polar_max_iter": 1},                                                          # no ranked sweep: exactly polar_gs
    "it2": {"polar_max_iter": 2},                                                          # one sweep in atom order, one in ranked order
    "it4": {"polar_max_iter": 4},
    "p": {"polar_precision": 1e-7, "polar_rrms": "on", "polar_max_iter": None},            # sweeps until converged
    "sor": {"polar_sor": "on", "polar_gamma": 0.9, "polar_max_iter": 6},                   # blended behind each sweep
    "esorpalmo": {"polar_esor": "on", "polar_gamma": 0.7, "polar_max_iter": 6, "polar_palmo": "on"},  # ... + Palmo-Krimm
    "it3": {"polar_max_iter": 3},                                                          # (the slab boxes only)
}
GS_RANKED_SLABS = ["slab1089_planted", "slab1089_planted_tri"]  # 18 tiles, the last with one atom: a ranked view whose tile pairs have classes
GS_RANKED_BASES = ["ion216_polar", "ion216_polar_nopbc", "water64_polar", "ion216_triclinic", "ion1000_gs"] + GS_RANKED_SLABS
GS_RANKED_FIXTURES = ([f"ion216_polar_gr_{v}" for v in GS_RANKED_VARIANTS if v != "it3"] + [f"{b}_gr_it4" for b in GS_RANKED_BASES[1:5]]
                      + [f"{b}_gr_it3" for b in GS_RANKED_SLABS])
GS_RANKED_SAMPLE_EVERY = 16  # boxes of more than 216 atoms keep the per-atom results of every 16th atom
GS_RANKED_GOLDEN = ("polar_gs_ranked.json", "polar_gs_ranked.npz")  # under tests/golden/: every fixture's scalars; the per-atom arrays


def _gs_ranked_fixture(name: str):
    base, variant = name.rsplit("_gr_", 1)
    rows, basis, o = fixture(base)
    o = dict(o, polar_gs="off", polar_gs_ranked="on", polar_max_iter=10)  # (ion1000_gs brings its own polar_gs; both together are an input error)
    for k, v in GS_RANKED_VARIANTS[variant].items():
        if v is None:
            o.pop(k, None)
        else:
            o[k] = v
    return rows, basis, o


def keep_gs_ranked_golden(golden_dir: str, names: Optional[List[str]] = None) -> None:
    """After `python oracle/make_golden.py <GS_RANKED_FIXTURES>`: the per-fixture files are folded into GS_RANKED_GOLDEN and removed, the box
    text too (the tests regenerate it with `materialize`), the way keep_relax_golden keeps its family."""
    import json

    import numpy as np

    scalars, arrays, by_bytes = {}, {}, {}
    for name in (names or GS_RANKED_FIXTURES):
        with open(os.path.join(golden_dir, f"{name}.json")) as f:
            res = json.load(f)
        n = res["natoms"]
        every = GS_RANKED_SAMPLE_EVERY if n > 216 else 1
        out = {k: v for k, v in res.items() if not isinstance(v, list) or k in ("basis", "reciprocal_basis")}
        out["sample_every"] = every
        out["arrays"] = {}
        for k in ("ef_static", "mu", "ef_induced"):
            a = np.asarray(res[k], dtype=np.float64).reshape(-1, 3)
            assert a.shape[0] == n, (name, k, a.shape)
            a = a[::every]
            key = by_bytes.setdefault(a.tobytes(), f"{name}.{k}")
            arrays.setdefault(key, a)
            out["arrays"][k] = key
        scalars[name] = out
    with open(os.path.join(golden_dir, GS_RANKED_GOLDEN[0]), "w") as f:
        json.dump(scalars, f, indent=0, separators=(",", ":"))
        f.write("\n")
    np.savez_compressed(os.path.join(golden_dir, GS_RANKED_GOLDEN[1]), **arrays)
    for name in (names or GS_RANKED_FIXTURES):
        for ext in (".json", ".in", ".pqr"):
            if os.path.exists(os.path.join(golden_dir, name + ext)):
                os.remove(os.path.join(golden_dir, name + ext))


def gs_ranked_golden(golden_dir: str, name: str) -> Dict[str, object]:
    """one fixture of GS_RANKED_GOLDEN: scalars, `sample_atoms`, and ef_static / mu / ef_induced as [k, 3] arrays"""
    import json

    import numpy as np

    with open(os.path.join(golden_dir, GS_RANKED_GOLDEN[0])) as f:
        g = json.load(f)[name]
    with np.load(os.path.join(golden_dir, GS_RANKED_GOLDEN[1])) as z:
        for k, key in g.pop("arrays").items():
            g[k] = z[key]
    g["sample_atoms"] = list(range(0, g["natoms"], g.pop("sample_every")))
    return g


def keep_three_body_golden(golden_dir: str, names: Optional[List[str]] = None) -> None:
    """After `python oracle/make_golden.py <THREE_BODY_FIXTURES>` (or <DISP_FIXTURES>, names = DISP_FIXTURES): keep each box's scalar
    results (energies, counts, cell) and drop the per-atom arrays and the box text.  The tests of these terms compare nothing else, and
    they regenerate the boxes with `materialize`, which writes the same bytes the reference read."""
    import json

    for name in (names or THREE_BODY_FIXTURES):
        path = os.path.join(golden_dir, f"{name}.json")
        with open(path) as f:
            res = json.load(f)
        res = {k: v for k, v in res.items() if not isinstance(v, list) or k in ("basis", "reciprocal_basis")}
        with open(path, "w") as f:
            json.dump(res, f, separators=(",", ":"))
            f.write("\n")
        for ext in (".in", ".pqr"):
            if os.path.exists(os.path.join(golden_dir, name + ext)):
                os.remove(os.path.join(golden_dir, name + ext))


def materialize(name: str, outdir: str):
    """write NAME.pqr / NAME.in into outdir; returns (in_path, pqr_path)."""
    rows, basis, opts = fixture(name)
    os.makedirs(outdir, exist_ok=True)
    pqr = os.path.join(outdir, f"{name}.pqr")
    inp = os.path.join(outdir, f"{name}.in")
    write_pqr(pqr, rows)
    write_input(inp, f"{name}.pqr", basis, opts)
    return inp, pqr


if __name__ == "__main__":
    import sys

    if sys.argv[1:2] == ["--keep-three-body-golden"]:
        keep_three_body_golden(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden"))
        sys.exit(0)
    if sys.argv[1:2] == ["--keep-direct-golden"]:
        keep_direct_golden(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden"))
        sys.exit(0)
    if sys.argv[1:2] == ["--keep-wolf-golden"]:
        keep_wolf_golden(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden"))
        sys.exit(0)
    if sys.argv[1:2] == ["--keep-rd-crystal-golden"]:
        keep_rd_crystal_golden(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden"))
        sys.exit(0)
    if sys.argv[1:2] == ["--keep-rd-model-golden"]:
        keep_rd_model_golden(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden"))
        sys.exit(0)
    if sys.argv[1:2] == ["--keep-sg-golden"]:
        keep_sg_golden(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden"))
        sys.exit(0)
    if sys.argv[1:2] == ["--keep-ewald-full-golden"]:
        keep_ewald_full_golden(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden"))
        sys.exit(0)
    if sys.argv[1:2] == ["--keep-relax-golden"]:
        keep_relax_golden(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden"))
        sys.exit(0)
    if sys.argv[1:2] == ["--keep-gs-ranked-golden"]:
        keep_gs_ranked_golden(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden"))
        sys.exit(0)
    if sys.argv[1:2] == ["--keep-disp-golden"]:
        keep_three_body_golden(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden"), DISP_FIXTURES)
        sys.exit(0)
    out = sys.argv[1] if len(sys.argv) > 1 else "."
    for nm in (sys.argv[2:] or SMALL_FIXTURES):
        print(materialize(nm, out))
