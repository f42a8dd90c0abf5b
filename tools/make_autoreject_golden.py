#!/usr/bin/env python3
"""Goldens of cavity_autoreject (mpmc_set_cavity_autoreject) from the reference's own object code (build container only).

Every case is a committed fixture of mpmcxx_amd/gen_box.py with the reference's keywords `cavity_autoreject`, `cavity_autoreject_absolute`
and `cavity_autoreject_scale` appended to its input file.  The derived input is written to a temporary directory, oracle/_ref/ref_harness
(the reference's System::energy(), `make -C oracle ref`) evaluates it, and only its scalars are kept, in tests/golden/autoreject_cases.json:
    name -> {"base": fixture, "options": the changed / added keywords, "box": the committed box where positions are new, "result": scalars}
`total` is what System::energy() RETURNS (the absolute rule's MAXVALUE included); rd, lj_pairs and the other parts are the observables.

The two absolute-rule boxes are water64_polar with one molecule moved, by a seeded direction, so that one of its H atoms sits 0.8 A from
the O of another molecule: once inside the cell, once across a periodic face (the moved molecule one lattice vector further).  Their boxes
are committed as tests/golden/autoreject_abs_{cell,face}.{in,pqr} WITHOUT the keywords: the Python reader refuses those in a file.

Each constructed case is checked against what it was built to show before anything is written.
Usage: python tools/make_autoreject_golden.py
"""
from __future__ import annotations

import json
import math
import os
import random
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mpmcxx_amd import gen_box  # noqa: E402

HARNESS = os.path.join(ROOT, "oracle", "_ref", "ref_harness")
GOLDEN = os.path.join(ROOT, "tests", "golden")
OUT = "autoreject_cases.json"
MAXVALUE = 1e40

SIGMA = {"cavity_autoreject": "on"}
ABSOLUTE = {"cavity_autoreject_absolute": "on"}


def abs_box(face: bool):
    """water64_polar with molecule 6 moved so that its first H sits 0.8 A from the O of molecule 21 (face: through the periodic image)"""
    rows, basis, opts = gen_box.fixture("water64_polar")
    rng = random.Random(20240 + int(face))
    mover = [r for r in rows if r.mol_id == 6]
    target = next(r for r in rows if r.mol_id == 21 and r.atomtype == "O")
    h = mover[1]
    while True:  # a direction away from the target's own H atoms, so that the planted pair is the closest one
        u = [rng.gauss(0.0, 1.0) for _ in range(3)]
        norm = math.sqrt(sum(v * v for v in u))
        u = [v / norm for v in u]
        spot = (target.x + 0.8 * u[0], target.y + 0.8 * u[1], target.z + 0.8 * u[2])
        if all(math.dist(spot, (r.x, r.y, r.z)) > 1.3 for r in rows if r.mol_id == 21 and r.atomtype == "H"):
            break
    shift = [spot[0] - h.x, spot[1] - h.y, spot[2] - h.z]
    if face:
        shift[0] += basis[0][0]
    for r in mover:
        r.x, r.y, r.z = r.x + shift[0], r.y + shift[1], r.z + shift[2]
    return rows, basis, opts


# name -> (base fixture or builder, committed box name or None, option changes, check on the harness result)
def n_replaced(res):
    return round(res["lj_pairs"] / MAXVALUE)


CASES = {
    # the four measured in the issue
    "ion216_polar_s10": ("ion216_polar", None, dict(SIGMA, cavity_autoreject_scale=1.0), lambda r, p: n_replaced(r) == 16 and r["es"] == p["es"] and r["polar"] == p["polar"]),
    "ion216_polar_s08": ("ion216_polar", None, dict(SIGMA, cavity_autoreject_scale=0.8), lambda r, p: r["total"] == p["total"] and r["rd"] == p["rd"]),
    "water64_polar_s07": ("water64_polar", None, dict(SIGMA, cavity_autoreject_scale=0.7), lambda r, p: r["total"] == p["total"]),
    "water64_polar_s09": ("water64_polar", None, dict(SIGMA, cavity_autoreject_scale=0.9), lambda r, p: n_replaced(r) == 92),
    "water64_polar_s10": ("water64_polar", None, dict(SIGMA, cavity_autoreject_scale=1.0), lambda r, p: n_replaced(r) == 155),
    "ion216_frozen_nopol_s10": ("ion216_frozen", None, dict(SIGMA, cavity_autoreject_scale=1.0, polarization="off"), lambda r, p: n_replaced(r) == 15),
    "water64_polar_abs10": ("water64_polar", None, dict(ABSOLUTE, cavity_autoreject_scale=1.0), lambda r, p: r["total"] == p["total"]),
    "ion216_frozen_nopol_abs05": ("ion216_frozen", None, dict(ABSOLUTE, cavity_autoreject_scale=0.5, polarization="off"),
                                  lambda r, p: r["total"] == MAXVALUE and abs(r["rd"]) < 1e6),
    "ion216_frozen_abs05": ("ion216_frozen", None, dict(ABSOLUTE, cavity_autoreject_scale=0.5), lambda r, p: r["total"] == p["total"]),
    # a skewed cell, and the other potential forms with Waldman-Hagler mixing
    "ion216_triclinic_s10": ("ion216_triclinic", None, dict(SIGMA, cavity_autoreject_scale=1.0), lambda r, p: n_replaced(r) > 0 and r["es"] == p["es"]),
    "ion216_polar_rdm_b147wh_s10": ("ion216_polar_rdm_b147wh", None, dict(SIGMA, cavity_autoreject_scale=1.0), lambda r, p: n_replaced(r) > 0),
    "ion216_polar_rdm_drdwh_s10": ("ion216_polar_rdm_drdwh", None, dict(SIGMA, cavity_autoreject_scale=1.0), lambda r, p: n_replaced(r) > 0),
    # the disp-expansion term: its own sigma test (no cutoff) and, with a threshold, its repulsion test
    "ion216_disp_s10": ("ion216_disp", None, dict(SIGMA, cavity_autoreject_scale=1.0), lambda r, p: n_replaced(r) > 0 and r["es"] == p["es"]),
    "ion216_disp_s09_rep100": ("ion216_disp", None, dict(SIGMA, cavity_autoreject_scale=0.9, cavity_autoreject_repulsion=100.0),
                               lambda r, p: n_replaced(r) > 0),
    "ion216_disp_s09": ("ion216_disp", None, dict(SIGMA, cavity_autoreject_scale=0.9), lambda r, p: True),
    # the absolute rule on a planted intermolecular O-H pair at 0.8 A, in the cell and across a periodic face; both rules together
    "abs_cell_abs10": (lambda: abs_box(False), "autoreject_abs_cell", dict(ABSOLUTE, cavity_autoreject_scale=1.0),
                       lambda r, p: r["total"] >= MAXVALUE and abs(r["rd"]) < 1e9),
    "abs_face_abs10": (lambda: abs_box(True), "autoreject_abs_face", dict(ABSOLUTE, cavity_autoreject_scale=1.0),
                       lambda r, p: r["total"] >= MAXVALUE and abs(r["rd"]) < 1e9),
    "abs_face_both10": (lambda: abs_box(True), "autoreject_abs_face", dict(SIGMA, **ABSOLUTE, cavity_autoreject_scale=1.0),
                        lambda r, p: r["total"] >= MAXVALUE and n_replaced(r) > 0),
}


def run_harness(wd: str, in_name: str):
    p = subprocess.run([HARNESS, in_name], cwd=wd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if p.returncode != 0:
        raise RuntimeError(f"ref_harness failed on {in_name}:\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
    return json.loads(p.stdout[p.stdout.rfind("\n{") + 1:])


def evaluate(rows, basis, opts):
    with tempfile.TemporaryDirectory(prefix="autoreject_") as wd:
        gen_box.write_pqr(os.path.join(wd, "case.pqr"), rows)
        gen_box.write_input(os.path.join(wd, "case.in"), "case.pqr", basis, opts)
        res = run_harness(wd, "case.in")
    return {k: v for k, v in res.items() if not isinstance(v, list)}


def main():
    if not os.path.exists(HARNESS):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "ref"])
    out = {}
    for name, (base, box, changes, check) in CASES.items():
        rows, basis, opts = base() if callable(base) else gen_box.fixture(base)
        plain_opts = {k: v for k, v in dict(opts, **changes).items() if not k.startswith("cavity_autoreject")}
        plain = evaluate(rows, basis, plain_opts)
        res = evaluate(rows, basis, dict(opts, **changes))
        if not check(res, plain):
            raise SystemExit(f"{name}: the reference's result is not what the case was built to show: {res}\nplain: {plain}")
        if box:  # the box without the keywords, in the reference's on-disk formats
            gen_box.write_pqr(os.path.join(GOLDEN, box + ".pqr"), rows)
            gen_box.write_input(os.path.join(GOLDEN, box + ".in"), box + ".pqr", basis, opts)
        out[name] = {"base": base if isinstance(base, str) else None, "box": box, "options": changes, "result": res, "plain": plain}
        print(f"{name}: total={res['total']!r} rd={res['rd']!r} lj_pairs={res['lj_pairs']!r} (plain total {plain['total']!r})")
    with open(os.path.join(GOLDEN, OUT), "w") as f:
        json.dump(out, f, indent=0, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
