#!/usr/bin/env python3
"""Rate of the disp-expansion kernels (kernels_disp.hip) on one GPU: pairs per second of the all-pairs sum, time of the trial-move
difference, and the 10 000-atom disp + Ewald + polarization evaluation next to the same box with LJ.

Boxes: jittered lattices of single-site atoms (gen_box.lattice_box / lattice_box_cell with the two species of gen_box._with_disp, damped)
at 1 000, 4 000 and 10 000 atoms in cubic cells at the density of the 10 000-atom benchmark box, plus one triclinic cell.  Per box: one warm
evaluation, then `reps` calls of the component entry point mpmc_disp_expansion with HIP-event timing of slot 0 (MPMC_K_PAIR: the all-pairs
kernel and its fixed-order sum, nothing else runs in that call) and the host wall time around each call.  Rate = n (n - 1) / 2 / kernel
time.  The delta: `reps` trial moves of one 3-atom block at 10 000 atoms (rejected), slot 0 time per trial (the disp difference and the
Ewald pair difference) and the trial's wall time.  The comparison: full evaluations of the 10 000-atom Ewald + polarization box with the
term and with LJ (the same positions and charges), wall time and every timing slot.

usage: python tools/disp_expansion_rate.py [--reps R] [--only compare] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mpmcxx_amd import energy, gen_box  # noqa: E402

K_PAIR = 0
SLOTS = ["pair", "recip", "field", "tensor", "dipole_iter", "reduce", "three_body", "classes"]


def case(n, basis=None, polar=False, disp=True):
    """(atoms, basis, options) of a lattice box, through the reference-format files (gen_box writes them, pqr reads them back)"""
    import tempfile

    from mpmcxx_amd import pqr

    L = 86.0 * (n / 10000.0) ** (1.0 / 3.0)
    if basis is None:
        rows, basis = gen_box.lattice_box(n, L, 13), gen_box.cubic(L)
    else:
        rows = gen_box.lattice_box_cell(n, basis, 22)
    opts = dict(gen_box.POLAR_OPTS) if polar else {"ewald_kmax": 7}
    if disp:
        rows = gen_box._with_disp(rows)
        opts.update(gen_box.DISP_OPTS, damp_dispersion="on")
    with tempfile.TemporaryDirectory() as d:
        gen_box.write_pqr(os.path.join(d, "b.pqr"), rows)
        gen_box.write_input(os.path.join(d, "b.in"), "b.pqr", basis, opts)
        return pqr.load_case(os.path.join(d, "b.in"))


def slots(S):
    t = energy.Timings()
    S._check(S._L.mpmc_get_timings(S.handle, C.byref(t), 1))
    return [t.ms[k] for k in range(8)], [t.launches[k] for k in range(8)]


def full_rate(label, atoms, basis, opts, reps):
    S = energy.System(atoms, basis, opts)
    e = S.energy()
    S._check(S._L.mpmc_set_profiling(S.handle, 1))
    slots(S)
    walls, kern = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        v = S.disp_expansion()
        walls.append(time.perf_counter() - t0)
        ms, nl = slots(S)
        kern.append(ms[K_PAIR] / 1e3)
    n = atoms["pos"].shape[0]
    pairs = n * (n - 1) // 2
    S.close()
    rec = {"box": label, "n": n, "pairs": pairs, "rd_energy": v, "total_energy": e, "kernel_s": kern, "wall_s": walls,
           "pairs_per_s_kernel": pairs / min(kern), "pairs_per_s_wall": pairs / min(walls)}
    print(f"{label:>22s}: n={n:6d}  kernel {min(kern) * 1e3:8.3f} ms  wall {min(walls) * 1e3:8.3f} ms  {rec['pairs_per_s_kernel']:.3e} pairs/s",
          flush=True)
    return rec


def delta_time(atoms, basis, opts, reps):
    S = energy.System(atoms, basis, opts)
    S.energy()
    S._check(S._L.mpmc_set_profiling(S.handle, 1))
    slots(S)
    rng = np.random.default_rng(5)
    kern, walls = [], []
    for _ in range(reps):
        first = int(rng.integers(0, atoms["pos"].shape[0] - 3))
        new = atoms["pos"][first:first + 3] + rng.normal(scale=0.2, size=(3, 3))
        t0 = time.perf_counter()
        S.trial_energy(first, new)
        walls.append(time.perf_counter() - t0)
        assert not S.last_trial_was_full()
        S.reject()
        ms, nl = slots(S)
        kern.append(ms[K_PAIR] / 1e3)
    S.close()
    print(f"delta, 3-atom move at {atoms['pos'].shape[0]} atoms: slot 0 {min(kern) * 1e3:.3f} ms, trial wall {min(walls) * 1e3:.3f} ms", flush=True)
    return {"n": int(atoms["pos"].shape[0]), "m": 3, "slot0_s": kern, "wall_s": walls}


def evaluation(label, atoms, basis, opts, reps):
    S = energy.System(atoms, basis, opts)
    S.energy()
    S._check(S._L.mpmc_set_profiling(S.handle, 1))
    slots(S)
    walls, per = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        S.energy()
        walls.append(time.perf_counter() - t0)
        per.append(slots(S))
    best = int(np.argmin(walls))
    ms, nl = per[best]
    sweep = S.last_pair_kernel()
    r = dict(S.observables)
    S.close()
    print(f"{label:>22s}: evaluation {walls[best] * 1e3:8.3f} ms  pair kernels: {sweep}  slots(ms) "
          + " ".join(f"{SLOTS[k]}={ms[k]:.3f}" for k in range(8) if nl[k]), flush=True)
    return {"box": label, "wall_s": walls, "slots_ms": dict(zip(SLOTS, ms)), "slot_launches": dict(zip(SLOTS, nl)), "pair_kernel": sweep,
            "energy": r["energy"], "rd_energy": r["rd_energy"], "coulombic_energy": r["coulombic_energy"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", choices=["compare"], default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rec = {"device": energy.device_name(0), "full": [], "delta": None, "compare": []}
    if a.only is None:
        for n in (1000, 4000, 10000):
            rec["full"].append(full_rate(f"cubic {n}", *case(n), a.reps))
        tri = [[44.0, 0.0, 0.0], [5.5, 42.0, 0.0], [-4.0, 6.5, 41.0]]
        rec["full"].append(full_rate("triclinic 4000", *case(4000, tri), a.reps))
        rec["delta"] = delta_time(*case(10000), max(a.reps, 5))
    rec["compare"].append(evaluation("10k disp+Ewald+polar", *case(10000, polar=True), a.reps))
    rec["compare"].append(evaluation("10k LJ+Ewald+polar", *case(10000, polar=True, disp=False), a.reps))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
