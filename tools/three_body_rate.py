#!/usr/bin/env python3
"""Rate of the Axilrod-Teller kernels (kernels_three_body.hip) on one GPU: unique triples per second of the full sum, time of the
trial-move difference.

Boxes: jittered lattices of single-site atoms (gen_box.lattice_box / lattice_box_cell, the c9 of gen_box.AT_C9) at 1 000, 4 000 and
10 000 atoms in cubic cells at the density of the 10 000-atom benchmark box, plus one triclinic cell.  Per box: one warm evaluation, then
`reps` calls of the component entry point mpmc_axilrod_teller with HIP-event timing of the three-body slot (MPMC_K_THREE_BODY = 6: the
full kernel and its fixed-order sum) and the host wall time around each call.  Rate = n (n - 1) (n - 2) / 6 / kernel time.  The delta:
`reps` trial moves of one 3-atom block at 10 000 atoms (rejected), slot 6 time per trial.

usage: python tools/three_body_rate.py [--reps R] [--out FILE.json]
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

K_THREE_BODY = 6


def case(n, basis=None):
    L = 86.0 * (n / 10000.0) ** (1.0 / 3.0)
    if basis is None:
        rows, basis = gen_box.lattice_box(n, L, 13), gen_box.cubic(L)
    else:
        rows = gen_box.lattice_box_cell(n, basis, 22)
    rows = gen_box._with_c9(rows, gen_box.AT_C9)
    atoms = {
        "pos": np.array([[r.x, r.y, r.z] for r in rows]), "charge": np.array([r.charge_e * 408.7816 for r in rows]),
        "polarizability": np.array([r.alpha for r in rows]), "epsilon": np.array([r.eps for r in rows]),
        "sigma": np.array([r.sigma for r in rows]), "mass": np.array([r.mass for r in rows]),
        "mol_id": np.arange(n, dtype=np.int32), "frozen": np.zeros(n, np.int32), "has_disp": np.zeros(n, np.int32),
        "c6": np.zeros(n), "c9": np.array([r.c9 for r in rows]),
    }
    opts = {"ewald_kmax": 7, "axilrod_teller": 1}
    return atoms, np.array(basis, dtype=np.float64), opts


def slot_ms(S):
    t = energy.Timings()
    S._check(S._L.mpmc_get_timings(S.handle, C.byref(t), 1))
    return t.ms[K_THREE_BODY], t.launches[K_THREE_BODY]


def full_rate(label, atoms, basis, opts, reps):
    S = energy.System(atoms, basis, opts)
    e = S.energy()
    S._check(S._L.mpmc_set_profiling(S.handle, 1))
    slot_ms(S)
    walls, kern = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        v = S.axilrod_teller()
        walls.append(time.perf_counter() - t0)
        ms, nl = slot_ms(S)
        kern.append(ms / 1e3)
    n = atoms["pos"].shape[0]
    triples = n * (n - 1) * (n - 2) // 6
    S.close()
    rec = {"box": label, "n": n, "triples": triples, "three_body_energy": v, "total_energy": e, "kernel_s": kern, "wall_s": walls,
           "triples_per_s_kernel": triples / min(kern), "triples_per_s_wall": triples / min(walls)}
    print(f"{label:>22s}: n={n:6d}  kernel {min(kern) * 1e3:9.3f} ms  wall {min(walls) * 1e3:9.3f} ms  "
          f"{rec['triples_per_s_kernel']:.3e} triples/s", flush=True)
    return rec


def delta_time(atoms, basis, opts, reps):
    S = energy.System(atoms, basis, opts)
    S.energy()
    S._check(S._L.mpmc_set_profiling(S.handle, 1))
    slot_ms(S)
    rng = np.random.default_rng(5)
    kern, walls = [], []
    for r in range(reps):
        first = int(rng.integers(0, atoms["pos"].shape[0] - 3))
        new = atoms["pos"][first:first + 3] + rng.normal(scale=0.2, size=(3, 3))
        t0 = time.perf_counter()
        S.trial_energy(first, new)
        walls.append(time.perf_counter() - t0)
        assert not S.last_trial_was_full()
        S.reject()
        ms, nl = slot_ms(S)
        kern.append(ms / 1e3)
    S.close()
    print(f"delta, 3-atom move at {atoms['pos'].shape[0]} atoms: kernels {min(kern) * 1e3:.3f} ms, trial wall {min(walls) * 1e3:.3f} ms", flush=True)
    return {"n": int(atoms["pos"].shape[0]), "m": 3, "kernel_s": kern, "wall_s": walls}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rec = {"device": energy.device_name(0), "full": [], "delta": None}
    for n in (1000, 4000, 10000):
        rec["full"].append(full_rate(f"cubic {n}", *case(n), a.reps))
    tri = [[44.0, 0.0, 0.0], [5.5, 42.0, 0.0], [-4.0, 6.5, 41.0]]
    rec["full"].append(full_rate("triclinic 4000", *case(4000, tri), a.reps))
    rec["delta"] = delta_time(*case(10000), max(a.reps, 5))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
