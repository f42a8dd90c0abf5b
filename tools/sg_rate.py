#!/usr/bin/env python3
"""Rate of the Silvera-Goldman kernels (kernels_sg.hip) on one GPU, beside the disp-expansion term on the same positions.

Box: lattice_box(N, L, 13) at hydrogen's liquid density (3.75 A between sites), single-site molecules of two masses; cutoff L / 2.  Per
size (10 000 and 1 000 atoms) and variant -- sg, sg + feynman_hibbs, and as the yardstick the disp-expansion term (every pair, no cutoff,
rd_only) -- the variants taken in turn inside every repetition:
  - the sum: wall time of System.energy() and the HIP-event time of MPMC_K_PAIR (the pair-term walk and its fixed-order reduction;
    under disp-expansion also the LJ pair pass, which the Silvera-Goldman evaluation does not run), median [min .. max];
  - a one-atom trial move (trial_energy + reject): wall time.
Kept terms per second = n_terms / the event time.

usage: python tools/sg_rate.py [--reps R] [--sizes 10000,1000] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mpmcxx_amd import energy, gen_box, pqr  # noqa: E402

K_PAIR = 0
VARIANTS = [("sg", {"sg": "on"}), ("sg+fh", {"sg": "on", "feynman_hibbs": "on", "temperature": 30.0}), ("disp-expansion", None)]


def case(n, extra):
    k = int(np.ceil(n ** (1.0 / 3.0) - 1e-9))
    L = 3.75 * k
    rows = gen_box.lattice_box(n, L, 13, charged=False, alpha=0.0)
    if extra is None:
        rows = gen_box._with_disp(rows)
        opts = dict(gen_box.DISP_OPTS, rd_only="on")
    else:
        for i, r in enumerate(rows):
            r.mass, r.eps, r.sigma = (4.028 if i % 2 else 2.016), 34.2, 2.96
        opts = dict(extra)
    with tempfile.TemporaryDirectory() as d:
        gen_box.write_pqr(os.path.join(d, "b.pqr"), rows)
        gen_box.write_input(os.path.join(d, "b.in"), "b.pqr", gen_box.cubic(L), opts)
        return pqr.load_case(os.path.join(d, "b.in"))


def pair_ms(S):
    t = energy.Timings()
    S._check(S._L.mpmc_get_timings(S.handle, C.byref(t), 1))
    return t.ms[K_PAIR]


def stat(v):
    return f"{np.median(v):.4f} [{min(v):.4f} .. {max(v):.4f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--sizes", default="10000,1000")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    print(f"device: {energy.device_name(0)}", flush=True)
    out = {}
    for n in [int(v) for v in a.sizes.split(",")]:
        lone = {name: energy.System(*case(n, extra)) for name, extra in VARIANTS}
        for S in lone.values():
            S.energy()
            S.energy()
            S.set_profiling(True)
            pair_ms(S)
        wall = {name: [] for name in lone}
        kern = {name: [] for name in lone}
        for _ in range(a.reps):
            for name, S in lone.items():
                t0 = time.perf_counter()
                S.energy()
                wall[name].append((time.perf_counter() - t0) * 1e3)
                kern[name].append(pair_ms(S))
        for S in lone.values():
            S.set_profiling(False)
        trial = {name: [] for name in lone}
        rng = np.random.default_rng(5)
        for _ in range(a.reps):
            i = int(rng.integers(0, n))
            for name, S in lone.items():
                new = S.atoms["pos"][i:i + 1] + rng.normal(scale=0.2, size=(1, 3))
                t0 = time.perf_counter()
                S.trial_energy(i, new)
                trial[name].append((time.perf_counter() - t0) * 1e3)
                S.reject()
        print(f"\n{n} atoms, cutoff {lone['sg'].silvera_goldman_info()['cutoff']:.3f} A, {a.reps} repetitions (ms, median [min .. max])")
        for name, S in lone.items():
            terms = S.silvera_goldman_info()["n_terms"] if name != "disp-expansion" else n * (n - 1) // 2
            rate = terms / (np.median(kern[name]) * 1e-3)
            print(f"  {name:<15s} energy() wall {stat(wall[name])}   MPMC_K_PAIR {stat(kern[name])}   terms {terms}   {rate:.3e} terms/s   "
                  f"one-atom trial wall {stat(trial[name])}   last trial full: {S.last_trial_was_full()}")
            out[f"{n}/{name}"] = {"wall_ms": wall[name], "pair_ms": kern[name], "trial_ms": trial[name], "terms": int(terms)}
            S.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f)


if __name__ == "__main__":
    main()
