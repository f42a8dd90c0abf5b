#!/usr/bin/env python3
"""Rate of the rd_crystal kernels (kernels_crystal.hip) on one GPU: image terms per second and evaluations per second of the lattice sum.

Boxes: rd_only jittered lattices of single-site atoms (gen_box.lattice_box) at 1 000 and 10 000 atoms in cubic cells at the density of the
10 000-atom benchmark box, orders 2 and 3.  Per box: two warm evaluations, then `reps` calls of mpmc_lj with HIP-event timing of slot 0
(MPMC_K_PAIR) and the host wall time around each call; every figure is the MEDIAN over the calls, with their range behind it.  Slot 0 of such a call holds the lattice-sum kernel with its two fixed-order sums AND
the plain pair sweep that still counts the pairs inside the box cutoff; the same box with the term off is timed next to it, and the rate is
image terms (mpmc_rd_crystal_info: the terms that passed |a| <= cut) / (median slot 0 with the term - median slot 0 without it).  "tested" counts every
(pair, image) the kernel looked at: n (n - 1) / 2 * (2 order - 1)^3.  The delta: `reps` trial moves of one 3-atom block (rejected).

usage: python tools/rd_crystal_rate.py [--reps R] [--sizes 1000,10000] [--orders 2,3]
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mpmcxx_amd import energy, gen_box  # noqa: E402

K_PAIR = 0


def case(n, order):
    """(atoms, basis, options) of an rd_only lattice box, through the reference-format files"""
    import tempfile

    from mpmcxx_amd import pqr

    L = 86.0 * (n / 10000.0) ** (1.0 / 3.0)
    rows, basis = gen_box.lattice_box(n, L, 13, charged=False, alpha=0.0), gen_box.cubic(L)
    opts = {"rd_only": "on"}
    if order:
        opts.update(rd_crystal="on", rd_crystal_order=order)
    with tempfile.TemporaryDirectory() as d:
        gen_box.write_pqr(os.path.join(d, "b.pqr"), rows)
        gen_box.write_input(os.path.join(d, "b.in"), "b.pqr", basis, opts)
        return pqr.load_case(os.path.join(d, "b.in"))


def slot0(S):
    t = energy.Timings()
    S._check(S._L.mpmc_get_timings(S.handle, C.byref(t), 1))
    return t.ms[K_PAIR] / 1e3


def stats(v):
    """(median, min, max)"""
    return float(np.median(v)), float(min(v)), float(max(v))


def span(t, unit=1e3):
    return f"{t[0] * unit:.3f} [{t[1] * unit:.3f} .. {t[2] * unit:.3f}]"


def lj_times(S, reps):
    S.energy()
    S.configure("single_launch", 0)  # (the plain box: the general path the box with the term takes too)
    S.lj()
    S.lj()
    S._check(S._L.mpmc_set_profiling(S.handle, 1))
    slot0(S)
    kern, walls = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        S.lj()
        walls.append(time.perf_counter() - t0)
        kern.append(slot0(S))
    return stats(kern), stats(walls)


def full_rate(n, order, reps):
    atoms, basis, opts = case(n, order)
    S = energy.System(atoms, basis, opts)
    k, w = lj_times(S, reps)
    info = S.rd_crystal_info()
    S.close()
    P = energy.System(*case(n, 0))
    k0, w0 = lj_times(P, reps)
    P.close()
    tested = n * (n - 1) // 2 * info["n_images"]
    dk = k[0] - k0[0]
    print(f"n={n:6d} order {order}: slot 0 {span(k)} ms (plain box {span(k0)} ms)  wall {span(w)} ms  {1.0 / w[0]:9.1f} evaluations/s\n"
          f"{'':18s}lattice sum {dk * 1e3:.3f} ms: tested {tested:.4e} (pair, image) terms {tested / dk:.3e}/s, kept {info['n_image_terms']:.4e} "
          f"{info['n_image_terms'] / dk:.3e}/s", flush=True)


def delta_time(n, order, reps):
    atoms, basis, opts = case(n, order)
    S = energy.System(atoms, basis, opts)
    S.energy()
    S._check(S._L.mpmc_set_profiling(S.handle, 1))
    slot0(S)
    rng = np.random.default_rng(5)
    kern, walls = [], []
    for _ in range(reps):
        first = int(rng.integers(0, n - 3))
        new = atoms["pos"][first:first + 3] + rng.normal(scale=0.2, size=(3, 3))
        t0 = time.perf_counter()
        S.trial_energy(first, new)
        walls.append(time.perf_counter() - t0)
        assert not S.last_trial_was_full()
        S.reject()
        kern.append(slot0(S))
    S.close()
    print(f"n={n:6d} order {order}: 3-atom trial move: slot 0 {span(stats(kern))} ms, wall {span(stats(walls))} ms", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--sizes", default="1000,10000")
    ap.add_argument("--orders", default="2,3")
    a = ap.parse_args()
    print(f"device: {energy.device_name(0)}", flush=True)
    for n in (int(v) for v in a.sizes.split(",")):
        for order in (int(v) for v in a.orders.split(",")):
            full_rate(n, order, a.reps)
    for n in (int(v) for v in a.sizes.split(",")):
        delta_time(n, 2, a.reps)


if __name__ == "__main__":
    main()
