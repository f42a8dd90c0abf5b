#!/usr/bin/env python3
"""Cost of one cavity-grid update (mpmc_cavity_update) on the generated 10 000-atom LJ + Ewald box, next to a displacement trial and an
exchange trial of the same context in the same run.
usage: python tools/cavity_rate.py [--out profiles/cavity_grid.txt] [--reps 30]
Per grid size G = 10, 25, 50 the sphere radius is the one of a fixed ladder that leaves the fraction of empty centres closest to one half
(it must lie between a tenth and nine tenths); the darts are the reference's (int)(0.1 V).  Wall clock: median and range of `reps` calls through
ctypes with every argument prepared outside the timed loop.  Kernel times: HIP events around the three kernel groups (mpmc_set_profiling),
median over the same calls.  The reference's own host time for the call is not measurable with the committed harness and is not estimated."""
import ctypes as C
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mpmcxx_amd import energy, gen_box, pqr  # noqa: E402

dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
LADDER = [1.0, 1.25, 1.5, 1.75, 2.0, 2.25, 2.5, 2.75, 3.0, 3.5, 4.0]


def main():
    args = sys.argv[1:]
    out_path = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "cavity_grid.txt")
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 30
    name = "ion10k_es"
    inp, _ = gen_box.materialize(name, tempfile.mkdtemp())
    atoms, basis, opts = pqr.load_case(inp)
    opts = dict(opts, polarization=0, polar_iterative=0)
    n = len(atoms["pos"])
    S = energy.System(atoms, basis, opts, max_atoms=n + 64)
    L, h = S._L, S.handle
    volume = energy.pbc_compute(basis)[1]
    n_darts = energy.cavity_num_darts(volume)
    frac = np.ascontiguousarray(-0.5 + np.random.default_rng(3).random((n_darts, 3)))
    res = energy.CavityResult()
    lines = [f"device: {energy.device_name(0)}", f"box: {name}, {n} atoms, volume {volume:.1f} A^3, {n_darts} darts per update, {reps} updates per line",
             "wall: time.perf_counter around mpmc_cavity_update (upload of the wrapped positions and darts, six launches, one stream synchronisation);",
             "kernels: HIP events on the context's stream, median over the same calls", ""]

    def ok(rc):
        if rc != 0:
            raise energy.MpmcError(rc, (L.mpmc_last_error(h) or b"").decode())

    S.energy()
    for G in (10, 25, 50):
        best = None
        for radius in LADDER:
            S.set_cavity_grid(G, radius)
            r = S.cavity_update(None)
            if 0.1 <= r["probability"] <= 0.9 and (best is None or abs(r["probability"] - 0.5) < abs(best[1] - 0.5)):
                best = (radius, r["probability"])
        if best is None:
            raise SystemExit(f"G = {G}: no radius of the ladder leaves between a tenth and nine tenths of the centres empty")
        radius = best[0]
        S.set_cavity_grid(G, radius)
        S.set_profiling(True)
        ok(L.mpmc_cavity_update(h, n_darts, dp(frac), C.byref(res)))  # (the first call allocates)
        wall, kern = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            ok(L.mpmc_cavity_update(h, n_darts, dp(frac), C.byref(res)))
            wall.append(time.perf_counter() - t0)
            kern.append(list(S.cavity_times().values()))
        S.set_profiling(False)
        plain = []
        for _ in range(reps):
            t0 = time.perf_counter()
            ok(L.mpmc_cavity_update(h, n_darts, dp(frac), C.byref(res)))
            plain.append(time.perf_counter() - t0)
        k = np.median(np.array(kern), axis=0) * 1e3
        us = lambda v: 1e6 * np.array(v)
        lines += [f"G = {G}: radius {radius} A, {res.cavities_open} of {res.total_points} centres empty ({res.probability:.3f}), {res.hits} of {res.n_darts} darts hit, "
                  f"cavity_volume {res.cavity_volume:.1f} A^3",
                  f"  distance tests: occupancy G^3 N = {G ** 3 * n:.3e}, darts x open = {n_darts * res.cavities_open:.3e} at most (a wave leaves once all its darts have hit)",
                  f"  mpmc_cavity_update wall: median {np.median(us(plain)):.1f} us, range {us(plain).min():.1f} - {us(plain).max():.1f} us"
                  f"   (with the events recorded: median {np.median(us(wall)):.1f} us)",
                  f"  kernels: occupancy {k[0]:.1f} us, compaction (3 launches) {k[1]:.1f} us, darts + sum {k[2]:.1f} us", ""]

    # a 3-atom displacement trial and an exchange trial of the same context, rejected each time
    m = 3
    rng = np.random.default_rng(7)
    moved = [np.ascontiguousarray(atoms["pos"][:m] + rng.normal(scale=0.15, size=(m, 3))) for _ in range(reps)]
    r = energy.Result()
    f = lambda key: np.ascontiguousarray(atoms[key][:1], dtype=np.float64)
    g = lambda key: np.ascontiguousarray(atoms[key][:1], dtype=np.int32)
    q, al, ep, sg, ms, fr, hd = f("charge"), f("polarizability"), f("epsilon"), f("sigma"), f("mass"), g("frozen"), g("has_disp")
    ok(L.mpmc_cavity_update(h, n_darts, dp(frac), C.byref(res)))
    spots = [np.ascontiguousarray(S.cavity_point(int(k)).reshape(1, 3)) for k in rng.integers(0, res.cavities_open, size=reps)]

    def displace(k):
        ok(L.mpmc_trial_begin(h, 0, m, dp(moved[k])))
        ok(L.mpmc_trial_energy(h, C.byref(r)))
        ok(L.mpmc_trial_reject(h))

    def insert(k):
        ok(L.mpmc_trial_insert_begin(h, 0, 1, dp(spots[k]), dp(q), dp(al), dp(ep), dp(sg), ip(fr), ip(hd), dp(ms)))
        ok(L.mpmc_trial_energy(h, C.byref(r)))
        ok(L.mpmc_trial_reject(h))

    for label, fn in (("3-atom displacement trial (rejected)", displace), ("exchange trial: one ion inserted on an empty centre (rejected)", insert)):
        fn(0)
        t = []
        for k in range(reps):
            t0 = time.perf_counter()
            fn(k)
            t.append(time.perf_counter() - t0)
        t = 1e6 * np.array(t)
        lines.append(f"{label}: median {np.median(t):.1f} us, range {t.min():.1f} - {t.max():.1f} us")
    assert not S.last_trial_was_full()
    lines += ["", "The reference's own host time for System::cavity_update_grid is not measurable with the committed harness (oracle/ builds the energy path",
              "only); none is estimated here."]
    S.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fo:
        fo.write(text)


if __name__ == "__main__":
    main()
