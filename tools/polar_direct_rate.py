#!/usr/bin/env python3
"""Rate of the direct dipole solve (`polar_iterative off`, kernels_chol.hip) on one GPU: time per evaluation and achieved fp64 flop rate
of the factorisation at 1 000, 4 000 and 10 000 atoms.

Boxes: jittered lattices of single-site polarizable ions (gen_box.lattice_box) in cubic cells at the density of the 10 000-atom benchmark
box, Ewald + polarization with `polar_iterative off`.  Per box, in a child process of its own with a time limit: `warmup` evaluations,
then `reps` evaluations with the library's HIP-event profiling; reported are the means over the repetitions of the wall time per
evaluation, of slot MPMC_K_DIPOLE_ITER (factorisation + the two triangular solves, one event pair around all their launches) and of
slot MPMC_K_TENSOR (the build of A).  Flop rate = (3 n)^3 / 3 / (slot MPMC_K_DIPOLE_ITER): the solves' 2 (3 n)^2 flops are not counted, so
the figure is a lower bound of the factorisation's own rate.  Peak: the fp64 matrix rate given with --peak-tflops (MI355X: 78.6).

usage: python tools/polar_direct_rate.py [--reps R] [--warmup W] [--sizes 1000,4000,10000] [--limit SECONDS] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K_TENSOR, K_DIPOLE_ITER = 3, 4


def one(n, reps, warmup):
    import tempfile

    import numpy as np

    from mpmcxx_amd import energy, gen_box, pqr

    L = 86.0 * (n / 10000.0) ** (1.0 / 3.0)
    with tempfile.TemporaryDirectory() as d:
        gen_box.write_pqr(os.path.join(d, "b.pqr"), gen_box.lattice_box(n, L, 13))
        gen_box.write_input(os.path.join(d, "b.in"), "b.pqr", gen_box.cubic(L), dict(gen_box.POLAR_OPTS, polar_iterative="off"))
        atoms, basis, opts = pqr.load_case(os.path.join(d, "b.in"))
    S = energy.System(atoms, basis, opts)
    for _ in range(warmup):
        S.energy()
    S.set_profiling(True)
    t = energy.Timings()
    S._check(S._L.mpmc_get_timings(S.handle, C.byref(t), 1))
    walls, fact, build = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        S.energy()
        walls.append(time.perf_counter() - t0)
        S._check(S._L.mpmc_get_timings(S.handle, C.byref(t), 1))
        fact.append(t.ms[K_DIPOLE_ITER] / 1e3)
        build.append(t.ms[K_TENSOR] / 1e3)
    info = S.direct_info()
    rec = {"n": n, "unknowns": info["n_unknowns"], "residual": info["residual"], "status": info["status"], "factor_bytes": info["factor_bytes"],
           "polarization_energy": S.observables["polarization_energy"], "wall_s": walls, "factor_solve_s": fact, "build_s": build,
           "flops": info["n_unknowns"] ** 3 / 3.0, "device": energy.device_name(0)}
    rec["tflops"] = rec["flops"] / float(np.mean(fact)) / 1e12
    S.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="1000,4000,10000")
    ap.add_argument("--limit", type=int, default=240, help="seconds per size (each runs in a child process of its own)")
    ap.add_argument("--peak-tflops", type=float, default=78.6)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", type=int, default=0)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(one(a.child, a.reps, a.warmup)))
        return 0
    out = []
    for n in [int(x) for x in a.sizes.split(",")]:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n), "--reps", str(a.reps), "--warmup", str(a.warmup)],
                           stdout=subprocess.PIPE, text=True, timeout=a.limit)
        if p.returncode != 0:  # nothing more is started on the device after a failed step
            print(f"n = {n}: exit status {p.returncode}", flush=True)
            return 1
        r = json.loads(p.stdout.strip().splitlines()[-1])
        mean = lambda v: sum(v) / len(v)
        r["fraction_of_peak"] = r["tflops"] / a.peak_tflops
        print(f"n = {n:6d}: evaluation {mean(r['wall_s']) * 1e3:9.3f} ms  factor + solves {mean(r['factor_solve_s']) * 1e3:9.3f} ms  build "
              f"{mean(r['build_s']) * 1e3:7.3f} ms  {r['tflops']:6.2f} Tflop/s fp64 = {100 * r['fraction_of_peak']:.1f} % of {a.peak_tflops}  "
              f"residual {r['residual']:.1e}", flush=True)
        out.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
