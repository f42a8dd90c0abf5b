#!/usr/bin/env python3
"""Cost of `polar_gs_ranked` at 10 000 atoms (the box ion10k_polar, 4 sweeps) on one GPU, against plain polar_gs on the same box.

Per configuration (gs4: polar_gs; ranked4: polar_gs_ranked) evaluations per second with one evaluation at a time (mpmc_energy in a loop)
and with `--beads` contexts in flight (mpmc_energy_async on all of them, then the waits), the configurations one after the other inside a
repetition and the repetitions interleaved; then, under mpmc_set_profiling, the device milliseconds per evaluation of every kernel class
(mpmc_get_timings): the rank pass, the order, the gathers and the view's tile classes are MPMC_K_CLASSES, the second block build is
MPMC_K_TENSOR.  MPMC_ENERGY_LIB names another build of the library (the parent's, for its polar_gs beside this one's): run the tool once
per build inside one job, alternating, with `--configs gs4` for a build without the setter.

usage: python tools/polar_gs_ranked_rate.py [--configs gs4,ranked4] [--reps 3] [--beads 32] [--evals 10] [--rounds 3] [--label TEXT] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"gs4": {"polar_gs": 1, "polar_max_iter": 4}, "ranked4": {"polar_gs_ranked": 1, "polar_max_iter": 4}}


def measure(label, case, beads, evals, rounds):
    from mpmcxx_amd import energy

    atoms, basis, opts = case
    systems = [energy.System(atoms, basis, opts) for _ in range(beads)]
    rec = {"config": label}
    try:
        S = systems[0]
        for _ in range(2):
            S.energy()
        t0 = time.perf_counter()
        for _ in range(evals):
            S.energy()
        rec["alone_per_s"] = evals / (time.perf_counter() - t0)
        rec["polarization_energy"] = S.observables["polarization_energy"]
        rec["polar_iterations"] = S.observables["polar_iterations"]
        for s in systems:
            s.hint_in_flight(beads)
        for r in range(rounds + 1):  # (the first round warms the other contexts up)
            if r == 1:
                t0 = time.perf_counter()
            for s in systems:
                s.energy_async()
            for s in systems:
                s.energy_wait()
        rec["in_flight_per_s"] = rounds * beads / (time.perf_counter() - t0)
    finally:
        for s in systems:
            s.close()
    return rec


def classes(case, evals):
    """device ms per evaluation of every kernel class, one evaluation at a time under profiling"""
    from mpmcxx_amd import energy

    atoms, basis, opts = case
    S = energy.System(atoms, basis, opts)
    try:
        for _ in range(2):
            S.energy()
        S.set_profiling(True)
        S.timings(reset=True)
        for _ in range(evals):
            S.energy()
        t = S.timings()
        info = S.polar_gs_ranked_info() if opts.get("polar_gs_ranked") else None
        return {k: (v["ms"] / evals, v["launches"] // evals) for k, v in t.items() if v["launches"]}, info
    finally:
        S.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="gs4,ranked4")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--beads", type=int, default=32)
    ap.add_argument("--evals", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from mpmcxx_amd import energy, gen_box, pqr

    with tempfile.TemporaryDirectory() as d:
        inp, _ = gen_box.materialize("ion10k_polar", d)
        atoms, basis, o = pqr.load_case(inp)
    configs = [c for c in a.configs.split(",") if c]
    lines = [f"# tools/polar_gs_ranked_rate.py {a.label} on {energy.device_name(0)}: ion10k_polar, {a.reps} interleaved repetitions, {a.evals} evaluations "
             f"alone, {a.rounds} rounds of {a.beads} in flight"]
    recs = []
    for rep in range(1, a.reps + 1):
        for label in configs:
            r = measure(label, (atoms, basis, dict(o, **CONFIGS[label])), a.beads, a.evals, a.rounds)
            r["rep"] = rep
            recs.append(r)
            lines.append(f"rep{rep} {label:8s} alone {r['alone_per_s']:8.1f} /s   {a.beads} in flight {r['in_flight_per_s']:8.1f} /s   "
                         f"iterations {r['polar_iterations']:2d}  polarization {r['polarization_energy']!r} K")
            print(lines[-1], flush=True)
    for key in ("alone_per_s", "in_flight_per_s"):
        for label in configs:
            v = [r[key] for r in recs if r["config"] == label]
            lines.append(f"{key:16s} {label:8s} min {min(v):8.1f}  median {sorted(v)[len(v) // 2]:8.1f}  max {max(v):8.1f}")
            print(lines[-1])
    for label in configs:
        t, info = classes((atoms, basis, dict(o, **CONFIGS[label])), a.evals)
        lines.append(f"classes {label:8s} " + "  ".join(f"{k} {ms:.3f} ms / {n} brackets" for k, (ms, n) in t.items()) + (f"  info {info}" if info else ""))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
            f.write("\n".join("# " + json.dumps(r) for r in recs) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
