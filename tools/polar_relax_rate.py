#!/usr/bin/env python3
"""Rates of the relaxed dipole solves and of zeroth-order dipoles at 10 000 atoms (the box ion10k_polar) on one GPU.

Per configuration -- eager plain Jacobi (10 iterations), polar_sor 0.8, polar_esor 0.6, Gauss-Seidel 4 sweeps without and with polar_sor 0.9,
polar_zodid, and the non-polarizable box ion10k_es -- evaluations per second with one evaluation at a time (mpmc_energy in a loop) and with
`--beads` contexts in flight (mpmc_energy_async on all of them, then the waits), and for plain Jacobi and zodid single-atom trial moves
per second (mpmc_trial_begin / energy / reject).  The configurations are measured one after the other inside a repetition and the
repetitions are interleaved (`--reps` passes over the whole list), so a drift of the device shows as spread, not as a difference
between configurations.  The relaxed solves are to be read against plain Jacobi of the same run, zodid against ion10k_es (the gap is the
static field).

usage: python tools/polar_relax_rate.py [--reps 3] [--beads 32] [--evals 10] [--rounds 3] [--trials 40] [--out FILE]
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

CONFIGS = [  # (label, fixture, option changes, measure trial moves)
    ("jacobi10", "ion10k_polar", {}, True),
    ("sor0.8", "ion10k_polar", {"polar_sor": 1, "polar_gamma": 0.8}, False),
    ("esor0.6", "ion10k_polar", {"polar_esor": 1, "polar_gamma": 0.6}, False),
    ("gs4", "ion10k_polar", {"polar_gs": 1, "polar_max_iter": 4}, False),
    ("gs4+sor0.9", "ion10k_polar", {"polar_gs": 1, "polar_max_iter": 4, "polar_sor": 1, "polar_gamma": 0.9}, False),
    ("zodid", "ion10k_polar", {"polar_zodid": 1}, True),
    ("ion10k_es", "ion10k_es", {}, False),
]


def measure(label, case, beads, evals, rounds, trials, want_trials):
    import numpy as np

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
        if want_trials:
            S.hint_in_flight(1)
            S.energy()
            rng = np.random.default_rng(5)
            moves = [(int(i), atoms["pos"][i:i + 1] + rng.normal(scale=0.2, size=(1, 3))) for i in rng.integers(0, len(atoms["charge"]), size=trials + 3)]
            for k, (i, p) in enumerate(moves):
                if k == 3:
                    t0 = time.perf_counter()
                S.trial_energy(i, p)
                S.reject()
            rec["trials_per_s"] = trials / (time.perf_counter() - t0)
            rec["trial_was_full"] = bool(S.last_trial_was_full())
    finally:
        for s in systems:
            s.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--beads", type=int, default=32)
    ap.add_argument("--evals", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--trials", type=int, default=40)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from mpmcxx_amd import energy, gen_box, pqr

    cases = {}
    with tempfile.TemporaryDirectory() as d:
        for name in ("ion10k_polar", "ion10k_es"):
            inp, _ = gen_box.materialize(name, d)
            cases[name] = pqr.load_case(inp)
    lines = [f"# tools/polar_relax_rate.py on {energy.device_name(0)}: {a.reps} interleaved repetitions, {a.evals} evaluations alone, "
             f"{a.rounds} rounds of {a.beads} in flight, {a.trials} single-atom trial moves (rejected)"]
    recs = []
    for rep in range(1, a.reps + 1):
        for label, fixture, extra, want_trials in CONFIGS:
            atoms, basis, o = cases[fixture]
            r = measure(label, (atoms, basis, dict(o, **extra)), a.beads, a.evals, a.rounds, a.trials, want_trials)
            r["rep"] = rep
            recs.append(r)
            line = (f"rep{rep} {label:11s} alone {r['alone_per_s']:8.1f} /s   {a.beads} in flight {r['in_flight_per_s']:8.1f} /s   "
                    f"iterations {r['polar_iterations']:2d}  polarization {r['polarization_energy']!r} K")
            if want_trials:
                line += f"   trial moves {r['trials_per_s']:8.1f} /s (full evaluation: {r['trial_was_full']})"
            print(line, flush=True)
            lines.append(line)
    for key in ("alone_per_s", "in_flight_per_s", "trials_per_s"):
        for label, *_ in CONFIGS:
            v = [r[key] for r in recs if r["config"] == label and key in r]
            if v:
                line = f"{key:16s} {label:11s} min {min(v):8.1f}  median {sorted(v)[len(v) // 2]:8.1f}  max {max(v):8.1f}"
                print(line)
                lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
            f.write("\n".join("# " + json.dumps(r) for r in recs) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
