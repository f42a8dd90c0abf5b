#!/usr/bin/env python3
"""Cost of one volume move on one GPU: the volume trial (mpmc_trial_volume_begin + mpmc_trial_energy + accept / reject) beside the
hand-built route of tests/test_gpu_box_moves.py (set_box + update_positions + energy; a reject is the way back plus the energy() that
re-bases the trial-move totals), on the 10 000-atom LJ + Ewald box (`ion10k_es`) and the polarizable one (`ion10k_polar`).

Per box and route: wall-clock milliseconds per move, median [min .. max] over `--moves` moves after `--warmup`, rejected and accepted
moves apart; the two routes are taken in turn inside every repetition.  The scale factors alternate 1.001 / 1 / 1.001 so that the cell
stays where it started.  Then, in a pass of its own under mpmc_set_profiling, the scaling kernel's own time: the MPMC_K_CLASSES class of
a volume trial minus that of a plain energy().  Usage: python tools/volume_trial_rate.py [--moves 20] [--warmup 5] [--out FILE]"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpmcxx_amd import energy, gen_box, pqr  # noqa: E402


def stat(v):
    return f"{statistics.median(v):.3f} [{min(v):.3f} .. {max(v):.3f}]"


def host_scale(pos, mass, starts, s):
    """the route's own host pass: per-molecule centres by segment sums (any arithmetic does: the route uploads what it computed)"""
    w = mass[:, None] * pos
    com = np.add.reduceat(w, starts[:-1]) / np.add.reduceat(mass, starts[:-1])[:, None]
    return pos + np.repeat(com * s - com, np.diff(starts), axis=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--moves", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [f"volume moves: trial against set_box + update_positions + energy; {a.moves} moves after {a.warmup} warm-up, ms per move, median [min .. max]",
             f"device: {energy.device_name(0)}", ""]
    for name in ("ion10k_es", "ion10k_polar"):
        with tempfile.TemporaryDirectory() as d:
            inp, _ = gen_box.materialize(name, d)
            atoms, basis, opts = pqr.load_case(inp)
        basis = np.asarray(basis, dtype=np.float64)
        ids = atoms["mol_id"]
        starts = np.array([0] + [i for i in range(1, len(ids)) if ids[i] != ids[i - 1]] + [len(ids)])
        mass = np.asarray(atoms["mass"], dtype=np.float64)
        s_up = 1.001
        T = energy.System(atoms, basis, opts)  # the trial route
        R = energy.System(atoms, basis, opts)  # the hand-built route
        T.energy()
        R.energy()
        t = {k: [] for k in ("trial_reject", "trial_accept", "route_reject", "route_accept")}
        for rep in range(a.warmup + a.moves):
            keep = rep >= a.warmup
            # rejected move
            t0 = time.perf_counter()
            T.trial_volume_energy(s_up)
            T.reject()
            t1 = time.perf_counter()
            pos0 = np.array(R.atoms["pos"])
            R.set_box(basis * s_up)
            R.update_positions(0, host_scale(pos0, mass, starts, s_up))
            R.energy()
            R.set_box(basis)
            R.update_positions(0, pos0)
            R.energy()  # (re-bases: the next trial needs an accepted configuration)
            t2 = time.perf_counter()
            if keep:
                t["trial_reject"].append(1e3 * (t1 - t0))
                t["route_reject"].append(1e3 * (t2 - t1))
            # accepted move, up and then back down so that the cell stays put
            for s in (s_up, 1.0 / s_up):
                t0 = time.perf_counter()
                T.trial_volume_energy(s)
                T.accept()
                t1 = time.perf_counter()
                b = np.array(R.basis) * s
                R.set_box(b)
                R.update_positions(0, host_scale(np.array(R.atoms["pos"]), mass, starts, s))
                R.energy()
                t2 = time.perf_counter()
                if keep:
                    t["trial_accept"].append(1e3 * (t1 - t0))
                    t["route_accept"].append(1e3 * (t2 - t1))
            R.set_box(basis)  # (the two routes round differently on the way back: both start the next repetition from the same cell and list)
            R.update_positions(0, np.array(atoms["pos"]))
            R.energy()
            T.set_box(basis)
            T.update_positions(0, np.array(atoms["pos"]))
            T.energy()
        counts = T.volume_trial_counts()
        # the scaling kernel's own time
        T.set_profiling(True)
        T.timings(reset=True)
        for _ in range(a.moves):
            T.energy()
        plain = T.timings(reset=True)["classes"]
        for _ in range(a.moves):
            T.trial_volume_energy(s_up)
            T.reject()
        vol = T.timings(reset=True)["classes"]
        T.set_profiling(False)
        lines += [f"{name}: {len(ids)} atoms, {len(starts) - 1} molecules",
                  f"  rejected  trial {stat(t['trial_reject'])}   route {stat(t['route_reject'])}   ratio of medians {statistics.median(t['route_reject']) / statistics.median(t['trial_reject']):.2f}",
                  f"  accepted  trial {stat(t['trial_accept'])}   route {stat(t['route_accept'])}   ratio of medians {statistics.median(t['route_accept']) / statistics.median(t['trial_accept']):.2f}",
                  f"  MPMC_K_CLASSES per evaluation: plain energy() {plain['ms'] / a.moves:.4f} ms in {plain['launches'] / a.moves:.1f} brackets, volume trial {vol['ms'] / a.moves:.4f} ms in "
                  f"{vol['launches'] / a.moves:.1f} brackets: the scaling kernel {(vol['ms'] - plain['ms']) / a.moves:.4f} ms",
                  f"  counters: {counts}", ""]
        T.close()
        R.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
