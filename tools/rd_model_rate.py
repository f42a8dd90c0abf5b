#!/usr/bin/env python3
"""Rate of the rd-model kernels (kernels_rd_model.hip) on one GPU, beside the plain model and the disp-expansion term on the same atoms.

Box: lattice_box(10000, 86.0, 13) with the three species of gen_box.rd_model_species, LJ + Ewald (no polarization).  Variants: the plain
model (LJ, Lorentz-Berthelot: none of the new code runs), LJ + Waldman-Hagler, buffered 14-7 + Halgren, DREIDING + Lorentz-Berthelot, and as
the yardstick the disp-expansion term on the same positions (its own two species: every pair, no cutoff).  Per variant, the variants taken
in turn inside every repetition:
  - one evaluation at a time: wall time of System.energy() and the HIP-event time of MPMC_K_PAIR (the pair sweep plus, where there is one,
    the model's / the disp-expansion sum and its fixed-order reduction), median [min .. max] over the repetitions;
  - 32 evaluations in flight: 32 contexts, every step enqueues all of them before the first wait; evaluations per second.
The model's own kernel time is MPMC_K_PAIR minus the plain box's; kept terms per second = n_terms / that.  A 3-atom trial move per variant.

usage: python tools/rd_model_rate.py [--reps R] [--steps S] [--beads B] [--n N] [--out FILE.json]
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
VARIANTS = [("plain", {}), ("lj+wh", {"waldmanhagler": "on"}), ("14-7+halgren", {"lj_buffered_14_7": "on", "halgren_mixing": "on"}),
            ("dreiding+lb", {"dreiding": "on"}), ("disp-expansion", None)]


def case(n, extra):
    L = 86.0 * (n / 10000.0) ** (1.0 / 3.0)
    rows = gen_box.lattice_box(n, L, 13)
    opts = {"ewald_kmax": 7}
    if extra is None:
        rows = gen_box._with_disp(rows)
        opts.update(gen_box.DISP_OPTS, damp_dispersion="on")
    else:
        rows = gen_box.rd_model_species(rows)
        opts.update(extra)
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
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--beads", type=int, default=32)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    print(f"device: {energy.device_name(0)}", flush=True)
    cases = {name: case(a.n, extra) for name, extra in VARIANTS}
    # ---- one evaluation at a time --------------------------------------------------------------------------------------------------------
    lone = {name: energy.System(*cases[name]) for name, _ in VARIANTS}
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
    trial = {name: [] for name in lone}
    rng = np.random.default_rng(5)
    for _ in range(a.reps):
        first = int(rng.integers(0, a.n - 3))
        for name, S in lone.items():
            new = cases[name][0]["pos"][first:first + 3] + 0.2
            S.trial_energy(first, new)
            assert not S.last_trial_was_full()
            S.reject()
            trial[name].append(pair_ms(S))
    rec = {"n": a.n, "variants": {}}
    base = float(np.median(kern["plain"]))
    for name, S in lone.items():
        info = S.rd_model_info() if name not in ("plain", "disp-expansion") else None
        own = float(np.median(kern[name])) - base
        terms = info["n_terms"] if info else (a.n * (a.n - 1) // 2 if name == "disp-expansion" else 0)
        line = f"{name:>16s}: alone wall {stat(wall[name])} ms, MPMC_K_PAIR {stat(kern[name])} ms"
        if name != "plain":
            # (by subtraction: presumes the pair sweep costs the same with and without the model)
            rate = f"{terms / (own * 1e-3):.3e} terms/s" if own > 0.0 else "no rate (not above the plain box's time)"
            line += f", own kernel {own:.4f} ms, {terms} terms, {rate}"
        if info:
            line += f", tile pairs {info['n_tile_pairs']} of which skipped {info['n_tile_pairs_skipped']}"
        line += f"; 3-atom trial MPMC_K_PAIR {stat(trial[name])} ms"
        print(line, flush=True)
        rec["variants"][name] = {"wall_ms": wall[name], "k_pair_ms": kern[name], "own_kernel_ms": own, "terms": int(terms), "info": info,
                                 "rd_energy": S.observables["rd_energy"], "trial_k_pair_ms": trial[name]}
        S.close()
    # ---- in flight -----------------------------------------------------------------------------------------------------------------------
    ens = {name: [energy.System(*cases[name]) for _ in range(a.beads)] for name, _ in VARIANTS}
    for beads in ens.values():
        for S in beads:
            S.hint_in_flight(a.beads)
        for _ in range(2):
            for S in beads:
                S.energy_async()
            for S in beads:
                S.energy_wait()
    rates = {name: [] for name in ens}
    for _ in range(a.steps):
        for name, beads in ens.items():
            t0 = time.perf_counter()
            for S in beads:
                S.energy_async()
            for S in beads:
                S.energy_wait()
            rates[name].append(a.beads / (time.perf_counter() - t0))
    for name, beads in ens.items():
        print(f"{name:>16s}: {a.beads} in flight {np.median(rates[name]):9.1f} [{min(rates[name]):.1f} .. {max(rates[name]):.1f}] evaluations/s", flush=True)
        rec["variants"][name]["in_flight_per_s"] = rates[name]
        for S in beads:
            S.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f)


if __name__ == "__main__":
    main()
