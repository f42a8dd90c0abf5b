#!/usr/bin/env python3
"""Cost of cavity_autoreject (mpmc_set_cavity_autoreject) next to the same build with the setting off, on the generated 10 000-atom
LJ + Ewald box (ion10k_es, polarization off) and the 1 000-atom LJ box (lj1000): one evaluation, one displacement trial of one atom, one
insertion trial of a rigid 3-site molecule and one batch of 256 insertion candidates.
usage: python tools/autoreject_rate.py [--out profiles/cavity_autoreject.txt] [--repeats 7] [--scale 1.0] [--off-only] [box ...]
A library named by MPMC_ENERGY_LIB that lacks the entry point (the parent build) gives the setting-off lines alone: the A/B of "off".
Every argument is prepared outside the timed windows and the library is driven through ctypes.  Each call ends in the library's own wait
for the device, so the host clock around a window of calls measures finished work.  Per line: one untimed warm-up window, then `repeats`
timed windows; the median and the range of the windows are reported.  Device time: HIP events on the context's stream
(mpmc_set_profiling), class MPMC_K_PAIR, in a pass of their own; the contact walk's share is the difference between on and off."""
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
E2R = 408.7816  # sqrt(K A) per elementary charge
MODES = (("off", 0, 1), ("sigma + absolute", 3, 1), ("sigma + absolute, contact_skip = 0", 3, 0))


def windows(fn, repeats):
    fn()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return np.array(out)


def line(label, t, per, unit="us"):
    t = 1e6 * t / per
    return f"    {label:<34s}{np.median(t):10.2f} {unit} ({t.min():.2f} .. {t.max():.2f})"


def measure(name, repeats, scale, lines, off_only=False):
    inp, _ = gen_box.materialize(name, tempfile.mkdtemp())
    atoms, basis, opts = pqr.load_case(inp)
    opts = dict(opts, polarization=0, polar_iterative=0)
    n = len(atoms["pos"])
    have = hasattr(energy.lib(), "mpmc_set_cavity_autoreject")
    lines.append(f"{name}: {n} atoms, scale {scale}, {repeats} windows per line (median, min .. max)")
    rng = np.random.default_rng(11)
    B = np.asarray(basis).reshape(3, 3)
    m = 3
    rel = np.array([[0.0, 0.0, 0.0], [0.8164904, 0.5773590, 0.0], [-0.8164904, 0.5773590, 0.0]])
    q = np.ascontiguousarray(np.array([-0.8476, 0.4238, 0.4238]) * E2R)
    al, ep, sg = np.zeros(m), np.array([78.2, 0.0, 0.0]), np.array([3.166, 0.0, 0.0])
    ms = np.array([15.999, 1.008, 1.008])
    fr, hd = np.zeros(m, dtype=np.int32), np.zeros(m, dtype=np.int32)
    args = (dp(q), dp(al), dp(ep), dp(sg), ip(fr), ip(hd), dp(ms))
    P = np.ascontiguousarray(np.stack([rel + rng.uniform(0.0, 1.0, size=3) @ B for _ in range(256)]))
    moves = np.ascontiguousarray(atoms["pos"][:256] + rng.normal(scale=0.1, size=(256, 3)))
    base = {}
    for label, rules, skip in MODES:
        if rules and (not have or off_only):
            continue
        S = energy.System(atoms, basis, opts, max_atoms=n + 64)
        L, h = S._L, S.handle
        if have:
            S.configure("contact_skip", skip)
            S.set_cavity_autoreject(rules, scale if rules else 0.0)
        r = energy.Result()
        out = (energy.Result * 256)()

        def ok(rc):
            if rc != 0:
                raise energy.MpmcError(rc, (L.mpmc_last_error(h) or b"").decode())

        def evaluate(count):
            for _ in range(count):
                ok(L.mpmc_energy(h, C.byref(r)))

        def displace(count):
            for c in range(count):
                ok(L.mpmc_trial_begin(h, c, 1, dp(moves[c])))
                ok(L.mpmc_trial_energy(h, C.byref(r)))
                ok(L.mpmc_trial_reject(h))

        def insert(count):
            for c in range(count):
                ok(L.mpmc_trial_insert_begin(h, n, m, dp(P[c]), *args))
                ok(L.mpmc_trial_energy(h, C.byref(r)))
                ok(L.mpmc_trial_reject(h))

        def batch(count):
            for _ in range(count):
                ok(L.mpmc_insert_candidates(h, m, 256, dp(P), *args, out))

        evaluate(1)
        lines.append(f"  {label}")
        if rules:
            i = S.cavity_autoreject_info()
            total = i["tile_pairs_walked"] + i["tile_pairs_skipped"]
            lines.append(f"    tile pairs walked {i['tile_pairs_walked']} of {total} ({100.0 * i['tile_pairs_walked'] / total:.1f} %), "
                         f"n_replaced {i['n_replaced']}, n_absolute {i['n_absolute']}")
        wall = {"evaluation": windows(lambda: evaluate(50), repeats) / 50, "displacement trial": windows(lambda: displace(256), repeats) / 256,
                "insertion trial": windows(lambda: insert(256), repeats) / 256, "batch of 256 candidates": windows(lambda: batch(20), repeats) / 20}
        S.set_profiling(True)
        dev = {}
        for key, fn, count in (("evaluation", evaluate, 20), ("displacement trial", displace, 64), ("insertion trial", insert, 64),
                               ("batch of 256 candidates", batch, 10)):
            S.timings(reset=True)
            fn(count)
            t = S.timings(reset=True)["pair"]
            dev[key] = (1e3 * t["ms"] / count, t["launches"] / count)
        S.set_profiling(False)
        for key, t in wall.items():
            text = line(key + ", wall", t, 1.0)
            if key in dev:
                text += f"   device (pair class) {dev[key][0]:9.2f} us in {dev[key][1]:.0f} brackets"
            if rules and key in base:
                text += f"   + {1e6 * (np.median(t) - base[key][0]):8.2f} us wall, + {dev[key][0] - base[key][1]:8.2f} us device against off"
            lines.append(text)
            if not rules and key in dev:
                base[key] = (float(np.median(t)), dev[key][0])
        S.close()
    lines.append("")


def main():
    argv = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "cavity_autoreject.txt")
    repeats, scale = 7, 1.0
    off_only = "--off-only" in argv  # (the A/B of "off" against another build: alternate the two libraries in one session)
    if off_only:
        argv.remove("--off-only")
    for flag in ("--out", "--repeats", "--scale"):
        if flag in argv:
            i = argv.index(flag)
            v = argv[i + 1]
            del argv[i:i + 2]
            if flag == "--out":
                out_path = v
            elif flag == "--repeats":
                repeats = int(v)
            else:
                scale = float(v)
    if energy.device_count() < 1:
        raise SystemExit("autoreject_rate.py: no HIP device (nothing here is measured on a CPU)")
    lib_path = os.environ.get("MPMC_ENERGY_LIB") or "the tree's own build"
    lines = [f"device: {energy.device_name(0)}", f"library: {lib_path}",
             "wall: time.perf_counter around windows of calls, each call ending in the library's own wait; every argument prepared outside",
             "device: HIP events on the context's stream under mpmc_set_profiling, class MPMC_K_PAIR, in a pass of their own", ""]
    for name in argv or ["ion10k_es", "lj1000"]:
        measure(name, repeats, scale, lines, off_only)
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
