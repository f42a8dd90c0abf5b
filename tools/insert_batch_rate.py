#!/usr/bin/env python3
"""Rate of batched insertion candidates (mpmc_insert_candidates) next to the same build's loop of single insertion trials
(mpmc_trial_insert_begin + mpmc_trial_energy + mpmc_trial_reject), on the generated 10 000-atom LJ + Ewald box (ion10k_es, polarization
off) and the 1 000-atom LJ box (lj1000), with a rigid 3-site molecule (one charged Lennard-Jones site, two charged sites without
dispersion).
usage: python tools/insert_batch_rate.py [--out profiles/insert_candidates.txt] [--repeats 7] [box ...]
Every argument is prepared outside the timed windows and the library is driven through ctypes, so that the rates are the library's.  Each
call ends in the library's own wait for the device, so the host clock around a window of calls measures finished work.  Per line: one
untimed warm-up window (the first call of a shape allocates), then `repeats` timed windows of at least 4096 candidates (or 200 calls)
each; the median and the range of the windows are reported.  Kernel times: HIP events on the context's stream (mpmc_set_profiling), in a
pass of their own after the wall-clock windows; the class is MPMC_K_PAIR ("pair") for both paths."""
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
BATCHES = (1, 16, 256, 4096)
E2R = 408.7816  # sqrt(K A) per elementary charge


def rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def windows(fn, repeats):
    fn()  # warm-up: the shape's first call allocates
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return np.array(out)


def measure(name, repeats, lines):
    inp, _ = gen_box.materialize(name, tempfile.mkdtemp())
    atoms, basis, opts = pqr.load_case(inp)
    opts = dict(opts, polarization=0, polar_iterative=0)
    n = len(atoms["pos"])
    S = energy.System(atoms, basis, opts, max_atoms=n + 64)
    L, h = S._L, S.handle
    S.energy()
    rng = np.random.default_rng(11)
    B = np.asarray(basis).reshape(3, 3)
    m = 3
    rel = np.array([[0.0, 0.0, 0.0], [0.8164904, 0.5773590, 0.0], [-0.8164904, 0.5773590, 0.0]])  # a rigid water-like geometry
    q = np.ascontiguousarray(np.array([-0.8476, 0.4238, 0.4238]) * E2R)
    al, ep, sg = np.zeros(m), np.array([78.2, 0.0, 0.0]), np.array([3.166, 0.0, 0.0])
    ms = np.array([15.999, 1.008, 1.008])
    fr, hd = np.zeros(m, dtype=np.int32), np.zeros(m, dtype=np.int32)
    n_max = max(BATCHES)
    P = np.ascontiguousarray(np.stack([rel @ rotation(rng).T + rng.uniform(0.0, 1.0, size=3) @ B for _ in range(n_max)]))
    out = (energy.Result * n_max)()
    r = energy.Result()
    args = (dp(q), dp(al), dp(ep), dp(sg), ip(fr), ip(hd), dp(ms))
    poses = [dp(P[c]) for c in range(n_max)]
    pP = dp(P)

    def ok(rc):
        if rc != 0:
            raise energy.MpmcError(rc, (L.mpmc_last_error(h) or b"").decode())

    def batch(n_cand, calls):
        for _ in range(calls):
            ok(L.mpmc_insert_candidates(h, m, n_cand, pP, *args, out))

    def loop(count):
        for c in range(count):
            ok(L.mpmc_trial_insert_begin(h, n, m, poses[c], *args))
            ok(L.mpmc_trial_energy(h, C.byref(r)))
            ok(L.mpmc_trial_reject(h))

    # the two paths answer the same question: candidate by candidate the same bits
    batch(n_max, 1)
    for c in (0, 1, 255, 256, n_max - 1):
        loop_r = energy.Result()
        ok(L.mpmc_trial_insert_begin(h, n, m, poses[c], *args))
        ok(L.mpmc_trial_energy(h, C.byref(loop_r)))
        ok(L.mpmc_trial_reject(h))
        assert bytes(loop_r) == bytes(out[c]), c
    lines.append(f"{name}: {n} atoms, {S.observables['n_pairs']} pairs, molecule of {m} sites, {repeats} windows per line (median, min .. max)")
    t = windows(lambda: loop(4096), repeats) / 4096
    t_loop = float(np.median(t))
    lines.append(f"  loop of single trials    {1e6 * t_loop:9.2f} us/candidate ({1e6 * t.min():.2f} .. {1e6 * t.max():.2f})  {1 / t_loop:12.0f} candidates/s"
                 f"   256 of them: {256e6 * t_loop:9.1f} us")
    t256 = None
    for n_cand in BATCHES:
        calls = max(1, min(200, 4096 // n_cand))
        t = windows(lambda: batch(n_cand, calls), repeats) / (calls * n_cand)
        med = float(np.median(t))
        lines.append(f"  batch of {n_cand:5d}           {1e6 * med:9.3f} us/candidate ({1e6 * t.min():.3f} .. {1e6 * t.max():.3f})  {1 / med:12.0f} candidates/s"
                     f"   one call: {1e6 * med * n_cand:9.1f} us   loop / batch: {t_loop / med:7.1f}")
        if n_cand == 256:
            t256 = med * 256
    lines.append(f"  a batch of 256 against the loop of 256 single trials it replaces: {1e6 * t256:.1f} us against {256e6 * t_loop:.1f} us "
                 f"({'faster' if t256 < 256 * t_loop else 'NOT faster'}, {256 * t_loop / t256:.1f} x)")
    # device time (HIP events; profiled calls wait through the stream, so these windows are not the wall-clock ones)
    S.set_profiling(True)
    S.timings(reset=True)
    loop(256)
    tl = S.timings(reset=True)["pair"]
    lines.append(f"  device, loop of 256 single trials: {1e3 * tl['ms']:9.1f} us in {tl['launches']} event brackets (k_exchange_all + k_delta_finish each): "
                 f"{1e3 * tl['ms'] / 256:.2f} us/candidate")
    for n_cand in BATCHES:
        calls = 10
        batch(n_cand, calls)
        tb = S.timings(reset=True)["pair"]
        chains = (n_cand + 255) // 256
        lines.append(f"  device, batch of {n_cand:5d}: {1e3 * tb['ms'] / calls:9.1f} us per call ({chains} x (k_insert_batch_all + k_insert_batch_finish)): "
                     f"{1e3 * tb['ms'] / calls / n_cand:.3f} us/candidate")
    S.set_profiling(False)
    calls, cands = S.insert_batch_counts()
    lines.append(f"  (mpmc_debug_insert_batch_counts: {calls} calls, {cands} candidates)")
    lines.append("")
    S.close()


def main():
    argv = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "insert_candidates.txt")
    repeats = 7
    if "--out" in argv:
        i = argv.index("--out")
        out_path = argv[i + 1]
        del argv[i:i + 2]
    if "--repeats" in argv:
        i = argv.index("--repeats")
        repeats = int(argv[i + 1])
        del argv[i:i + 2]
    if energy.device_count() < 1:
        raise SystemExit("insert_batch_rate.py: no HIP device (nothing here is measured on a CPU)")
    lines = [f"device: {energy.device_name(0)}",
             "wall: time.perf_counter around windows of calls, each call ending in the library's own wait; every argument prepared outside",
             "device: HIP events on the context's stream under mpmc_set_profiling, class MPMC_K_PAIR, in a pass of their own", ""]
    for name in argv or ["ion10k_es", "lj1000"]:
        measure(name, repeats, lines)
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
