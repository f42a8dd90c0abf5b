#!/usr/bin/env python3
"""Rates of exchange trials (mpmc_trial_insert_begin / mpmc_trial_remove_begin) next to displacement trials of a molecule of the same
size and next to what the same moves cost without them (mpmc_set_atoms + mpmc_energy; twice that for a rejected move).
usage: python tools/exchange_bench.py [fixture ...] [--reps N]     (default: ion10k_es lj1000, the boxes of bench.py's configs[2] and [1])
The library is driven through ctypes with every argument prepared outside the timed loops, so that the rates are the library's."""
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


def clock(fn, reps):
    t0 = time.perf_counter()
    for k in range(reps):
        fn(k)
    return (time.perf_counter() - t0) / reps


def measure(name, reps):
    inp, _ = gen_box.materialize(name, tempfile.mkdtemp())
    atoms, basis, opts = pqr.load_case(inp)
    opts = dict(opts, polarization=0, polar_iterative=0)
    ids = atoms["mol_id"]
    m = int(np.argmax(ids != ids[0])) if (ids != ids[0]).any() else len(ids)  # atoms of the first molecule
    n = len(ids)
    S = energy.System(atoms, basis, opts, max_atoms=n + m + 64)
    L, h, r = S._L, S.handle, energy.Result()
    S.energy()
    rng = np.random.default_rng(7)
    f = lambda k: np.ascontiguousarray(atoms[k][:m], dtype=np.float64)
    g = lambda k: np.ascontiguousarray(atoms[k][:m], dtype=np.int32)
    q, al, ep, sg, ms, fr, hd = f("charge"), f("polarizability"), f("epsilon"), f("sigma"), f("mass"), g("frozen"), g("has_disp")
    B = np.asarray(basis).reshape(3, 3)
    centre = atoms["pos"][:m].mean(axis=0)
    # insertion sites: of 20 candidates per trial the ones farthest from every atom (an overlap would put 1e10 K into the totals, and what
    # is left of it after the removal would say nothing about the path)
    Binv = np.linalg.inv(B)
    cand = rng.uniform(0, 1, (20 * reps, 3)) @ B
    gap = np.empty(len(cand))
    for c0 in range(0, len(cand), 256):
        d = (cand[c0:c0 + 256, None, :] - atoms["pos"][None, :, :]) @ Binv
        d -= np.rint(d)
        gap[c0:c0 + 256] = np.sqrt((((d @ B) ** 2).sum(axis=2)).min(axis=1))
    best = np.argsort(gap)[-reps:]
    spots = [np.ascontiguousarray(atoms["pos"][:m] - centre + cand[i]) for i in best]
    moved = [np.ascontiguousarray(atoms["pos"][:m] + rng.normal(scale=0.15, size=(m, 3))) for _ in range(reps)]
    p_spots, p_moved = [dp(a) for a in spots], [dp(a) for a in moved]
    pq, pal, pep, psg, pms, pfr, phd = dp(q), dp(al), dp(ep), dp(sg), dp(ms), ip(fr), ip(hd)
    res = C.byref(r)

    def ok(rc):
        if rc != 0:
            raise energy.MpmcError(rc, (L.mpmc_last_error(h) or b"").decode())

    def insert(k, verdict):
        ok(L.mpmc_trial_insert_begin(h, 0, m, p_spots[k], pq, pal, pep, psg, pfr, phd, pms))
        ok(L.mpmc_trial_energy(h, res))
        ok(verdict(h))

    def remove(k, verdict):
        ok(L.mpmc_trial_remove_begin(h, 0, m))
        ok(L.mpmc_trial_energy(h, res))
        ok(verdict(h))

    def displace(k, verdict):
        ok(L.mpmc_trial_begin(h, 0, m, p_moved[k]))
        ok(L.mpmc_trial_energy(h, res))
        ok(verdict(h))

    for fn in (insert, remove, displace):  # first uses allocate
        fn(0, L.mpmc_trial_reject)
    out = {"box": name, "atoms": n, "molecule": m, "reps": reps, "closest": float(gap[best].min())}
    out["displace_reject"] = clock(lambda k: displace(k, L.mpmc_trial_reject), reps)
    out["displace_accept"] = clock(lambda k: displace(k, L.mpmc_trial_accept), reps)
    out["insert_reject"] = clock(lambda k: insert(k, L.mpmc_trial_reject), reps)
    out["remove_reject"] = clock(lambda k: remove(k, L.mpmc_trial_reject), reps)
    # accepted exchanges in turn, so that the box holds n or n + m atoms: each accepted list is uploaded by the next trial, inside its time
    t_in = t_out = 0.0
    for k in range(reps):
        t0 = time.perf_counter()
        insert(k, L.mpmc_trial_accept)
        t1 = time.perf_counter()
        remove(k, L.mpmc_trial_accept)
        t_out += time.perf_counter() - t1
        t_in += t1 - t0
    out["insert_accept"], out["remove_accept"] = t_in / reps, t_out / reps
    assert not S.last_trial_was_full()
    e_delta = r.energy
    e_full = S.energy()
    out["drift"] = abs(e_delta - e_full) / abs(e_full)
    # the same moves today: the whole list again, and a full evaluation
    big = {k: np.concatenate([np.asarray(atoms[k][:m]), np.asarray(atoms[k])]) for k in atoms}
    big["pos"] = np.concatenate([spots[0], atoms["pos"]])
    big["mol_id"] = np.concatenate([np.full(m, int(ids.max()) + 1, dtype=ids.dtype), ids])
    lists = [big, atoms]
    reps_full = max(10, reps // 10)

    def today(k):
        S.set_atoms(lists[k & 1])
        ok(L.mpmc_energy(h, C.byref(r)))

    today(0), today(1)
    out["set_atoms_energy"] = clock(today, reps_full)
    S.close()
    return out


def main():
    args = sys.argv[1:]
    reps = 1000
    if "--reps" in args:
        i = args.index("--reps")
        reps = int(args[i + 1])
        del args[i:i + 2]
    print(f"device: {energy.device_name(0)}")
    for name in args or ["ion10k_es", "lj1000"]:
        o = measure(name, reps)
        us = lambda k: o[k] * 1e6
        print(f"{o['box']}: {o['atoms']} atoms, molecule of {o['molecule']}, {o['reps']} trials per line, insertion sites at least {o['closest']:.2f} A from every atom")
        for k in ("displace_reject", "displace_accept", "insert_reject", "insert_accept", "remove_reject", "remove_accept"):
            print(f"  {k:18s} {us(k):9.1f} us  {1 / o[k]:10.0f} /s")
        print(f"  set_atoms + energy {us('set_atoms_energy'):9.1f} us  {1 / o['set_atoms_energy']:10.0f} /s   (an accepted exchange today; a rejected one: "
              f"{2 * us('set_atoms_energy'):.1f} us)")
        print(f"  exchange / displacement: insert {o['insert_reject'] / o['displace_reject']:.2f} (reject) {o['insert_accept'] / o['displace_accept']:.2f} (accept), "
              f"remove {o['remove_reject'] / o['displace_reject']:.2f} (reject) {o['remove_accept'] / o['displace_accept']:.2f} (accept); "
              f"totals after {2 * o['reps']} accepted exchanges against a full evaluation: {o['drift']:.1e} relative")


if __name__ == "__main__":
    main()
