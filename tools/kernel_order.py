#!/usr/bin/env python3
"""Kernel order per hardware queue of two BUILDS of the library, on the two-stream polarizable box of the size ladder (64 tiles plus one
atom, compact solver: sweep plus generic list, panel table and reciprocal space on the side stream).  Per build:
   cd /tmp && export TMPDIR=/tmp && MPMC_ENERGY_LIB=<.so> rocprofv3 --kernel-trace --output-format csv -d $OUT_<label> -- python3 $ROOT/tools/kernel_order.py
(three evaluations: the one that allocates and two steady-state ones), then
   python3 tools/kernel_order.py --compare parent=$OUT_parent tree=$OUT_tree > profiles/enqueue_stages_kernel_order.txt
prints both lists (queues in the order of their first dispatch, kernels in dispatch order) and whether they are equal: as they stand, without the
runtime's own fill and copy kernels (an allocation is filled, the panel segments uploaded, where that is done), and with them behind the first evaluation; exit status 1 unless the last two hold."""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def queues(trace_dir):
    f = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r.get("Dispatch_Id") or r["Start_Timestamp"]))
    out = {}
    for r in rows:  # (dicts keep insertion order: queues come out by their first dispatch)
        out.setdefault(r["Queue_Id"], []).append(r["Kernel_Name"].replace("mpmc::", "").split("(")[0])
    return list(out.values())


if len(sys.argv) > 1 and sys.argv[1] == "--compare":
    lists = {}
    for spec in sys.argv[2:]:
        label, _, d = spec.partition("=")
        lists[label] = queues(d)
        for q, names in enumerate(lists[label]):
            print(f"== {label}: queue {q}, {len(names)} kernels")
            for k, name in enumerate(names):
                print(f"  {k:4d} {name}")
    (la, a), (lb, b) = lists.items()
    fill = lambda name: name.startswith("__amd_rocclr_")  # the runtime's own kernels behind hipMemsetAsync and hipMemcpyAsync: allocation fills and the segment upload, but clears too

    def steady(qs):  # the queue that posts results from the end of its first evaluation on; the other queues whole
        return [q[q.index("k_post_results") + 1:] if "k_post_results" in q else q for q in qs]

    def verdict(what, x, y):
        same = x == y
        print(f"== {what}: {la} has {[len(q) for q in x]} kernels per queue, {lb} {[len(q) for q in y]}: ordered kernel names per queue " + ("EQUAL" if same else "DIFFER"))
        if not same:
            for q, (u, v) in enumerate(zip(x, y)):
                k = next((i for i, (m, n) in enumerate(zip(u, v)) if m != n), min(len(u), len(v)))
                if k < max(len(u), len(v)):
                    print(f"   queue {q}: first difference at {k}: {u[k:k + 1]} against {v[k:k + 1]}")
        return same

    verdict("every kernel (an allocation's fill and the upload of the panel segments stand where they are made)", a, b)
    ok = verdict("every kernel of ours (the runtime's fill and copy kernels left out)", [[n for n in q if not fill(n)] for q in a], [[n for n in q if not fill(n)] for q in b])
    ok = verdict("every kernel, fills included, behind the first evaluation (which is the one that allocates)", steady(a), steady(b)) and ok
    sys.exit(0 if ok else 1)

import util  # noqa: E402
from mpmcxx_amd import energy  # noqa: E402
from test_gpu_size_ladder import POLAR, box, options  # noqa: E402

n = util.rung_sizes(util.size_ladder()["sweep"][0])[1]
atoms, basis = box(n, "ortho")
S = energy.System(atoms, basis, options(POLAR, solver="compact"))
for _ in range(3):
    S.energy()
print(f"{n} atoms, {S.tile_stats()['tile_pairs']} tile pairs, pair kernel {S.last_pair_kernel()}, tensor store {S.memory_usage()[1]} bytes, "
      f"energy {S.observables['energy']!r}")
S.close()
