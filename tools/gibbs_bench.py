#!/usr/bin/env python3
"""Gibbs steps per second of examples/gibbs_nvt.cpp, every move as a device trial (`--trials`) beside the full evaluation of both boxes per
step, on two generated inputs: two boxes of a few thousand charged Lennard-Jones atoms (LJ + Ewald, no polarization), and the same boxes
polarizable (ten Jacobi iterations, Ewald field).  transfer_probability 0.3 as in tests/golden/gibbs_*, volume_probability left to the
reference's default (1 / N_total), so a run is displacements and transfers with the odd volume exchange.

Per input and mode: `--runs` runs of `--steps` steps after one warm-up run; steps/s = steps / the wall time of the step loop alone as the
program measures it (`--time`: reading, context creation and the initial evaluation are outside), median [min .. max]; the spread is
max - min of the full-evaluation mode's runs.  Usage: python tools/gibbs_bench.py [--steps 2000] [--polar-steps 300] [--runs 5] [--out FILE]"""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mpmcxx_amd import build, gen_box  # noqa: E402

BOXES = ((4096, 58.0, 21), (2744, 58.0, 22))  # (atoms, cubic edge / A, seed): a denser and a more dilute box in the same cell (one basis per input file)


def write_case(d, polar, steps):
    for (n, L, seed), tag in zip(BOXES, "AB"):
        gen_box.write_pqr(os.path.join(d, f"box{tag}.pqr"), gen_box.lattice_box(n, L, seed))
    opts = {"job_name": "gibbs_bench", "ensemble": "nvt_gibbs", "temperature": 300.0, "numsteps": steps, "corrtime": 10, "seed": 7,
            "move_factor": 0.05, "rot_factor": 0.05, "transfer_probability": 0.3, "volume_change_factor": 0.25}
    if polar:
        opts.update({"polarization": "on", "polar_damp_type": "exponential", "polar_damp": 2.1304, "polar_iterative": "on", "polar_max_iter": 10,
                     "polar_ewald": "on"})
    path = os.path.join(d, "input.in")
    gen_box.write_input(path, "boxA.pqr", gen_box.cubic(BOXES[0][1]), opts)
    with open(path, "a") as f:
        f.write("pqr_input_B boxB.pqr\n")
    return path


def wall(cmd):
    t0 = time.perf_counter()
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    dt = time.perf_counter() - t0
    assert out.returncode == 0, out.stdout[-300:] + out.stderr[-300:]
    loop = [ln for ln in out.stderr.splitlines() if ln.startswith("step loop:")]
    return (float(loop[-1].split()[2]) if loop else dt), out.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--polar-steps", type=int, default=300)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build.build_library()
    libdir = os.path.join(ROOT, "mpmcxx_amd")
    lines = [f"Gibbs steps per second, gibbs_nvt --trials beside gibbs_nvt; boxes of {BOXES[0][0]} and {BOXES[1][0]} atoms in cubic cells of {BOXES[0][1]} A; {a.runs} runs each",
             ""]
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "gibbs_nvt")
        subprocess.check_call(["g++", "-std=c++14", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "gibbs_nvt.cpp"), "-L", libdir,
                               "-lmpmc_energy", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
        for polar, steps in ((False, a.steps), (True, a.polar_steps)):
            inp = write_case(d, polar, steps)
            rate = {}
            for flags in ((), ("--trials",)):
                wall([exe, inp, str(steps), "--time"] + list(flags))  # (warm-up: code objects, file cache)
                runs = [wall([exe, inp, str(steps), "--time"] + list(flags)) for _ in range(a.runs)]
                rate[flags] = [steps / dt for dt, _ in runs]
                tail = runs[-1][1]
                accepted = tail[tail.find('"accept"'):tail.find('"energy_calls"')].strip().rstrip(",")
                lines.append(f"{'polarizable' if polar else 'LJ + Ewald'}, {steps} steps, {'--trials' if flags else 'full evaluations'}: "
                             f"{statistics.median(rate[flags]):.1f} [{min(rate[flags]):.1f} .. {max(rate[flags]):.1f}] steps/s; {accepted}")
            full, tr = rate[()], rate[("--trials",)]
            spread = (max(full) - min(full)) / statistics.median(full)
            lines += [f"  ratio of medians trials / full evaluations: {statistics.median(tr) / statistics.median(full):.2f}; spread of the full-evaluation runs: {100 * spread:.1f} % of their median", ""]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
