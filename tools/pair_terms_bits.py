#!/usr/bin/env python3
"""Every bit the pair-sum terms (disp-expansion, rd_crystal, the rd model) hand back, as text: for comparing two builds of the library byte
for byte (MPMC_ENERGY_LIB selects the build; tools/ab_libs.sh says where an older build lives).

Printed as float.hex() and integers, one line per call: every field of the result and the term's info block (rd_crystal_info, rd_model_info)
  - for every fixture of the FIXTURES lists of tests/test_gpu_disp_expansion.py, test_gpu_rd_crystal.py and test_gpu_rd_model.py;
  - for every trial move of those files' cases: the trial result, then the result after accept or after reject, alternating;
  - for an 11 648-atom rd_only lattice box (182 tiles, 16 653 tile pairs: more than the 16 384 workgroups of a launch, so the grid stride
    takes a second pass), evaluated once each with disp-expansion, rd_crystal order 1 and DREIDING + Lorentz-Berthelot.

usage: python tools/pair_terms_bits.py > bits.txt        (twice, once per build; cmp the two files)
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from mpmcxx_amd import energy, gen_box  # noqa: E402

import test_gpu_disp_expansion as TD  # noqa: E402
import test_gpu_rd_crystal as TC  # noqa: E402
import test_gpu_rd_model as TM  # noqa: E402
import util  # noqa: E402

FIELDS = [f for f, _ in energy.Result._fields_]
BIG = 11648


def text(v):
    return float(v).hex() if isinstance(v, float) else str(int(v))


def line(label, S, obs, info):
    blk = info(S) if info else {}
    print(label, " ".join(f"{k}={text(obs[k])}" for k in FIELDS), " ".join(f"{k}={text(v)}" for k, v in blk.items()), flush=True)


def fixtures(tag, mod, info):
    for name in mod.FIXTURES:
        atoms, basis, opts = mod.R.load(name) if hasattr(mod, "R") else mod.D.load(name)
        S = energy.System(atoms, basis, opts)
        S.energy()
        line(f"{tag} fixture {name}", S, S.observables, info)
        S.close()


def trial(tag, label, atoms, basis, opts, first, new, keep, info):
    S = energy.System(atoms, basis, opts)
    S.energy()
    S.trial_energy(first, new)
    line(f"{tag} trial {label}", S, S.trial_observables, info)
    S.accept() if keep else S.reject()
    S.energy()
    line(f"{tag} {'accepted' if keep else 'rejected'} {label}", S, S.observables, info)
    S.close()


def trials():
    k = 0
    for name, m in TD.CASES:
        atoms, basis, opts = TD.D.load(name)
        first = 150 if "framework" in name else 0
        trial("disp", f"{name} m={m}", atoms, basis, opts, first, util.moved(atoms, first, m, seed=m), k % 2 == 0, None)
        k += 1
    crystal_cases = [("water64_polar_rc2", c) for c in ("translated", "rotated", "one_atom", "far")] + [("water64_fh2_rc2", "rotated")] + \
        [("ion216_framework_rc2", c) for c in ("one_atom", "mobile_run", "framework_part")]  # (test_trial_move_against_a_fresh_evaluation's)
    for name, case in crystal_cases:
        atoms, basis, opts = TC.R.load(name)
        first, new = TC._trial_cases(name, atoms)[case]
        trial("crystal", f"{name} {case}", atoms, basis, opts, first, new, k % 2 == 0, lambda S: S.rd_crystal_info())
        k += 1
    for name, m in TM.CASES:
        atoms, basis, opts = TM.R.load(name)
        if name.startswith("ion4000"):
            opts = util.nonpolar(opts)
        first = 150 if "framework" in name else 0
        trial("rdm", f"{name} m={m}", atoms, basis, opts, first, util.moved(atoms, first, m, seed=m), k % 2 == 0, lambda S: S.rd_model_info())
        k += 1


def big_boxes():
    L = 90.0
    for tag, opts, info in (("disp", {"rd_only": 1, "disp_expansion": 1, "damp_dispersion": 1}, None),
                            ("crystal", {"rd_only": 1, "rd_lrc": 1, "rd_crystal": 1, "rd_crystal_order": 1}, lambda S: S.rd_crystal_info()),
                            ("rdm", {"rd_only": 1, "rd_lrc": 1, "dreiding": 1}, lambda S: S.rd_model_info())):
        rows = gen_box.lattice_box(BIG, L, 11, charged=False, alpha=0.0)
        rows = gen_box._with_disp(rows) if tag == "disp" else gen_box.rd_model_species(rows) if tag == "rdm" else rows
        n = BIG
        atoms = {"pos": np.array([[r.x, r.y, r.z] for r in rows]), "charge": np.zeros(n), "polarizability": np.zeros(n),
                 "epsilon": np.array([r.eps for r in rows]), "sigma": np.array([r.sigma for r in rows]), "mass": np.full(n, 39.948),
                 "mol_id": np.arange(n, dtype=np.int32), "frozen": np.zeros(n, np.int32), "has_disp": np.zeros(n, np.int32)}
        if tag == "disp":
            atoms.update(has_disp=np.ones(n, np.int32), c6=np.array([r.c6 for r in rows]), c8=np.array([r.c8 for r in rows]),
                         c10=np.array([r.c10 for r in rows]))
        S = energy.System(atoms, np.diag([L] * 3), opts)
        S.energy()
        line(f"{tag} box {BIG}", S, S.observables, info)
        S.close()


if __name__ == "__main__":
    if energy.device_count() < 1:
        sys.exit("pair_terms_bits.py: no HIP device")
    fixtures("disp", TD, None)
    fixtures("crystal", TC, lambda S: S.rd_crystal_info())
    fixtures("rdm", TM, lambda S: S.rd_model_info())
    trials()
    big_boxes()
