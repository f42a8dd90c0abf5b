"""GPU (MI355X): the trial-move kernels that share one scaffold (csrc/trial_kernels.h, the reductions of csrc/device_math.h) give the bits
and the launches of the commit before they were merged.

tests/golden/trial_kernels_parent.json holds, per case, what `record` returns with the PARENT commit's library on an MI355X: every field
of the result as a bit pattern (float.hex(); the counts as integers) and the launches per timing class, for the sequence
    energy();  then per move size m:  trial + reject,  trial + accept,  trial + reject,  energy()
on one live context (a map left marked, or a finish kernel that adds twice, shows in the trial or the evaluation behind it).  Sizes:
1, 8 | 9 (the two sides of the scan / map switch of the Ewald paths), 64 (moved-moved pairs within a tile and across tiles), on the
water box one whole molecule as well (intramolecular moved-moved pairs).  Boxes of four tiles, so the sums over tiles have more than
one term.  Every trial must be a delta (last_trial_was_full() False); the Gauss-Seidel case is an evaluation only (k_palmo_reduce).

To regenerate the golden (a compiler or ROCm change that moves a last bit): build the library of the commit before "One moved-atom scaffold
and one block sum for the trial-move kernels" (python -c "from mpmcxx_amd import build; build.build_library()" in a checkout of it) and run,
in this tree on the GPU,
    MPMC_ENERGY_LIB=/path/to/that/libmpmc_energy.so python tests/test_gpu_trial_parent_bits.py tests/golden/trial_kernels_parent.json
(energy.py loads the library the variable names instead of the tree's own)."""
import functools
import json
import os
import tempfile

import pytest

import disp_expansion_ref as D
import three_body_ref as T
import util
from mpmcxx_amd import energy, gen_box

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(util.GOLDEN, "trial_kernels_parent.json")
SIZES = (1, 8, 9, 64)
FIRSTS = (3, 40, 100)  # first atom of the rejected, the accepted and the second rejected move of a size


@functools.lru_cache(maxsize=None)
def _wolf(name):
    return util.load_generated(name, tempfile.mkdtemp(prefix="trial_parent_bits_"))


def _with(load, name, **extra):
    atoms, basis, opts = load(name)
    return atoms, basis, dict(opts, **extra)


# label -> (box, evaluation only)
CASES = {
    "ion216_polar": (lambda: util.load_fixture("ion216_polar"), False),                                # Ewald field, orthorhombic
    "ion216_polar_noewald": (lambda: _with(util.load_fixture, "ion216_polar", polar_ewald=0), False),  # FIELD 2
    "ion216_triclinic": (lambda: util.load_fixture("ion216_triclinic"), False),                        # skewed cell
    "water64_polar": (lambda: util.load_fixture("water64_polar"), False),                              # intramolecular flags
    "ion216_polar_pw_jac": (lambda: _wolf("ion216_polar_pw_jac"), False),                              # Wolf field, damped
    "ion216_polar_pw0_jac": (lambda: _wolf("ion216_polar_pw0_jac"), False),                            # undamped
    "ion216_triclinic_pw_jac": (lambda: _wolf("ion216_triclinic_pw_jac"), False),                      # skewed cell
    "ion216_at": (lambda: T.load("ion216_at"), False),                                                 # three-body marker and sum
    "ion216_triclinic_at": (lambda: T.load("ion216_triclinic_at"), False),
    "ion216_disp": (lambda: D.load("ion216_disp"), False),                                             # dispersion expansion, undamped
    "ion216_triclinic_disp": (lambda: D.load("ion216_triclinic_disp"), False),                         # damped, skewed cell
    "ion216_polar_disp": (lambda: D.load("ion216_polar_disp"), False),                                 # damped, with the polarizable path
    "ion216_polar_disp_undamped": (lambda: _with(D.load, "ion216_polar_disp", damp_dispersion=0), False),
    "water64_nonpolar": (lambda: _with(util.load_fixture, "water64_polar", polarization=0, polar_iterative=0), False),  # k_intra_terms, k_delta_finish + recip
    "ion216_polar_pw_gsp": (lambda: _wolf("ion216_polar_pw_gsp"), True),                               # k_palmo_reduce
}


def bits(obs):
    return {k: (float(v).hex() if isinstance(v, float) else int(v)) for k, v in obs.items()}


def launches(S):
    return {k: v["launches"] for k, v in S.timings(reset=True).items()}


def record(label):
    box, evaluation_only = CASES[label]
    atoms, basis, opts = box()
    S = energy.System(atoms, basis, opts)
    S.energy()  # (allocations, the position-independent terms: the recorded evaluations are steady-state ones)
    S.set_profiling(True)
    S.timings(reset=True)
    S.energy()
    rec = {"energy": bits(S.observables), "energy_launches": launches(S), "moves": []}
    if not evaluation_only:
        moves = [(m, FIRSTS) for m in SIZES]
        if label.startswith("water64"):
            mols = [a for a, b in util.molecules(atoms) if b - a == 3]
            moves.append((3, (mols[1], mols[13], mols[33])))
        for m, firsts in moves:
            step = {"m": m, "trials": []}
            for n, (first, verdict) in enumerate(zip(firsts, ("reject", "accept", "reject"))):
                S.trial_energy(first, util.moved(atoms, first, m, seed=1000 * m + n))
                assert not S.last_trial_was_full(), (label, m, first)  # a full evaluation in disguise would test nothing
                t = bits(S.trial_observables)
                getattr(S, verdict)()
                step["trials"].append({"first": first, "verdict": verdict, "result": t, "launches": launches(S)})
            S.energy()
            step["energy"] = bits(S.observables)
            step["energy_launches"] = launches(S)
            rec["moves"].append(step)
    S.close()
    return rec


@pytest.mark.parametrize("label", sorted(CASES))
def test_bits_and_launches_of_the_parent(label):
    with open(GOLDEN) as f:
        want = json.load(f)[label]
    got = json.loads(json.dumps(record(label)))
    if got != want:  # name what differs first: the whole record is long
        assert got["energy"] == want["energy"] and got["energy_launches"] == want["energy_launches"], (label, "first evaluation", got["energy"], want["energy"])
        for g, w in zip(got["moves"], want["moves"]):
            for tg, tw in zip(g["trials"], w["trials"]):
                assert tg == tw, (label, "m", g["m"], "first", tg["first"], tg, tw)
            assert g["energy"] == w["energy"] and g["energy_launches"] == w["energy_launches"], (label, "m", g["m"], "evaluation", g["energy"], w["energy"])
    assert got == want, label


if __name__ == "__main__":  # regenerate the golden from the library MPMC_ENERGY_LIB names (see the module docstring)
    import sys

    with open(sys.argv[1], "w") as f:
        json.dump({k: record(k) for k in sorted(CASES)}, f, indent=0, sort_keys=True)
