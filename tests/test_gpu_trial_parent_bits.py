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
(energy.py loads the library the variable names instead of the tree's own).

The second half of this file does the same for the HOST side of a trial: the bookkeeping of csrc/trial.cpp and csrc/evaluate.cpp -- one
record per configuration's totals (accepted, trial, last evaluation), one state of the open trial, one composition of the totals -- gives
the bits, the launches and the counters of the commit before "One record per configuration's totals; one trial state across list edits".
tests/golden/trial_parent.json holds, per case, what `record_state` returns with that commit's library: after every call of the scripted
sequence of `sequence` every field of the result, mpmc_debug_last_trial_was_full, mpmc_debug_exchange_counts and the info structs of the
terms that are on; and, from a second, profiled run of the same sequence, the launches per timing class of every step.  The sequence and
the term combinations are listed at STATE_CASES.  Every trial asserts the path it was written for (delta or full evaluation, by
last_trial_was_full() and the exchange counters): a step that silently took another path would test nothing.  No oracle runs here.
Box sizes: a displacement takes the full path of a non-polarizable box only with more than MPMC_TRIAL_MAX_ATOMS = 256 atoms, so the
sequences run on the first 261 atoms of ion1000_polar (five tiles, the last with five atoms; three species, ten three-site molecules in
front); one sequence starts from exactly 128 atoms, where the accepted insertion opens a new tile (no step 5 / 6 there); the two growth
cases run on water64_polar with max_atoms = 193, its own size, as the growth tests of the terms do.  To regenerate that golden:
    MPMC_ENERGY_LIB=/path/to/that/libmpmc_energy.so python tests/test_gpu_trial_parent_bits.py tests/golden/trial_parent.json"""
import ctypes
import functools
import json
import os
import re
import tempfile

import numpy as np
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


# ---- the host side: records, trial state, composition of the totals ---------------------------------------------------------------------
STATE_GOLDEN = os.path.join(util.GOLDEN, "trial_parent.json")
TRIAL_MAX = int(re.findall(r"#define MPMC_TRIAL_MAX_ATOMS (\d+)", open(os.path.join(util.ROOT, "include", "mpmc_energy.h")).read())[0])
N_BOX = TRIAL_MAX + 5  # five tiles, the last with five atoms
SPECIES = ((119.8, 3.405), (36.7, 2.958), (10.22, 2.28))  # (epsilon K, sigma A): the mixing rules see three species
DISP_SPECIES = ((3.10, 3.45, 64.3, 1623.0, 49060.0), (2.85, 3.70, 129.6, 4187.0, 155500.0))  # alpha, r0, c6, c8, c10 (gen_box.DISP_SPECIES A, B)
SIGMA, ABSOLUTE = energy.AUTOREJECT_SIGMA, energy.AUTOREJECT_ABSOLUTE
CONTACT = np.array([0.5, 0.4, 0.3])  # an inserted molecule this far (0.71 A) from a resident one: a contact of both rules at scale 0.9


def ion_box(n=N_BOX, polar=False, frozen=False, **extra):
    """the first n atoms of ion1000_polar: three species, atoms 0..29 as ten three-site molecules, optionally the last twenty frozen"""
    atoms, basis, opts = util.load_fixture("ion1000_polar")
    atoms = {k: np.array(v[:n]) for k, v in atoms.items()}
    i = np.arange(n)
    atoms["epsilon"] = np.array([SPECIES[k % 3][0] for k in i])
    atoms["sigma"] = np.array([SPECIES[k % 3][1] for k in i])
    atoms["mol_id"] = np.where(i < 30, i // 3, i - 20).astype(np.int32)
    if frozen:
        atoms["frozen"][-20:] = 1
    return atoms, basis, dict(opts if polar else util.nonpolar(opts), **extra)


def at_box():
    atoms, basis, opts = ion_box(axilrod_teller=1)
    atoms["c9"] = np.full(N_BOX, 518.3)
    return atoms, basis, opts


def disp_box():
    atoms, basis, opts = ion_box(disp_expansion=1)
    sp = np.array([DISP_SPECIES[k % 2] for k in range(N_BOX)])
    atoms["epsilon"], atoms["sigma"], atoms["c6"], atoms["c8"], atoms["c10"] = sp.T.copy()
    atoms["has_disp"] = np.ones(N_BOX, dtype=np.int32)
    return atoms, basis, opts


def water_box(**extra):
    atoms, basis, opts = util.load_fixture("water64_polar")
    return {k: np.array(v) for k, v in atoms.items()}, basis, dict(util.nonpolar(opts), **extra)


# label -> (box, what the context is told behind its creation, the steps that do not apply).  Every case runs `sequence`:
#  1 energy()   2 a displacement, rejected   3 a displacement, accepted   4 a no-op displacement, accepted
#  5 a displacement of more than MPMC_TRIAL_MAX_ATOMS atoms (full path), rejected   6 the same, accepted
#  7 an insertion, rejected   8 accepted   9 a removal, rejected   10 accepted
#  11 a trial begun, enqueued with mpmc_trial_energy_async and rejected without a wait
#  12 (rd_only) a position update, then lj(), whose mask is full_mask: it re-bases, and the trial behind it stands on its totals
#  13 (delta-path exchanges) insert_candidates with four poses, then the single trial of one of them
#  14 energy(): the running accepted total, to the bits the parent gives
STATE_CASES = {
    "plain": dict(box=ion_box),
    "plain_128": dict(box=lambda: ion_box(128), small=True),  # (the accepted insertion opens the third tile)
    "rd_only": dict(box=lambda: ion_box(rd_only=1), rd_only=True),
    "polar_full": dict(box=lambda: ion_box(polar=True), polar=True, configure={"polar_delta": 0}),
    "polar_delta": dict(box=lambda: ion_box(polar=True), polar=True, polar_delta=True),
    "rd_crystal": dict(box=lambda: ion_box(rd_crystal=1, rd_crystal_order=2), xch_full=True, info=("rd_crystal_info",)),
    "rd_model_lj_waldmanhagler": dict(box=lambda: ion_box(waldmanhagler=1), xch_full=True, info=("rd_model_info",)),
    "rd_model_14_7": dict(box=lambda: ion_box(lj_buffered_14_7=1), xch_full=True, info=("rd_model_info",)),
    "axilrod_teller": dict(box=at_box, exchange=False),
    "disp_expansion": dict(box=disp_box, exchange=False),
    "autoreject_sigma": dict(box=ion_box, autoreject=(SIGMA, 0.9)),
    # (a frozen species goes in, beside a movable molecule: the unmeasured frozen pairs of the trial composition differ from the list's)
    "autoreject_absolute": dict(box=lambda: ion_box(frozen=True), autoreject=(ABSOLUTE, 0.9), species=-1),
    "autoreject_both": dict(box=lambda: ion_box(frozen=True), autoreject=(SIGMA | ABSOLUTE, 0.9), species=-1),
    "autoreject_sigma_disp": dict(box=disp_box, exchange=False, autoreject=(SIGMA, 0.9)),
}


class Run:
    """one context walking a script: after every step either the state the library shows, or (profiled) the launches of the step"""

    def __init__(self, case, profiled, max_atoms=None):
        self.case, self.profiled = case, profiled
        atoms, self.basis, self.opts = case["box"]()
        self.S = S = energy.System(atoms, self.basis, self.opts, max_atoms=max_atoms)
        for k, v in case.get("configure", {}).items():
            S.configure(k, v)
        if case.get("autoreject"):
            S.set_cavity_autoreject(*case["autoreject"])
        self.steps = []
        self.e_real = False  # polarizable boxes: the resident real-space field is the accepted configuration's (what the polar delta needs)
        S.energy()  # (allocations, the position-independent terms: the recorded calls are steady-state ones)
        if profiled:
            S.set_profiling(True)
            S.timings(reset=True)

    def note(self, step, obs, **extra):
        S = self.S
        if self.profiled:
            self.steps.append({"step": step, "launches": launches(S)})
            return
        rec = {"step": step, "result": bits(obs), "last_trial_was_full": int(S._L.mpmc_debug_last_trial_was_full(S.handle)),
               "exchange_counts": list(util.exchange_counts(S))}
        for name in self.case.get("info", ()) + (("cavity_autoreject_info",) if self.case.get("autoreject") else ()):
            rec[name] = bits(getattr(S, name)())
        rec.update(extra)
        self.steps.append(rec)

    def energy(self, step):
        self.S.energy()
        self.e_real = True
        self.note(step, self.S.observables)

    def molecule(self, k):
        return util.molecules(self.S.atoms)[k]

    def expect(self, step, full, exchange=False):
        """the path of the trial just evaluated: by last_trial_was_full() and, for an exchange, by the counter that moved"""
        S = self.S
        assert S.last_trial_was_full() == full, (step, "full evaluation" if full else "delta", "expected")
        if exchange:
            now = util.exchange_counts(S)
            assert (now[0] - self.xch[0], now[1] - self.xch[1]) == ((0, 1) if full else (1, 0)), (step, self.xch, now)
        if full:
            self.e_real = True

    def move_is_full(self, m):
        c = self.case
        return m > TRIAL_MAX or (bool(c.get("polar")) and not (c.get("polar_delta") and self.e_real))

    def displace(self, step, first, m, verdict, seed, noop=False):
        S = self.S
        pos = S.atoms["pos"][first:first + m].copy() if noop else util.moved(S.atoms, first, m, seed=seed)
        full = self.move_is_full(m)
        S.trial_energy(first, pos)
        if not noop:  # (a no-op enqueues nothing and leaves the diagnostic of the trial before it)
            self.expect(step, full)
        getattr(S, verdict)()
        if full and verdict == "reject" and not noop:
            self.e_real = False
        self.note(step, S.trial_observables)

    def exchange(self, step, verdict, insert=None, remove=None):
        S, c = self.S, self.case
        self.xch = util.exchange_counts(S)
        if insert is not None:
            S.trial_insert_energy(S.n, insert)
        else:
            S.trial_remove_energy(*remove)
        full = bool(c.get("polar") or c.get("xch_full"))
        self.expect(step, full, exchange=True)
        getattr(S, verdict)()
        if full and verdict == "reject":
            self.e_real = False
        self.note(step, S.trial_observables)

    def species(self, k, offset, beside=None):
        """a copy of molecule k, `offset` away from where it stands (or from where molecule `beside` stands)"""
        a, b = self.molecule(k)
        mol = {key: np.array(v[a:b]) for key, v in self.S.atoms.items()}
        if beside is not None:
            mol["pos"] = mol["pos"] - mol["pos"][0] + self.S.atoms["pos"][self.molecule(beside)[0]]
        mol["pos"] = mol["pos"] + offset
        return mol

    def close(self):
        self.S.close()
        return self.steps


def sequence(case, profiled):
    R = Run(case, profiled)
    S = R.S
    try:
        R.energy("1 energy")
        R.displace("2 displacement rejected", *R.molecule(2)[:1], 3, "reject", seed=11)
        R.displace("3 displacement accepted", 40, 2, "accept", seed=12)
        R.displace("4 no-op accepted", 50, 4, "accept", seed=0, noop=True)
        if not case.get("small"):
            R.displace("5 full displacement rejected", 2, TRIAL_MAX + 1, "reject", seed=13)
            R.displace("6 full displacement accepted", 2, TRIAL_MAX + 1, "accept", seed=13)
        if case.get("exchange", True):
            R.exchange("7 insertion rejected", "reject", insert=R.species(case.get("species", 1), CONTACT, beside=1))
            R.exchange("8 insertion accepted", "accept", insert=R.species(case.get("species", 1), CONTACT, beside=1))
            a, b = R.molecule(4)
            R.exchange("9 removal rejected", "reject", remove=(a, b - a))
            R.exchange("10 removal accepted", "accept", remove=(a, b - a))
        # 11: enqueued, never waited for: the rejection drains it
        first, m = 60, 2
        new = np.ascontiguousarray(util.moved(S.atoms, first, m, seed=14)).reshape(-1)
        full = R.move_is_full(m)
        S._check(S._L.mpmc_trial_begin(S.handle, first, m, energy._dp(new)))
        fn = S._L.mpmc_trial_energy_async
        fn.argtypes, fn.restype = [ctypes.c_void_p], ctypes.c_int
        S._check(fn(S.handle))
        S.reject()
        R.expect("11", full)
        R.e_real = R.e_real and not full
        R.note("11 enqueued and rejected without a wait", S.observables)
        if case.get("rd_only"):
            S.update_positions(70, util.moved(S.atoms, 70, 2, seed=15))  # (the accepted totals are gone: only a re-basing call brings them back)
            lj = S.lj()
            R.displace("12 trial behind lj()", 80, 1, "reject", seed=16)
            if not profiled:
                R.steps[-1]["lj"] = float(lj).hex()
        if case.get("exchange", True) and not case.get("polar") and not case.get("xch_full"):
            sp = R.species(3, 0.0)
            poses = np.stack([sp["pos"] + d for d in (CONTACT, 2.0 * CONTACT, np.array([1.9, 1.9, 1.9]), np.array([-2.1, 1.7, 2.0]))])
            before = util.exchange_counts(S)
            out = S.insert_candidates(sp, poses)
            assert util.exchange_counts(S) == before and len(out) == 4  # (no trial was opened for the batch)
            extra = {"candidates": [bits(r) for r in out]}
            if case.get("autoreject"):
                extra["candidate_contacts"] = [[int(v) for v in col] for col in S.insert_candidates_contacts(4)]
            R.note("13 insert_candidates", S.observables, **extra)
            R.exchange("13 single trial behind the batch", "reject", insert=dict(sp, pos=poses[1]))
            if not profiled:
                assert R.steps[-1]["result"] == R.steps[-2]["candidates"][1]
        R.energy("14 energy")
        if not profiled and case.get("autoreject") and case.get("exchange", True):  # (the counts took part: the contact pose was counted)
            seen = [s["cavity_autoreject_info"] for s in R.steps]
            assert any(i["n_replaced"] > 0 or i["n_absolute"] > 0 for i in seen), seen
    finally:
        steps = R.close()
    return steps


def growth(case, verdict, profiled):
    """water64_polar in a context of exactly its size: the insertion outgrows it"""
    R = Run(case, profiled, max_atoms=193)
    S = R.S
    try:
        assert S.n == 193
        R.energy("energy")
        sp = R.species(5, np.array([0.9, -0.6, 0.5]))
        R.exchange("insertion " + verdict, verdict, insert=sp)
        assert S.n == (196 if verdict == "accept" else 193)
        R.displace("displacement behind it", *R.molecule(7)[:1], 3, "reject", seed=21)
        R.displace("no-op behind it", 0, 3, "accept", seed=0, noop=True)
        R.energy("energy behind it")
    finally:
        steps = R.close()
    return steps


for _label, _case in list(STATE_CASES.items()):
    STATE_CASES[_label] = functools.partial(sequence, _case)
# xch_accept_delta's growth branch, with the contact counts on; xch_replace_list across grow_capacity, rejected (the list goes back into the
# grown context) and accepted
STATE_CASES["growth_delta_autoreject"] = functools.partial(growth, dict(box=water_box, autoreject=(SIGMA | ABSOLUTE, 0.9)), "accept")
_crystal = dict(box=lambda: water_box(rd_crystal=1, rd_crystal_order=2), xch_full=True, info=("rd_crystal_info",))
STATE_CASES["growth_full_rd_crystal_rejected"] = functools.partial(growth, _crystal, "reject")
STATE_CASES["growth_full_rd_crystal_accepted"] = functools.partial(growth, _crystal, "accept")


def record_state(label):
    run = STATE_CASES[label]
    return json.loads(json.dumps({"steps": run(False), "launches": run(True)}))


@pytest.mark.parametrize("label", sorted(STATE_CASES))
def test_trial_state_bits_launches_and_counters_of_the_parent(label):
    with open(STATE_GOLDEN) as f:
        want = json.load(f)[label]
    got = record_state(label)
    for key in ("steps", "launches"):  # (name what differs first: the whole record is long)
        assert [s["step"] for s in got[key]] == [s["step"] for s in want[key]], (label, key)
        for g, w in zip(got[key], want[key]):
            for k in sorted(set(g) | set(w)):
                assert g.get(k) == w.get(k), (label, key, g["step"], k, g.get(k), w.get(k))
    assert got == want, label


if __name__ == "__main__":  # regenerate a golden from the library MPMC_ENERGY_LIB names (see the module docstring): the one the file name says
    import sys

    which = {os.path.basename(GOLDEN): (CASES, record), os.path.basename(STATE_GOLDEN): (STATE_CASES, record_state)}
    cases, rec = which[os.path.basename(sys.argv[1])]
    with open(sys.argv[1], "w") as f:
        json.dump({k: rec(k) for k in sorted(cases)}, f, indent=0, sort_keys=True)
