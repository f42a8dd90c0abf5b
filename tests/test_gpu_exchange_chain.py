"""GPU (MI355X): a long chain of accepted exchange and displacement moves with no full evaluation, across kXchResum.

A grand-canonical run does thousands of accepted insertions and removals and never calls mpmc_energy: the accepted totals and the structure
factors are only ever updated incrementally, the host sums behind lrc_pair, lrc_self and es_self by one molecule per accepted exchange
(lrc_pair from binomial moment products, with cancellation), and after kXchResum accepted exchanges those sums are re-made from the list.
The chain here runs 1100 accepted steps on a heterogeneous box of about 190 atoms around the three-tile edge (test_gpu_size_ladder's
recipe with a frozen framework of 64 sites; Ewald, rd_lrc on), drawn insert / remove / displace so that n stays in [150, 260].  The exchange
trials number kXchResum - 1, kXchResum, kXchResum + 1 (counted from 0: the middle one is the trial that re-sums) and the last step are held
to a fresh context (1e-11), to the oracle (1e-9) and to the oracle's position-independent terms and counts (check_exchange); the final
energy() agrees with the running accepted total at 1e-10.  mpmc_debug_exchange_counts shows that every exchange took the delta path and
that the sums were made exactly twice.

The start list ends in an atom that adds nothing to the host sums (epsilon 0, no charge) and the fourth exchange appends a charged
Lennard-Jones atom that stays the last one: an error in the re-summation of the list's end shows at the checkpoints behind kXchResum and
not in front of it.

Measured on an MI355X (profiles/exchange_chain_drift.txt; -s prints the figures): 1059 exchanges and 41 displacements, n from 189 to 258;
the largest relative deviation of a checkpoint's trial is 1.3e-14 from the fresh context and 5.6e-14 from the oracle (the total, at the
last step), lrc_pair stays within 2.6e-14 of the oracle and does not move across the re-summation, and at the end of the chain the running
total is 9.2e-15 from energy().  These are records, not tolerances: the asserted bounds are the project's 1e-11, 1e-9 and 1e-10."""
import numpy as np
import pytest

import test_gpu_size_ladder as ladder
import util
from mpmcxx_amd import energy
from test_gpu_exchange_ladder import contact, small_insertion
from test_gpu_exchange_moves import check_exchange, inserted, removed

pytestmark = pytest.mark.gpu

molecules = util.molecules
STEPS = 1100
N_START, N_FRAME, SEED = 190, 64, 31
N_BAND = (150, 260)
LOUD_AT_EXCHANGE = 3  # the exchange (counted from 0) that appends the atom which stays the list's last one
OPTS = ladder.options()  # Ewald, rd_lrc on


def chain_box():
    atoms, basis = ladder.ladder_box(N_START, "ortho", SEED, n_frame=N_FRAME)
    atoms["epsilon"][-1] = 0.0  # the last atom of the start list: nothing in the host sums
    atoms["charge"][-1] = 0.0
    return atoms, basis


def loud_atom(atoms, basis):
    """a mobile, charged Lennard-Jones atom: every host sum has a share of it"""
    rng = np.random.default_rng(SEED)
    while True:
        pos = (rng.uniform(-1.0, 2.0, size=3) @ np.asarray(basis).reshape(3, 3))[None, :]
        if contact(atoms, basis, pos) >= 2.6:
            break
    return {"pos": pos, "charge": np.array([0.5 * ladder.E2R]),
            "polarizability": np.array([1.0]), "epsilon": np.array([80.0]), "sigma": np.array([3.2]), "frozen": np.zeros(1, dtype=np.int32),
            "has_disp": np.zeros(1, dtype=np.int32), "mass": np.array([20.0])}


def chain_steps(atoms, basis, steps=STEPS, seed=SEED):
    """The chain, every step accepted: yields (kind, arguments, trial list) with kind "insert" (at, molecule), "remove" (first, count) or
    "move" (first, new positions).  Drawn 4 % displacements, otherwise insertions with a probability that falls from 0.66 at the lower edge
    of N_BAND to 0.50 at the upper one (insertions are the smaller edits: a clear site is easier to find for a small molecule) and forced
    at the edges, so that the walk visits both the three- and the four-tile edge.  Insertions keep test_gpu_exchange_ladder.GAP from
    every resident atom.  Never a copy or a removal of the framework, never an edit of the list's end but the one appended atom, and the
    last step is an exchange.  Pure Python: tests/test_exchange_ladder_boxes.py runs it without a device."""
    rng = np.random.default_rng(seed)
    lo, hi = N_BAND
    exchanges = 0
    for step in range(steps):
        n = len(atoms["pos"])
        small = [mm for mm in molecules(atoms)[:-1] if mm[1] - mm[0] <= 4]
        if exchanges == LOUD_AT_EXCHANGE:
            kind, args = "insert", (n, loud_atom(atoms, basis))
        elif step < steps - 1 and rng.random() < 0.04:
            a, b = small[rng.integers(len(small))]
            kind, args = "move", (a, atoms["pos"][a:b] + rng.normal(scale=0.3, size=(b - a, 3)))
        elif n + 4 > hi or (n - 4 >= lo and rng.random() >= 0.66 - 0.16 * (n - lo) / (hi - lo)):
            a, b = small[rng.integers(len(small))]
            kind, args = "remove", (a, b - a)
        else:
            kind, args = "insert", small_insertion(rng, atoms, basis, at_end=False)
        if kind == "insert":
            trial = inserted(atoms, *args)
        elif kind == "remove":
            trial = removed(atoms, args[0], args[0] + args[1])
        else:
            trial = dict(atoms, pos=atoms["pos"].copy())
            trial["pos"][args[0]:args[0] + len(args[1])] = args[1]
        exchanges += kind != "move"
        yield kind, args, trial
        atoms = trial


COMPONENTS = util.TRIAL_KEYS + ["lrc_pair", "lrc_self", "es_self"]


def deviations(obs, ref):
    return {k: (abs(obs[k] - ref[k]) / abs(ref[k]) if ref[k] else abs(obs[k])) for k in COMPONENTS if k != "polarization_energy"}


def test_chain_of_accepted_moves_across_the_resummation():
    from oracle import OracleSystem

    resum = util.xch_resum()
    checkpoints = {resum - 1: "before the re-summation", resum: "the re-summing trial", resum + 1: "behind the re-summation"}
    atoms, basis = chain_box()
    S = energy.System(atoms, basis, OPTS, max_atoms=512)  # (a growth rebuild would reset the count of accepted exchanges)
    try:
        e_acc = S.energy()
        exchanges = 0
        for step, (kind, args, trial) in enumerate(chain_steps(atoms, basis)):
            if kind == "insert":
                e_trial = S.trial_insert_energy(*args)
            elif kind == "remove":
                e_trial = S.trial_remove_energy(*args)
            else:
                e_trial = S.trial_energy(*args)
            assert not S.last_trial_was_full(), step
            last = step == STEPS - 1
            if kind != "move" and (exchanges in checkpoints or last):
                label = f"step {step}, exchange {exchanges} ({'the last step' if last else checkpoints[exchanges]}), n = {len(trial['pos'])}"
                T = energy.System(trial, basis, OPTS)
                T.energy()
                dev_f, dev_o = deviations(S.trial_observables, T.observables), deviations(S.trial_observables, OracleSystem(trial, basis, OPTS).energy(want_atoms=False))
                T.close()
                print(f"\n{label}\n  vs fresh context: " + ", ".join(f"{k} {v:.1e}" for k, v in dev_f.items()) +
                      "\n  vs oracle:        " + ", ".join(f"{k} {v:.1e}" for k, v in dev_o.items()))
                check_exchange(S, trial, basis, OPTS, label)
                want_resums = 1 if exchanges < resum else 2
                assert util.exchange_counts(S) == (exchanges + 1, 0, want_resums), (label, util.exchange_counts(S))
            S.accept()
            atoms, e_acc = trial, e_trial
            exchanges += kind != "move"
            assert S.n == len(atoms["pos"]) and N_BAND[0] <= S.n <= N_BAND[1], step
        assert exchanges >= resum + 2
        assert util.exchange_counts(S) == (exchanges, 0, 2)  # the delta path throughout; the sums made at the first trial and at kXchResum
        e_final = S.energy()
        print(f"\nend of chain ({STEPS} accepted steps, {exchanges} exchanges): running total {e_acc!r}, energy() {e_final!r}, "
              f"relative drift {abs(e_acc - e_final) / abs(e_final):.2e}")
        assert util.close(e_acc, e_final, 1e-10), (e_acc, e_final)
        ref = OracleSystem(atoms, basis, OPTS).energy()
        util.assert_matches_oracle(S.observables, None, ref, atoms, OPTS, label="end of chain")
    finally:
        S.close()
