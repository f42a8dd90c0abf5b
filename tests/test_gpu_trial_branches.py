"""GPU (MI355X): trial moves (mpmc_trial_*, csrc/trial.cpp + csrc/kernels_delta.hip) on every move-size branch, and at the production
box size where the accepted totals come from the fast pair sweep (kernels_pair.hip) and the deltas from pair_terms / k_pair_fused.

Every trial is checked against a stateless evaluation of the trial configuration in a fresh context (1e-11 per component, in-cutoff
counts exact) and against the oracle (1e-9 per component, counts bit-exact, the same number of dipole iterations); the dispatch
(delta or full evaluation) is asserted through last_trial_was_full().

Branches by move size m (MPMC_TRIAL_MAX_ATOMS = 256, kMvInline = 8):
  m <= 8, non-polarizable            the move in the kernel arguments (MvArg), moved atoms found by scanning the list
  m <= 8 with inline_move = 0        the same kernels on the staging block (MvDev): bit-identical results
  m > 8                              the staging block + the slot -> list-index map of k_mark_moved (delta_pairs_tile,
                                     delta_intra_block, k_delta_field)
  m > 64                             several moved atoms per lane (delta_intra_block, delta_recip_k), grids of more than one
                                     block (k_mark_moved, k_delta_field_finish)
  m = 256 / 257                      the largest delta move / the fall-back to a full evaluation, and its two reject paths
  polar, > 8 touched tiles           the store-only pass over every tile pair (touch_n = -1)
The ion1000_polar cases run on the fixture's atoms listed in a seeded random order (scattered_ion1000), so that a move of m consecutive
atoms touches many of the 16 tiles: from m = 65 on, the polarizable cases run the store-only pass over every tile pair."""
import numpy as np
import pytest

import util
from mpmcxx_amd import energy

pytestmark = pytest.mark.gpu

MAX_DELTA = 256  # MPMC_TRIAL_MAX_ATOMS


def fixture(name, polar):
    atoms, basis, opts = util.load_fixture(name)
    return atoms, basis, (opts if polar else util.nonpolar(opts))


def scattered_ion1000(polar):
    """ion1000_polar with its atoms listed in a seeded random order.  The fixture lists its 10 x 10 x 10 lattice plane by plane, and the
    context's spatial sort (slabs in x, strips in y, runs in z) keeps the first three planes in the 6 tiles of one slab: every move of
    the ladders below, up to 256 atoms, would stay inside those 6 of the 16 tiles.  In a random order a run of m atoms meets about
    16 (1 - (15/16)^m) tiles: 6.9 for m = 9, 15.7 for m = 65 -- a polarizable trial then has more than 8 touched tiles (touch_n = -1,
    the store-only pass covers every tile pair).  Every molecule is a single atom, so this is the same physical box relabelled."""
    atoms, basis, opts = fixture("ion1000_polar", polar)
    assert len(util.molecules(atoms)) == len(atoms["pos"])
    perm = np.random.default_rng(1000).permutation(len(atoms["pos"]))
    atoms = {k: (v if k == "mol_id" else np.ascontiguousarray(v[perm])) for k, v in atoms.items()}
    return atoms, basis, opts


def run_ladder_case(atoms, basis, opts, first, m, seed, label, pair_kernel=None, oracle=True):
    """one trial of m atoms from `first`, checked against a fresh context and the oracle; then accepted, and the context's own full
    evaluation of the new state (and, for polarizable boxes, its dipoles) must agree with the fresh one"""
    polar = bool(opts.get("polarization"))
    S = energy.System(atoms, basis, opts)
    try:
        if pair_kernel is not None:
            S.configure("pair_kernel", pair_kernel)
        S.energy()
        if pair_kernel == 2:
            assert S.last_pair_kernel() == "sweep", label
        trial = util.moved(atoms, first, m, seed)
        pos = atoms["pos"].copy()
        pos[first:first + m] = trial
        e_trial = S.trial_energy(first, trial)
        assert S.last_trial_was_full() == (m > MAX_DELTA), (label, S.last_trial_was_full())
        fresh = util.check_trial_against_fresh(S, atoms, basis, opts, pos, label=label)
        if oracle:
            util.check_trial_against_oracle(S.trial_observables, atoms, basis, opts, pos, label=label)
        S.accept()
        if polar:  # the accepted state's E0 / mu / E_ind are the trial solve's
            for got, ref, what in zip(S.dipoles(), fresh, ("mu", "E0", "E_ind")):
                assert util.max_rel(got, ref) < util.REL_TOL, (label, what, util.max_rel(got, ref))
        assert util.close(S.energy(), e_trial, 1e-11), label
    finally:
        S.close()


# ---- 1. move-size ladder ---------------------------------------------------------------------------------------------------------

ION1000_M = [1, 8, 9, 64, 65, 256, 257]


@pytest.mark.parametrize("polar", [False, True], ids=["nonpolar", "polar"])
@pytest.mark.parametrize("m", ION1000_M, ids=[f"m{m}" for m in ION1000_M])
def test_ion1000_ladder(m, polar):
    atoms, basis, opts = scattered_ion1000(polar)
    run_ladder_case(atoms, basis, opts, 3, m, 100 + m, f"ion1000_polar {'polar' if polar else 'nonpolar'} m={m}")


# water64_polar: atoms 0-191 are 64 waters of 3 sites in order; [1, 1 + m) starts inside water 0 and ends inside a later water for
# every m here (9: 1-9, 66: 1-66, 190: 1-190), so the intramolecular erf term meets moved-moved, moved-fixed and fixed-moved pairs
# of partly moved molecules -- with m >= 65 also in the second and third pass of the k += 64 loop
WATER_M = [9, 66, 190]


@pytest.mark.parametrize("polar", [False, True], ids=["nonpolar", "polar"])
@pytest.mark.parametrize("m", WATER_M, ids=[f"m{m}" for m in WATER_M])
def test_water64_partial_molecules(m, polar):
    atoms, basis, opts = fixture("water64_polar", polar)
    ids = atoms["mol_id"]
    assert ids[0] == ids[1] and ids[m] == ids[m + 1] and len(set(ids[1:1 + m].tolist())) > 1  # cut molecules at both ends
    run_ladder_case(atoms, basis, opts, 1, m, 200 + m, f"water64_polar {'polar' if polar else 'nonpolar'} m={m}")


# the EXT delta kernels (Wolf electrostatics, Feynman-Hibbs corrections) through the staging block and the slot map
EXT_CASES = [("ion216_wolf", 5, 9), ("ion216_wolf", 5, 65), ("water64_fh2", 1, 9), ("water64_fh2", 1, 65)]


@pytest.mark.parametrize("name,first,m", EXT_CASES, ids=[f"{n}-nonpolar-m{m}" for n, _, m in EXT_CASES])
def test_ext_device_list(name, first, m):
    atoms, basis, opts = fixture(name, False)
    run_ladder_case(atoms, basis, opts, first, m, 300 + m, f"{name} m={m}")


def test_framework_moves_frozen_molecule():
    """ion216_framework: the 150-site frozen framework (atoms 0-149) moved as a whole -- the ABI allows it, and the oracle of the moved
    positions defines the answer: the frozen-frozen skips of delta_pairs_tile / k_delta_field, the AF_FROZEN split of delta_recip_k"""
    atoms, basis, opts = fixture("ion216_framework", True)
    assert atoms["frozen"][:150].all() and not atoms["frozen"][150:].any() and len(set(atoms["mol_id"][:150].tolist())) == 1
    run_ladder_case(atoms, basis, opts, 0, 150, 400, "ion216_framework polar m=150")


@pytest.mark.parametrize("accept", [False, True], ids=["reject", "accept"])
def test_ion64_inline_move_is_bit_identical_to_device_list(accept):
    """m = 1..8: the move in the kernel arguments and the same move through the staging block run the same loops in the same order"""
    atoms, basis, opts = fixture("ion64_es", False)
    A = energy.System(atoms, basis, opts)
    B = energy.System(atoms, basis, opts)
    try:
        B.configure("inline_move", 0)
        assert A.energy() == B.energy()
        pos = atoms["pos"].copy()
        for m in range(1, 9):
            first = 7 * m
            trial = util.moved(dict(atoms, pos=pos), first, m, 500 + m)
            ea, eb = A.trial_energy(first, trial), B.trial_energy(first, trial)
            assert not A.last_trial_was_full() and not B.last_trial_was_full()
            assert ea == eb and A.trial_observables == B.trial_observables, (m, A.trial_observables, B.trial_observables)
            if accept:
                new = pos.copy()
                new[first:first + m] = trial
                util.check_trial_against_fresh(B, atoms, basis, opts, new, label=f"ion64_es staged m={m}")
                pos = new
                A.accept()
                B.accept()
            else:
                A.reject()
                B.reject()
        assert A.energy() == B.energy()  # the two commit paths left the same positions behind
        util.check_trial_against_oracle(A.observables, atoms, basis, opts, pos, label="ion64_es final")
    finally:
        A.close()
        B.close()


# ---- 2. accept / reject sequences that cross branches --------------------------------------------------------------------------

def test_polar_sequence_crosses_branches():
    """ion1000_polar: a rejected 3-atom delta leaves its tiles dirty; a 65-atom delta (> 8 tiles with the dirty ones: store-only pass over
    every tile pair) is accepted; a rejected 257-atom full trial clears e_real_valid, so the next trial (1 atom) runs in full and is
    accepted; the 9-atom trial after it is a delta again."""
    atoms, basis, opts = scattered_ion1000(True)
    S = energy.System(atoms, basis, opts)
    try:
        e_acc = S.energy()
        pos = atoms["pos"].copy()
        steps = [(10, 3, False, False), (500, 65, True, False), (200, 257, False, True), (700, 1, True, True), (30, 9, True, False)]
        for k, (first, m, accept, full) in enumerate(steps):
            label = f"polar sequence step {k} (m={m})"
            trial = util.moved(dict(atoms, pos=pos), first, m, 600 + k)
            new = pos.copy()
            new[first:first + m] = trial
            e_trial = S.trial_energy(first, trial)
            assert S.last_trial_was_full() == full, label
            fresh = util.check_trial_against_fresh(S, atoms, basis, opts, new, label=label)
            if accept:
                S.accept()
                pos, e_acc = new, e_trial
                for got, ref, what in zip(S.dipoles(), fresh, ("mu", "E0", "E_ind")):
                    assert util.max_rel(got, ref) < util.REL_TOL, (label, what, util.max_rel(got, ref))
            else:
                S.reject()
        ref = util.check_trial_against_oracle(S.observables, atoms, basis, opts, pos, label="polar sequence, accumulated")
        assert util.close(e_acc, ref["energy"], 1e-10)
        assert util.close(S.energy(), ref["energy"])
    finally:
        S.close()


def test_nonpolar_sequence_does_not_drift():
    """ion1000_polar without polarization: 20 trials of m in {1, 9, 65, 256} (two of them 257, rejected), half accepted; the accumulated totals against the
    oracle of the final positions (energy at 1e-10), then a full evaluation"""
    atoms, basis, opts = scattered_ion1000(False)
    rng = np.random.default_rng(7)
    S = energy.System(atoms, basis, opts)
    try:
        e_acc = S.energy()
        pos = atoms["pos"].copy()
        sizes = [int(m) for m in rng.choice([1, 9, 65, 256], size=20)]
        verdicts = rng.permutation([True] * 10 + [False] * 10)
        for k in (4, 13):  # two full evaluations (257 atoms), rejected: the reject path re-bases the structure factors with an extra evaluation
            sizes[k], verdicts[k] = MAX_DELTA + 1, False
        for k, m in enumerate(sizes):
            first = int(rng.integers(0, len(pos) - m + 1))
            trial = pos[first:first + m] + rng.normal(scale=0.3, size=(m, 3))
            new = pos.copy()
            new[first:first + m] = trial
            e_trial = S.trial_energy(first, trial)
            assert S.last_trial_was_full() == (m > MAX_DELTA)
            util.check_trial_against_fresh(S, atoms, basis, opts, new, label=f"nonpolar sequence step {k} (m={m})")
            if verdicts[k]:
                S.accept()
                pos, e_acc = new, e_trial
            else:
                S.reject()
        ref = util.check_trial_against_oracle(S.observables, atoms, basis, opts, pos, label="nonpolar sequence, accumulated")
        assert util.close(e_acc, ref["energy"], 1e-10)
        assert util.close(S.energy(), ref["energy"])
    finally:
        S.close()


# ---- 3. production size: totals from the pair sweep, deltas from pair_terms (+ k_pair_fused store patches) -------------------------
# Oracle calls on 10 000-atom boxes: 3 (ion10k_es) + 2 (ion10k_polar) + 1 (ion8000_triclinic) = 6.

LARGE_CASES = {
    "ion10k_es": [(0, 1, True), (100, 9, False), (5000, 65, True)],
    "ion10k_polar": [(0, 1, True), (200, 9, True)],
    "ion8000_triclinic": [(0, 9, True)],  # non-orthogonal min_image_sq<false> in the deltas, on top of the sweep
}


@pytest.mark.parametrize("name", list(LARGE_CASES))
def test_production_size_trials(name, tmp_path):
    atoms, basis, opts = util.load_generated(name, tmp_path)
    polar = bool(opts.get("polarization"))
    S = energy.System(atoms, basis, opts)
    try:
        S.energy()
        assert S.last_pair_kernel() == "sweep", name
        pos = atoms["pos"].copy()
        for k, (first, m, accept) in enumerate(LARGE_CASES[name]):
            label = f"{name} {'polar' if polar else 'nonpolar'} m={m}"
            trial = util.moved(dict(atoms, pos=pos), first, m, 700 + k)
            new = pos.copy()
            new[first:first + m] = trial
            S.trial_energy(first, trial)
            assert not S.last_trial_was_full(), label
            util.check_trial_against_fresh(S, atoms, basis, opts, new, label=label)
            util.check_trial_against_oracle(S.trial_observables, atoms, basis, opts, new, label=label)
            if accept:
                S.accept()
                pos = new
            else:
                S.reject()
    finally:
        S.close()


# ---- 4. the sweep / delta combination on a small box (pair_kernel = 2 forces k_pair_sweep) --------------------------------------

SWEEP_M = [1, 9, 65, 256]


@pytest.mark.parametrize("polar", [False, True], ids=["nonpolar", "polar"])
@pytest.mark.parametrize("m", SWEEP_M, ids=[f"m{m}" for m in SWEEP_M])
def test_ion1000_ladder_on_sweep(m, polar):
    atoms, basis, opts = scattered_ion1000(polar)
    run_ladder_case(atoms, basis, opts, 3, m, 800 + m, f"ion1000_polar sweep {'polar' if polar else 'nonpolar'} m={m}", pair_kernel=2)
