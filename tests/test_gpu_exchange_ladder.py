"""GPU (MI355X): exchange trials on one LIVE context across the launch-path switches of enqueue(), across the re-sort inside a chain, and
of the 320-site framework molecule (the full path of a non-polarizable box).

test_gpu_size_ladder holds both sides of every switch of util.size_ladder() to the oracle with a freshly built context each; here an
accepted insertion takes a context from 64 nt to 64 nt + 3 atoms (splice_atoms re-sizes the tile tables, the accepted totals and structure
factors are kept), the next trials run the other launch path on that state, and removals take it back.  Rungs: single_launch, side_stream,
sweep and pair_waves.  The ksplit_* rungs steer the reciprocal FIELD kernel, which a non-polarizable box never runs (and a polarizable box
has no exchange delta), so they are left out.

Every exchange trial is held to a fresh context on the trial list (1e-11 per component, every count exact, the position-independent terms
at util.REL_TOL); the crossing insertion, the crossing removal and the full evaluations are held to the oracle as well (1e-9, counts
bit-exact) -- at pair_waves the crossing insertion and the final state only.  The start boxes are test_gpu_size_ladder.ladder_box's
(tests/test_exchange_ladder_boxes.py shows that no compared component of them is ill-conditioned).  Which path a trial took is read from
mpmc_debug_exchange_counts / last_trial_was_full(), which kernel an evaluation ran from last_pair_kernel()."""
import time

import numpy as np
import pytest

import test_gpu_size_ladder as ladder
import util
from mpmcxx_amd import energy
from test_gpu_exchange_moves import STATIC_COUNTS, check_exchange, count_N, inserted, random_insertion, removed

pytestmark = pytest.mark.gpu

molecules = util.molecules
options = ladder.options
E2R = ladder.E2R
LADDER = util.size_ladder()
TILE = util.ladder_constants()["kTile"]
SWEEP_MIN_PAIRS = util.ladder_constants()["kSweepMinPairs"]
FH2 = dict(feynman_hibbs=1, feynman_hibbs_order=2, temperature=77.0)  # as the fixture water64_fh2 sets it
# rung -> (cell, options, seed, the mixing site of the inserted molecule): every rung differs from its neighbours in cell and terms
RUNGS = {
    "single_launch": ("cubic", options(rd_only=1), 11, "neg_sigma"),     # the one-launch LJ evaluation is an rd_only box's
    "side_stream": ("triclinic", options(FH2), 12, "has_disp"),         # Ewald (the side stream carries the reciprocal work) + Feynman-Hibbs
    "sweep": ("ortho", options(), 13, "neg_sigma"),                      # plain Ewald: the domain of the pair sweep
    "pair_waves": ("cubic", options(wolf=1), 14, "has_disp"),            # Wolf: k_pair_fused at every size, one wave per tile pair above
}
FRAMEWORK_BOX = (640, "ortho", 21)   # ten tiles, half of them the frozen framework molecule
RESORT_BOX = (512, "triclinic", 22)  # eight full tiles


def start_box(rung):
    cell, opts, seed, _ = RUNGS[rung]
    atoms, basis = ladder.ladder_box(TILE * LADDER[rung][0], cell, seed)
    return atoms, basis, opts


def hetero_molecule(basis, frac, mixing):
    """three sites around the fractional position `frac` (outside [0, 1): the image is wrapped): a charged Lennard-Jones site, a charged
    site that changes lj_mix (sigma < 0, or dispersion coefficients) and a site of epsilon 0 and no charge"""
    centre = np.asarray(frac, dtype=np.float64) @ np.asarray(basis).reshape(3, 3)
    rel = np.array([[0.0, 0.0, 0.0], [0.9, 0.3, -0.2], [-0.4, 0.8, 0.5]])
    return {"pos": centre + rel, "charge": np.array([0.45, -0.45, 0.0]) * E2R, "polarizability": np.array([1.0, 0.0, 0.5]),
            "epsilon": np.array([60.0, 35.0, 0.0]), "sigma": np.array([3.1, -2.7 if mixing == "neg_sigma" else 2.7, 2.4]),
            "frozen": np.zeros(3, dtype=np.int32), "has_disp": np.array([0, 1 if mixing == "has_disp" else 0, 0], dtype=np.int32),
            "mass": np.array([16.0, 12.0, 1.0])}


def fresh_observables(atoms, basis, opts):
    T = energy.System(atoms, basis, opts)
    try:
        T.energy()
        return dict(T.observables)
    finally:
        T.close()


def check_exchange_fresh(S, trial_atoms, basis, opts, label, full=False):
    """the open exchange trial of S against a fresh context on `trial_atoms` alone: the energy components at 1e-11, every count exactly,
    the position-independent terms at util.REL_TOL (the bound check_exchange holds them to against the oracle)"""
    assert S.last_trial_was_full() == full, label
    obs = S.trial_observables
    ref = fresh_observables(trial_atoms, basis, opts)
    bad = util.component_errors(obs, ref, util.TRIAL_KEYS, 1e-11)
    assert not bad, f"{label}: trial vs fresh context (rel 1e-11): " + "; ".join(bad)
    for k in STATIC_COUNTS + ["n_lj_in_cutoff", "n_es_in_cutoff"]:
        assert obs[k] == ref[k], (label, k, obs[k], ref[k])
    bad = util.component_errors(obs, ref, ["lrc_pair", "lrc_self", "es_self"], util.REL_TOL)
    assert not bad, f"{label}: position-independent terms vs fresh context: " + "; ".join(bad)
    assert obs["N"] == count_N(trial_atoms) == ref["N"], (label, obs["N"], ref["N"])
    assert obs["NU"] == obs["N"] * obs["energy"], label
    return ref


def displacement(S, atoms, basis, opts, a, b, seed, label, delta=True):
    """one displacement trial of atoms [a, b) against a fresh context (1e-11, counts exact); returns the trial list, the trial stays open"""
    trial = dict(atoms, pos=atoms["pos"].copy())
    trial["pos"][a:b] = util.moved(atoms, a, b - a, seed)
    S.trial_energy(a, trial["pos"][a:b])
    assert S.last_trial_was_full() == (not delta), label
    util.check_trial_against_fresh(S, trial, basis, opts, trial["pos"], rel=1e-11, label=label)
    return trial


def silent_site(atoms, a, b):
    return bool(np.any((atoms["epsilon"][a:b] == 0.0) | (atoms["charge"][a:b] == 0.0)))


def pick(atoms, size, skip=0):
    """a mobile molecule of `size` sites with a site of epsilon 0 or charge 0 (the classes the position-independent counts tell apart)"""
    found = [(a, b) for a, b in molecules(atoms) if b - a == size and not atoms["frozen"][b - 1] and silent_site(atoms, a, b)]
    return found[skip % len(found)]


def contact(atoms, basis, pos):
    """the smallest distance of the points `pos` from an atom of the list, over the images of the nearest cell"""
    B = np.asarray(basis, dtype=np.float64).reshape(3, 3)
    f = (np.asarray(pos)[:, None, :] - atoms["pos"][None, :, :]) @ np.linalg.inv(B)
    d = (f - np.round(f)) @ B
    return float(np.sqrt((d * d).sum(axis=-1)).min())


GAP = 2.2  # Angstrom


def small_insertion(rng, atoms, basis, at_end=True):
    """random_insertion of a molecule of at most four sites (never a copy of the framework) that comes no closer than GAP to a resident
    atom: one r^-12 contact would be the whole energy, and the relative comparisons would then hold everything else to nothing"""
    while True:
        at, mol = random_insertion(rng, atoms, basis)
        if len(mol["pos"]) <= 4 and (at_end or at != len(atoms["pos"])) and contact(atoms, basis, mol["pos"]) >= GAP:
            return at, mol


def wrapped_clear_site(atoms, basis, seed):
    """a fractional position outside [0, 1) in every coordinate around which hetero_molecule keeps GAP from every resident atom"""
    rng = np.random.default_rng(seed)
    while True:
        frac = rng.uniform(0.05, 0.95, size=3) + rng.choice([-1.0, 1.0], size=3)
        if contact(atoms, basis, hetero_molecule(basis, frac, "neg_sigma")["pos"]) >= GAP + 0.4:
            return frac


def tile_pairs(nt):
    return nt * (nt + 1) // 2


@pytest.mark.parametrize("rung", list(RUNGS))
def test_exchange_across_a_launch_path_switch(rung):
    t0 = time.perf_counter()
    nt = LADDER[rung][0]
    n0 = TILE * nt
    atoms, basis, opts = start_box(rung)
    mixing = RUNGS[rung][3]
    oracle_everywhere = rung != "pair_waves"  # (8 128 atoms: the oracle sees the crossing insertion and the final state)
    in_sweep_domain = not (opts["rd_only"] or opts["wolf"] or opts["feynman_hibbs"])
    S = energy.System(atoms, basis, opts, max_atoms=n0 + 2 * TILE)  # no growth rebuild
    try:
        S.energy()
        assert S.tile_stats()["tile_pairs"] == tile_pairs(nt), rung
        if rung == "sweep":
            assert tile_pairs(nt) <= SWEEP_MIN_PAIRS < tile_pairs(nt + 1) and S.last_pair_kernel() != "sweep", rung
        counts = util.exchange_counts(S)
        assert counts == (0, 0, 0)

        # ---- the crossing insertion: nt + 1 tiles, the new molecule alone in the last one
        mol = hetero_molecule(basis, wrapped_clear_site(atoms, basis, RUNGS[rung][2]), mixing)
        at = molecules(atoms)[len(molecules(atoms)) // 3][0]
        trial = inserted(atoms, at, mol)
        S.trial_insert_energy(at, mol)
        check_exchange(S, trial, basis, opts, f"{rung}: crossing insertion")
        assert util.exchange_counts(S) == (1, 0, 1), rung  # the delta path, the host sums made once
        S.accept()
        atoms = trial
        assert S.n == n0 + 3 and -(-S.n // TILE) == nt + 1
        # ---- with no energy() in between: the inserted molecule (it lives in the last, spatially misplaced tile), then one elsewhere
        displacement(S, atoms, basis, opts, at, at + 3, 1, f"{rung}: displacement of the inserted molecule")
        S.reject()
        a, b = pick(atoms, 2, skip=5)
        atoms = displacement(S, atoms, basis, opts, a, b, 2, f"{rung}: displacement elsewhere")
        S.accept()
        # ---- the other launch path on the carried state
        S.energy()
        assert S.tile_stats()["tile_pairs"] == tile_pairs(nt + 1), rung
        if oracle_everywhere:
            util.assert_matches_oracle(S.observables, None, util.oracle_energy(atoms, basis, opts), atoms, opts, label=f"{rung}: {nt + 1} tiles")
        else:
            ref = fresh_observables(atoms, basis, opts)
            bad = util.component_errors(S.observables, ref, util.TRIAL_KEYS, 1e-11)
            assert not bad, (rung, bad)
            assert all(S.observables[k] == ref[k] for k in util.COUNT_KEYS), rung
        if tile_pairs(nt + 1) > SWEEP_MIN_PAIRS:
            assert S.last_pair_kernel() == ("sweep" if in_sweep_domain else "fused"), (rung, S.last_pair_kernel())
            if rung == "sweep":
                assert S.last_pair_kernel() == "sweep"  # the crossing is not vacuous

        # ---- back: removals until the box has nt tiles again; the last one crosses
        a, b = pick(atoms, 2, skip=1)
        trial = removed(atoms, a, b)
        S.trial_remove_energy(a, b - a)
        check_exchange_fresh(S, trial, basis, opts, f"{rung}: removal before the crossing")
        S.accept()
        atoms = trial
        assert S.n == n0 + 1
        a, b = pick(atoms, 3, skip=2)
        trial = removed(atoms, a, b)
        S.trial_remove_energy(a, b - a)
        if oracle_everywhere:
            check_exchange(S, trial, basis, opts, f"{rung}: crossing removal")
        check_exchange_fresh(S, trial, basis, opts, f"{rung}: crossing removal")
        S.accept()
        atoms = trial
        assert S.n == n0 - 2 and -(-S.n // TILE) == nt
        assert util.exchange_counts(S) == (3, 0, 1), rung
        a, b = pick(atoms, 4, skip=3)
        displacement(S, atoms, basis, opts, a, b, 3, f"{rung}: displacement after the crossing removal")
        S.reject()
        S.energy()
        assert S.tile_stats()["tile_pairs"] == tile_pairs(nt), rung
        if rung == "sweep":
            assert S.last_pair_kernel() != "sweep"
        util.assert_matches_oracle(S.observables, None, util.oracle_energy(atoms, basis, opts), atoms, opts, label=f"{rung}: {nt} tiles again")
    finally:
        S.close()
    print(f"\n{rung}: {time.perf_counter() - t0:.1f} s")


def test_framework_molecule_out_and_in_again():
    """The 320 sites of the frozen framework are more than MPMC_TRIAL_MAX_ATOMS: the full path of a non-polarizable Ewald box, with its
    re-base behind a reject"""
    n, cell, seed = FRAMEWORK_BOX
    atoms, basis = ladder.ladder_box(n, cell, seed)
    opts = options()
    fa, fb = next((a, b) for a, b in molecules(atoms) if b - a == ladder.N_FRAME)
    frame = {k: np.array(v[fa:fb]) for k, v in atoms.items()}
    S = energy.System(atoms, basis, opts, max_atoms=n)
    try:
        S.energy()
        accepted = dict(S.observables)
        without = removed(atoms, fa, fb)
        S.trial_remove_energy(fa, fb - fa)
        check_exchange(S, without, basis, opts, "framework out", full=True)
        assert util.exchange_counts(S) == (0, 1, 0)
        assert S.trial_observables["N"] == accepted["N"] and 0 <= S.trial_observables["n_frozen"] < accepted["n_frozen"]
        S.reject()
        assert S.n == n
        a, b = pick(atoms, 3)
        displacement(S, atoms, basis, opts, a, b, 4, "displacement straight after the rejected removal")
        S.reject()
        S.trial_remove_energy(fa, fb - fa)
        check_exchange_fresh(S, without, basis, opts, "framework out again", full=True)
        S.accept()
        atoms = without
        assert S.n == n - ladder.N_FRAME
        at = molecules(atoms)[7][0]
        assert at != fa
        back = inserted(atoms, at, frame)
        S.trial_insert_energy(at, frame)
        check_exchange_fresh(S, back, basis, opts, "framework in at another boundary", full=True)
        assert util.exchange_counts(S) == (0, 3, 0)
        S.accept()
        atoms = back
        a, b = pick(atoms, 2)
        displacement(S, atoms, basis, opts, a, b, 5, "displacement straight after the accepted insertion")
        S.reject()
        S.energy()
        util.assert_matches_oracle(S.observables, None, util.oracle_energy(atoms, basis, opts), atoms, opts, label="framework in again")
        assert S.observables["n_frozen"] == accepted["n_frozen"] and S.observables["N"] == accepted["N"]
    finally:
        S.close()


def test_resort_inside_a_chain():
    """carry_spatial_order refuses after 64 atom edits since the last sort: the next upload sorts for real and every slot moves -- here
    between two delta trials, with no full evaluation anywhere in the chain.  The box sits on the eight-tile edge, so the chain also
    crosses 512 | 513 atoms again and again."""
    n0, cell, seed = RESORT_BOX
    atoms, basis = ladder.ladder_box(n0, cell, seed)
    opts = options()
    rng = np.random.default_rng(7)
    S = energy.System(atoms, basis, opts, max_atoms=n0 + TILE)
    try:
        S.energy()
        carried0, sorted0 = util.upload_counts(S)
        edits, step, sort_seen, after_sort = 0, 0, False, 0
        with_oracle = False
        while after_sort < 3:
            assert step < 120, "no sort observed"
            last = sort_seen and after_sort == 2
            if len(atoms["pos"]) > n0:
                small = [mm for mm in molecules(atoms) if mm[1] - mm[0] <= 4]
                a, b = small[rng.integers(len(small))]
                trial = removed(atoms, a, b)
                S.trial_remove_energy(a, b - a)
                kind, m = "removal", b - a
            else:
                at, mol = small_insertion(rng, atoms, basis)
                trial = inserted(atoms, at, mol)
                S.trial_insert_energy(at, mol)
                kind, m = "insertion", len(mol["pos"])
            label = f"chain step {step} {kind} (n = {len(atoms['pos'])})"
            if with_oracle or last:  # the first exchange trial behind the observed sort, and the last one
                check_exchange(S, trial, basis, opts, label)
            check_exchange_fresh(S, trial, basis, opts, label)
            S.accept()
            atoms = trial
            edits += m
            assert abs(len(atoms["pos"]) - n0) <= 8
            before = util.upload_counts(S)
            mols = [mm for mm in molecules(atoms) if mm[1] - mm[0] <= 4]
            a, b = mols[rng.integers(len(mols))]
            displacement(S, atoms, basis, opts, a, b, 100 + step, label + ": displacement behind it")
            S.reject()
            now = util.upload_counts(S)
            assert sum(now) == sum(before) + 1, label  # the displacement trial uploaded the edited list
            with_oracle = now[1] > before[1]  # ... and sorted: a real sort between two delta trials
            if sort_seen:
                after_sort += 1
            sort_seen = sort_seen or with_oracle
            step += 1
        carried, sorted_ = util.upload_counts(S)
        assert edits > TILE and sorted_ > sorted0 and carried > carried0, (edits, carried, sorted_)
        assert util.exchange_counts(S) == (step, 0, 1)
        print(f"\nre-sort chain: {step} exchanges, {edits} atom edits, uploads carried {carried - carried0}, sorted {sorted_ - sorted0}")
    finally:
        S.close()
