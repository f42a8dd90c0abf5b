"""GPU (MI355X): batched insertion candidates (mpmc_insert_candidates, kernels_insert_batch.hip).

out[c] of a batch must be the mpmc_result of mpmc_trial_insert_begin(pose c) + mpmc_trial_energy + mpmc_trial_reject on the same context,
in every field and bit for bit, whatever the batch size, the internal chunking and the candidate's place in the batch; the call leaves the
accepted state as it found it.  The candidates are also held to the oracle and to a fresh context by the rules of
test_gpu_exchange_moves.check_exchange (1e-9 per component against the oracle, counts bit-exact, the position-independent terms, N and NU;
1e-11 against a stateless evaluation of the inserted list).  Poses: rotated copies of one molecule of the box, centres uniform over
fractional coordinates in [-1, 2), so wrapped images occur."""
import json
import re
import struct
import subprocess

import numpy as np
import pytest

import test_gpu_size_ladder as ladder
import util
from mpmcxx_amd import energy
from test_gpu_exchange_moves import check_exchange, inserted, molecule, random_rotation, removed

pytestmark = pytest.mark.gpu

molecules = util.molecules
nonpolar = util.nonpolar
ERR_ARG, ERR_INVALID_DATUM, ERR_UNSUPPORTED = -3, 6001, energy.ERR_UNSUPPORTED
FIXTURES = ["lj64", "ion64_es", "water64_polar", "ion216_triclinic", "ion216_frozen", "ion216_wolf", "water64_fh2"]
GENERATED = "gen1100"  # 1100 atoms = 18 tiles (past 16), triclinic, Ewald, with the 320-site frozen framework molecule of the ladder boxes
CASES = FIXTURES + [GENERATED]
SMALL = ["lj64", "ion64_es", "water64_polar", "water64_fh2"]  # every candidate goes to the oracle; six of the batch on the larger boxes
N_BATCH = 65
TRIAL_MAX = int(re.findall(r"#define MPMC_TRIAL_MAX_ATOMS (\d+)", open(util.ROOT + "/include/mpmc_energy.h").read())[0])
CAP = int(re.findall(r"#define MPMC_INSERT_MAX_CANDIDATES (\d+)", open(util.ROOT + "/include/mpmc_energy.h").read())[0])
CHUNK = int(re.findall(r"\bkInsBatchChunk\s*=\s*(\d+)\s*;", util.csrc_text("kernels.h"))[0])  # candidates per internal launch chain


def bits(obs):
    """every field of an observables dict as its bit pattern (so that -0.0 and 0.0 differ and a NaN equals itself)"""
    return tuple((k, struct.pack("<d", v) if isinstance(v, float) else int(v)) for k, v in sorted(obs.items()))


def load(name):
    if name == GENERATED:
        atoms, basis = ladder.ladder_box(1100, "triclinic", 31)
        opts = ladder.options()
    else:
        atoms, basis, opts = util.load_fixture(name)
        opts = nonpolar(opts)
    return {k: np.array(v) for k, v in atoms.items()}, basis, opts


def poses_of(rng, atoms, basis, n_cand, size=None):
    """one species (a molecule of the box, the first mobile one of `size` sites if given) and n_cand poses of it: (mol, (n_cand, m, 3))"""
    mols = [(a, b) for a, b in molecules(atoms) if not atoms["frozen"][b - 1] and (size is None or b - a == size)]
    a, b = mols[rng.integers(len(mols))]
    p = atoms["pos"][a:b]
    rel = p - p.mean(axis=0)
    B = np.asarray(basis).reshape(3, 3)
    out = np.empty((n_cand, b - a, 3))
    for c in range(n_cand):
        r = rel @ random_rotation(rng).T if b - a > 1 else rel
        out[c] = r + rng.uniform(-1.0, 2.0, size=3) @ B
    return molecule(atoms, a, b), out


def synthetic_species(atoms, m, seed):
    """m charged Lennard-Jones sites with the per-atom keys of `atoms` (as test_gpu_exchange_moves.test_long_molecule builds its molecule);
    for m >= 3 one site has no dispersion and one no charge"""
    rng = np.random.default_rng(seed)
    mol = {k: np.repeat(v, m, axis=0) for k, v in molecule(atoms, 0, 1).items()}
    mol["pos"] = rng.normal(scale=1.2 if m < 64 else 4.0, size=(m, 3))
    mol["charge"] = np.where(np.arange(m) % 2 == 0, 0.35, -0.35) * ladder.E2R
    mol["epsilon"] = np.linspace(20.0, 60.0, m)
    mol["sigma"] = np.linspace(2.5, 3.5, m)
    mol["polarizability"] = np.zeros(m)
    mol["frozen"] = np.zeros(m, dtype=mol["frozen"].dtype)
    if m >= 3:
        mol["epsilon"][1], mol["charge"][2] = 0.0, 0.0
    return mol


def poses_around(rng, mol, basis, n_cand):
    rel = mol["pos"] - mol["pos"].mean(axis=0)
    B = np.asarray(basis).reshape(3, 3)
    return np.stack([rel @ random_rotation(rng).T + rng.uniform(-1.0, 2.0, size=3) @ B for _ in range(n_cand)])


def single(S, mol, pose):
    """begin / energy / reject of one pose (appended: at_index does not enter a delta-path result)"""
    S.trial_insert_energy(S.n, dict(mol, pos=pose))
    assert not S.last_trial_was_full()
    obs = dict(S.trial_observables)
    S.reject()
    return obs


class Evaluated:
    """what check_exchange reads of a System, for a candidate of a batch"""

    def __init__(self, obs):
        self.trial_observables = obs

    def last_trial_was_full(self):
        return False


def check_candidate(obs, atoms, basis, opts, mol, pose, label):
    check_exchange(Evaluated(obs), inserted(atoms, len(atoms["pos"]), dict(mol, pos=pose)), basis, opts, label)


_BATCH = {}


def batch_of(name):
    """(atoms, basis, opts, mol, poses, batch observables, single-trial observables before and after the batch, the accepted observables
    before and after): made once per box, shared by the tests below and left unchanged"""
    if name not in _BATCH:
        atoms, basis, opts = load(name)
        mol, P = poses_of(np.random.default_rng(77), atoms, basis, N_BATCH, size=3 if name.startswith("water") else None)
        S = energy.System(atoms, basis, opts)
        S.energy()
        acc0 = dict(S.observables)
        before = [single(S, mol, P[c]) for c in range(N_BATCH)]
        xc = util.exchange_counts(S)
        batch = S.insert_candidates(mol, P)
        assert util.exchange_counts(S) == xc and S.insert_batch_counts() == (1, N_BATCH)  # no trial was opened for it
        after = [single(S, mol, P[c]) for c in range(N_BATCH)]
        S.energy()
        acc1 = dict(S.observables)
        S.close()
        _BATCH[name] = (atoms, basis, opts, mol, P, batch, before, after, acc0, acc1)
    return _BATCH[name]


# ---- 1. equal to the single trial, bit for bit --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_batch_equals_single_trials_bit_for_bit(name):
    atoms, basis, opts, mol, P, batch, before, after, acc0, acc1 = batch_of(name)
    assert len(batch) == N_BATCH and set(batch[0]) == set(before[0])
    for c in range(N_BATCH):
        assert bits(batch[c]) == bits(before[c]), (name, c, {k: (batch[c][k], before[c][k]) for k in batch[c] if batch[c][k] != before[c][k]})
        assert bits(batch[c]) == bits(after[c]), (name, c, "single trial after the batch")
    assert bits(acc0) == bits(acc1), name  # energy() returns the bits it returned before
    # the candidates are not all alike (wrapped and unwrapped centres, in and out of each other's cutoff)
    assert len({batch[c]["energy"] for c in range(N_BATCH)}) == N_BATCH
    if name == GENERATED:
        assert (len(atoms["pos"]) + 63) // 64 > 16


# ---- 2. against the oracle and a fresh context --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_batch_against_oracle_and_fresh_context(name):
    atoms, basis, opts, mol, P, batch = batch_of(name)[:6]
    which = range(N_BATCH) if name in SMALL else [0, 13, 31, 47, 63, 64]
    for c in which:
        check_candidate(batch[c], atoms, basis, opts, mol, P[c], f"{name} candidate {c}")


# ---- 3. batch shapes ----------------------------------------------------------------------------------------------------------------------
def test_batch_sizes_and_internal_chunks():
    atoms, basis, opts = load("ion64_es")
    rng = np.random.default_rng(5)
    mol, P = poses_of(rng, atoms, basis, 2 * CHUNK + 1)
    S = energy.System(atoms, basis, opts)
    S.energy()
    whole = S.insert_candidates(mol, P)
    sizes = sorted({1, 2, 63, 64, 65, 257, CHUNK, CHUNK + 1})
    for n in sizes:
        part = S.insert_candidates(mol, P[:n])
        assert len(part) == n and [bits(o) for o in part] == [bits(o) for o in whole[:n]], n
    for c in sorted({0, 1, 62, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK}):
        assert bits(single(S, mol, P[c])) == bits(whole[c]), c
    assert [bits(o) for o in S.insert_candidates(mol, P)] == [bits(o) for o in whole]  # a repeated call: the same bits
    assert S.insert_batch_counts() == (len(sizes) + 2, sum(sizes) + 2 * len(P))
    S.close()


def test_result_is_independent_of_the_place_in_the_batch():
    atoms, basis, opts = load("water64_polar")
    rng = np.random.default_rng(6)
    mol, P = poses_of(rng, atoms, basis, CHUNK + 44, size=3)
    places = [0, 63, 64, len(P) - 1]
    for p in places:
        P[p] = P[7]
    S = energy.System(atoms, basis, opts)
    S.energy()
    got = S.insert_candidates(mol, P)
    want = bits(single(S, mol, P[7]))
    for p in places + [7]:
        assert bits(got[p]) == want, p
    S.close()


@pytest.mark.parametrize("m", [1, 3, 5])
def test_molecule_sizes(m):
    atoms, basis, opts = load("ion216_triclinic")
    mol = synthetic_species(atoms, m, 40 + m)
    P = poses_around(np.random.default_rng(m), mol, basis, N_BATCH)
    S = energy.System(atoms, basis, opts)
    S.energy()
    got = S.insert_candidates(mol, P)
    for c in range(N_BATCH):
        assert bits(got[c]) == bits(single(S, mol, P[c])), (m, c)
    for c in (0, 64):
        check_candidate(got[c], atoms, basis, opts, mol, P[c], f"m = {m} candidate {c}")
    S.close()


def test_longest_molecule_and_more_than_one_staging_pass():
    """m = MPMC_TRIAL_MAX_ATOMS: the staging block holds 2^17 records, so 2^17 / m + 2 candidates take a second pass"""
    atoms, basis, opts = load("lj64")
    m = TRIAL_MAX
    mol = synthetic_species(atoms, m, 3)
    n_cand = (1 << 17) // m + 2
    P = poses_around(np.random.default_rng(8), mol, basis, n_cand)
    S = energy.System(atoms, basis, opts)
    S.energy()
    got = S.insert_candidates(mol, P)
    for c in (0, 1, CHUNK, n_cand - 3, n_cand - 2, n_cand - 1):
        assert bits(got[c]) == bits(single(S, mol, P[c])), c
    check_candidate(got[n_cand - 1], atoms, basis, opts, mol, P[n_cand - 1], "longest molecule, last candidate")
    S.close()


# ---- 4. on carried state ------------------------------------------------------------------------------------------------------------------
def check_batch_here(S, atoms, basis, opts, mol, P, label, fresh=(0, 5)):
    got = S.insert_candidates(mol, P)
    for c in range(len(P)):
        assert bits(got[c]) == bits(single(S, mol, P[c])), (label, c)
    for c in fresh:
        check_candidate(got[c], atoms, basis, opts, mol, P[c], f"{label} candidate {c}")
    return got


@pytest.mark.parametrize("name", ["water64_polar", "ion64_es"])
def test_batches_on_carried_state(name):
    atoms, basis, opts = load(name)
    rng = np.random.default_rng(9)
    mol, P = poses_of(rng, atoms, basis, 20, size=3 if name.startswith("water") else None)
    S = energy.System(atoms, basis, opts, max_atoms=256)
    S.energy()
    # directly behind an accepted insertion: the upload of the edited list is pending
    S.trial_insert_energy(molecules(atoms)[4][0], dict(mol, pos=P[3]))
    S.accept()
    atoms = inserted(atoms, molecules(atoms)[4][0], dict(mol, pos=P[3]))
    check_batch_here(S, atoms, basis, opts, mol, P, f"{name} behind an accepted insertion")
    # behind an accepted removal
    a, b = molecules(atoms)[11]
    S.trial_remove_energy(a, b - a)
    S.accept()
    atoms = removed(atoms, a, b)
    check_batch_here(S, atoms, basis, opts, mol, P, f"{name} behind an accepted removal")
    # behind a rejected displacement
    a, b = molecules(atoms)[2]
    S.trial_energy(a, atoms["pos"][a:b] + 0.3)
    S.reject()
    got = check_batch_here(S, atoms, basis, opts, mol, P, f"{name} behind a rejected displacement")
    # a chosen candidate, taken through the single trial and accepted: the result bits are the batch's, and the next batch works on the
    # new composition
    pick = 12
    S.trial_insert_energy(S.n, dict(mol, pos=P[pick]))
    assert bits(S.trial_observables) == bits(got[pick])
    S.accept()
    assert bits(S.observables) == bits(got[pick])
    atoms = inserted(atoms, len(atoms["pos"]), dict(mol, pos=P[pick]))
    check_batch_here(S, atoms, basis, opts, mol, P[:8], f"{name} second batch")
    ref = util.oracle_energy(atoms, basis, opts)
    assert util.close(S.energy(), ref["energy"])
    util.assert_counts(S.observables, ref, bool(opts.get("rd_only")) or bool(opts.get("wolf")), label=name)
    S.close()


def test_eight_contexts_one_after_the_other():
    base, basis, opts = load("ion64_es")
    rng = np.random.default_rng(10)
    mol, P = poses_of(rng, base, basis, 33)
    boxes = [dict(base, pos=base["pos"] + np.random.default_rng(100 + k).normal(scale=0.05, size=base["pos"].shape)) for k in range(8)]
    alone = []
    for k in range(8):
        S = energy.System(boxes[k], basis, opts)
        S.energy()
        alone.append([bits(o) for o in S.insert_candidates(mol, P)])
        S.close()
    held = [energy.System(boxes[k], basis, opts) for k in range(8)]
    for S in held:
        S.energy()
    together = [[bits(o) for o in S.insert_candidates(mol, P)] for S in held]
    again = [[bits(o) for o in S.insert_candidates(mol, P)] for S in reversed(held)][::-1]
    for S in held:
        S.close()
    assert together == alone and again == alone
    assert len({t[0] for t in alone}) == 8  # (the eight boxes do differ)


# ---- 5. refusals and arguments ------------------------------------------------------------------------------------------------------------
def fails(code, fn, *args):
    with pytest.raises(energy.MpmcError) as e:
        fn(*args)
    assert e.value.code == code, (e.value.code, str(e.value))
    assert len(str(e.value)) > len(f"mpmc error {code}: "), str(e.value)  # a text comes with the code


def test_refusals_and_arguments():
    atoms, basis, opts = load("ion64_es")
    rng = np.random.default_rng(11)
    mol, P = poses_of(rng, atoms, basis, 5)
    m = P.shape[1]
    S = energy.System(atoms, basis, opts)
    fails(ERR_ARG, S.insert_candidates, mol, P)  # no accepted configuration
    S.energy()
    want = [bits(single(S, mol, P[c])) for c in range(5)]

    def usable():
        assert [bits(o) for o in S.insert_candidates(mol, P)] == want
        assert bits(single(S, mol, P[2])) == want[2]

    usable()
    a, b = molecules(atoms)[3]
    S.trial_energy(a, atoms["pos"][a:b] + 0.1)
    fails(ERR_ARG, S.insert_candidates, mol, P)  # an open trial
    S.reject()
    usable()
    fails(ERR_ARG, S.insert_candidates, mol, P[:0])  # n_cand = 0
    fails(ERR_ARG, S.insert_candidates, mol, np.zeros((CAP + 1, m, 3)))
    usable()
    long_mol = synthetic_species(atoms, TRIAL_MAX + 1, 1)
    fails(ERR_UNSUPPORTED, S.insert_candidates, long_mol, long_mol["pos"][None, :, :])  # count above the limit
    bad = P.copy()
    bad[3, m - 1, 1] = np.nan
    fails(ERR_INVALID_DATUM, S.insert_candidates, mol, bad)  # NaN in one candidate
    bad[3, m - 1, 1] = np.inf
    fails(ERR_INVALID_DATUM, S.insert_candidates, mol, bad)
    usable()
    counts = S.insert_batch_counts()
    # terms without an insertion delta
    S.set_rd_crystal(True, 2)
    S.energy()
    fails(ERR_UNSUPPORTED, S.insert_candidates, mol, P)
    S.set_rd_crystal(False, 0)
    S.set_rd_model("lj", "waldmanhagler")
    S.energy()
    fails(ERR_UNSUPPORTED, S.insert_candidates, mol, P)
    S.set_rd_model(0, 0)
    # Axilrod-Teller coefficients: refused in front of the accepted-configuration check, as the single trial refuses
    S.set_axilrod_teller(True, c9=np.full(len(atoms["pos"]), 100.0))
    fails(ERR_UNSUPPORTED, S.insert_candidates, mol, P)
    fails(ERR_UNSUPPORTED, S.trial_insert_energy, S.n, dict(mol, pos=P[0]))
    S.set_axilrod_teller(False)
    assert S.insert_batch_counts() == counts  # refused calls are not counted
    S.energy()
    usable()
    S.close()
    # a polarizable box
    patoms, pbasis, popts = util.load_fixture("water64_polar")
    T = energy.System(patoms, pbasis, popts)
    T.energy()
    pmol, PP = poses_of(rng, {k: np.array(v) for k, v in patoms.items()}, pbasis, 3, size=3)
    fails(ERR_UNSUPPORTED, T.insert_candidates, pmol, PP)
    e = T.trial_insert_energy(T.n, dict(pmol, pos=PP[0]))  # ... whose single trial (a full evaluation) still works
    assert T.last_trial_was_full() and np.isfinite(e)
    T.reject()
    T.close()


# ---- 6. the C++ facade --------------------------------------------------------------------------------------------------------------------
def test_cpp_facade_insert_candidates(tmp_path):
    import test_insert_candidates

    exe = test_insert_candidates.build(tmp_path)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["n_batch"] == 70 and r["mismatches"] == 0  # every field of every candidate: energy_trial_insert + reject_trial
    assert r["e_after"] == r["e0"]  # the accepted state is untouched
    assert r["e_in"] == r["e_batch_17"] and r["n_in"] == 130  # the accepted candidate has the batch's bits
    assert r["n_second"] == 70 and r["N_second"] == 66.0 and r["refused"] == ERR_ARG
