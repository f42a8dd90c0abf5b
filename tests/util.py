"""shared helpers of the test-suite (tests may use the oracle; the product package may not)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "oracle"))

from mpmcxx_amd import pqr  # noqa: E402

REL_TOL = 1e-9  # BASELINE.json north_star: energies within 1e-9 relative of the reference CPU path

SMALL = ["ar2", "lj64", "ion64_es", "ion216_polar", "ion216_polar_nopbc", "ion216_triclinic", "ion216_frozen",
         "ion216_precision", "ion216_gamma", "ion216_alpha", "water64_polar", "lj1000", "ion1000_polar",
         "ion216_wolf", "water64_fh2", "water64_fh4", "ion216_fh4_polar", "ion216_gs", "water64_gs_precision", "ion1000_gs", "ion216_framework",
         "ion1000_triclinic"]
LARGE = ["ion10k_es", "ion10k_polar", "ion8000_triclinic"]

ENERGY_KEYS = [("energy", "total"), ("rd_energy", "rd"), ("coulombic_energy", "es"), ("polarization_energy", "polar"),
               ("es_real", "es_real"), ("es_recip", "es_recip"), ("es_self", "es_self"),
               ("lj_pairs", "lj_pairs"), ("lrc_pair", "lrc_pair"), ("lrc_self", "lrc_self")]
COUNT_KEYS = ["n_pairs", "n_intra", "n_rd_excluded", "n_es_excluded", "n_frozen", "n_lj_in_cutoff"]


def golden(name):
    with open(os.path.join(GOLDEN, f"{name}.json")) as f:
        return json.load(f)


def load_fixture(name):
    """(atoms, basis, options) parsed from the committed reference-format files."""
    return pqr.load_case(os.path.join(GOLDEN, f"{name}.in"))


def load_generated(name, tmpdir):
    """large boxes are regenerated deterministically instead of being committed as text."""
    from mpmcxx_amd import gen_box

    inp, _ = gen_box.materialize(name, str(tmpdir))
    return pqr.load_case(inp)


def close(a, b, tol=REL_TOL):
    if b == 0.0:
        return abs(a) <= tol
    return abs(a - b) <= tol * abs(b)


def assert_energies(res, g, rd_only, tol=REL_TOL, label="", wolf=False):
    bad = []
    for k_ours, k_gold in ENERGY_KEYS:
        if rd_only and k_gold in ("es", "es_real", "es_recip", "es_self", "polar"):
            continue
        if wolf and k_gold in ("es_real", "es_recip", "es_self"):
            continue  # with wolf on, coulombic() is coulombic_wolf(); the harness' Ewald component columns are not part of it
        if not close(res[k_ours], g[k_gold], tol):
            bad.append(f"{k_gold}: ours {res[k_ours]!r} ref {g[k_gold]!r}")
    assert not bad, f"{label} energy mismatch (tol {tol}): " + "; ".join(bad)


def assert_counts(res, g, rd_only, label=""):
    keys = list(COUNT_KEYS) + ([] if rd_only else ["n_es_in_cutoff"])
    bad = [f"{k}: ours {res[k]} ref {g[k]}" for k in keys if int(res[k]) != int(g[k])]
    assert not bad, f"{label} pair-count mismatch (must be bit-exact): " + "; ".join(bad)


def max_rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = np.abs(b).max()
    return float(np.abs(a - b).max() / scale) if scale > 0 else float(np.abs(a).max())


# ---- trial moves (mpmc_trial_*): shared by test_gpu_trial_moves and test_gpu_trial_branches -------------------------------------------
TRIAL_KEYS = ["energy", "rd_energy", "coulombic_energy", "polarization_energy", "es_real", "es_recip", "lj_pairs"]


def molecules(atoms):
    """(first, end) of every molecule: consecutive atoms with one mol_id"""
    ids = atoms["mol_id"]
    starts = [0] + [i for i in range(1, len(ids)) if ids[i] != ids[i - 1]] + [len(ids)]
    return [(starts[k], starts[k + 1]) for k in range(len(starts) - 1)]


def nonpolar(opts):
    o = dict(opts)
    o.update(polarization=0, polar_iterative=0)
    return o


def moved(atoms, first, m, seed, sigma=0.3):
    """trial positions of atoms [first, first + m): seeded per-atom Gaussian noise, so intramolecular distances change too"""
    rng = np.random.default_rng(seed)
    return atoms["pos"][first:first + m] + rng.normal(scale=sigma, size=(m, 3))


def with_positions(atoms, pos):
    a = dict(atoms)
    a["pos"] = pos
    return a


def component_errors(got, ref, keys, rel):
    """the components of `keys` where |got - ref| > rel * |ref|.  Relative per component, with no absolute floor: a component that is
    identically zero (the polarization energy of a non-polarizable box, the Ewald parts under Wolf) must be exactly 0.0 on both sides,
    so a delta that leaves a residue where there is no term fails.  None of the boxes of the trial tests has a component small enough
    against its terms for rounding to reach these tolerances (1e-11 against a fresh context, 1e-9 against the oracle); a case that
    needs a floor has to state it, with its bound, next to the comparison."""
    return [f"{k}: {got[k]!r} vs {ref[k]!r} (rel {abs(got[k] - ref[k]) / abs(ref[k]) if ref[k] else float('inf'):.2e})"
            for k in keys if not abs(got[k] - ref[k]) <= rel * abs(ref[k])]


def check_trial_against_fresh(S, atoms, basis, opts, pos, rel=1e-11, label=""):
    """S's last trial against a stateless evaluation of the trial configuration `pos` in a new context: every energy component at `rel`,
    the in-cutoff counts exactly.  Returns the fresh context's dipoles (mu, E0, E_ind) for polarizable boxes (None otherwise)."""
    from mpmcxx_amd import energy

    T = energy.System(with_positions(atoms, pos), basis, opts)
    try:
        T.energy()
        got, ref = S.trial_observables, T.observables
        bad = component_errors(got, ref, TRIAL_KEYS, rel)
        assert not bad, f"{label}: trial vs fresh context (rel {rel}): " + "; ".join(bad)
        for k in ("n_lj_in_cutoff", "n_es_in_cutoff", "polar_iterations"):
            assert got[k] == ref[k], (label, k, got[k], ref[k])
        return T.dipoles() if opts.get("polarization") and not opts.get("rd_only") else None
    finally:
        T.close()


def check_trial_against_oracle(obs, atoms, basis, opts, pos, rel=REL_TOL, label=""):
    """trial observables against the oracle on the trial configuration: per component at `rel`, counts bit-exact, the same number of
    dipole iterations.  (Under Wolf the oracle reports the Coulomb energy alone, no Ewald parts and no count.)"""
    from oracle import OracleSystem

    ref = OracleSystem(with_positions(atoms, pos), basis, opts).energy(want_atoms=False)
    wolf = bool(opts.get("wolf"))
    keys = [k for k in TRIAL_KEYS if not (wolf and k in ("es_real", "es_recip"))]
    bad = component_errors(obs, ref, keys, rel)
    assert not bad, f"{label}: trial vs oracle (rel {rel}): " + "; ".join(bad)
    assert obs["n_lj_in_cutoff"] == ref["n_lj_in_cutoff"], (label, obs["n_lj_in_cutoff"], ref["n_lj_in_cutoff"])
    if not wolf:
        assert obs["n_es_in_cutoff"] == ref["n_es_in_cutoff"], (label, obs["n_es_in_cutoff"], ref["n_es_in_cutoff"])
    if opts.get("polarization") and not opts.get("rd_only"):
        assert obs["polar_iterations"] == ref["polar_iterations"], (label, obs["polar_iterations"], ref["polar_iterations"])
    return ref
