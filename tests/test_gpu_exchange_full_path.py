"""GPU (MI355X): exchange trials that evaluate the trial composition in full, each with the state it carries, and the refusal.

xch_energy_async takes the full path for a polarizable box, for rd_crystal, for a non-default rd model and for molecules of more than
MPMC_TRIAL_MAX_ATOMS atoms (the last: test_gpu_exchange_ladder).  Each has state of its own across the verdict: the kept-terms counts
(rc_terms_accepted, rdm_terms_accepted), the saved list that a reject puts back, the re-base of the structure factors behind a reject
(not for polarizable boxes, whose real-space field is marked stale instead, and not under Wolf), the cached pair correction of the LJ
form.  Per case and verdict: an insertion and a removal, each held to a fresh context with the same term on (1e-11 per component, every
count and the term's kept-terms count exactly) and to the reference test_gpu_rd_model / test_gpu_rd_crystal / test_gpu_exchange_moves /
test_gpu_polar_relax hold a full evaluation to, at their tolerances; and straight behind every verdict, with NO energy() in between, a
displacement trial against a fresh context on the list the verdict left.

The refusal: a context with Axilrod-Teller or disp-expansion coefficients answers an exchange trial with MPMC_ERR_UNSUPPORTED -- also
straight behind the call that switched the term on, which drops the accepted totals -- and stays usable."""
import numpy as np
import pytest

import util  # (first: it puts the oracle's directory on the path, which the restatements below import from)
import polar_relax_ref
import rd_crystal_ref
import rd_model_ref
from mpmcxx_amd import energy
from test_gpu_exchange_moves import count_N, inserted, molecule, random_insertion, removed

pytestmark = pytest.mark.gpu

molecules = util.molecules
MODEL_KEYS = energy.RD_MODEL_KEYS + ("rd_crystal", "rd_crystal_order")
KEYS = util.TRIAL_KEYS + ["lrc_pair", "lrc_self", "es_self"]
COUNTS = util.COUNT_KEYS + ["n_es_in_cutoff", "n_pairs", "polar_iterations"]
REF_REL_POLAR = util.REL_TOL + 8e-13  # test_gpu_polar_relax.REF_REL_E: 1e-9 plus ten times the restatement's own distance from the reference


def _water_rdm(name):
    atoms, basis, opts = rd_model_ref.load(name)
    return atoms, basis, util.nonpolar(opts)  # (the rd model is the reason for the full path, not a dipole solve)


def _crystal(tmp):
    atoms, basis, opts = rd_crystal_ref.load("water64_polar_rc2")
    return atoms, basis, util.nonpolar(opts)


def _wolf_b147(tmp):
    atoms, basis, opts = util.load_fixture("ion216_wolf")
    return atoms, basis, dict(util.nonpolar(opts), lj_buffered_14_7=1)


# case -> (loader, what the case is: the term whose kept-terms count is compared, whether a displacement trial has a delta path)
CASES = {
    "rd_crystal": (_crystal, "crystal"),
    "rd_lj_waldmanhagler": (lambda tmp: _water_rdm("water64_polar_rdm_ljwh"), "model"),  # the LJ form: the cached pair correction
    "rd_buffered_14_7": (lambda tmp: _water_rdm("water64_polar_rdm_b147hal"), "model"),
    "polar_jacobi": (lambda tmp: util.load_fixture("water64_polar"), "polar"),
    "polar_zodid": (lambda tmp: util.load_generated("water64_polar_rx_zodid", tmp), "zodid"),
    "wolf_buffered_14_7": (_wolf_b147, "model"),  # a reject under Wolf does not re-base
}


def term_info(S, what):
    if what == "crystal":
        return S.rd_crystal_info()
    if what == "model":
        return S.rd_model_info()
    return {}


def fresh(atoms, basis, opts, what):
    T = energy.System(atoms, basis, opts)
    try:
        T.energy()
        return dict(T.observables), term_info(T, what)
    finally:
        T.close()


def against_fresh(obs, info, atoms, basis, opts, what, label):
    ref, ref_info = fresh(atoms, basis, opts, what)
    bad = util.component_errors(obs, ref, KEYS, 1e-11)
    assert not bad, f"{label}: vs fresh context (rel 1e-11): " + "; ".join(bad)
    for k in COUNTS:
        assert obs[k] == ref[k], (label, k, obs[k], ref[k])
    # the term's own record: its kept terms exactly (n_tile_pairs_skipped is the spatial order's, not the list's)
    for k in ("form", "mixing", "n_terms", "order", "n_images", "n_image_terms"):
        assert info.get(k) == ref_info.get(k), (label, k, info, ref_info)
    for k in ("cutoff", "crystal_self"):
        assert k not in info or abs(info[k] - ref_info[k]) <= 1e-11 * abs(ref_info[k]), (label, k, info, ref_info)
    assert obs["N"] == ref["N"] == count_N(atoms), label


def against_reference(obs, info, atoms, basis, opts, what, label):
    """the trial against the yardstick of a full evaluation of its term"""
    from oracle import OracleSystem

    plain = {k: v for k, v in opts.items() if k not in MODEL_KEYS}
    if what == "polar":  # the oracle, as test_gpu_exchange_moves
        util.check_trial_against_oracle(obs, atoms, basis, opts, atoms["pos"], label=label)
        return
    # everything but the term: the oracle on the same list without it
    ref = OracleSystem(atoms, basis, util.nonpolar(plain)).energy(want_atoms=False)
    keys = ["coulombic_energy"] + ([] if opts.get("wolf") else ["es_real", "es_recip", "es_self"])
    bad = util.component_errors(obs, ref, keys, util.REL_TOL)
    assert not bad, f"{label}: electrostatics vs oracle: " + "; ".join(bad)
    if not opts.get("wolf"):
        assert obs["n_es_in_cutoff"] == ref["n_es_in_cutoff"], label
    if what == "zodid":  # the restatement of test_gpu_polar_relax; the plain rd terms are the oracle's
        bad = util.component_errors(obs, ref, ["rd_energy", "lj_pairs", "lrc_pair", "lrc_self"], util.REL_TOL)
        assert not bad, f"{label}: rd vs oracle: " + "; ".join(bad)
        want = polar_relax_ref.solve(atoms, basis, opts)["polarization_energy"]
        assert abs(obs["polarization_energy"] - want) <= REF_REL_POLAR * abs(want), (label, obs["polarization_energy"], want)
        return
    r = (rd_crystal_ref if what == "crystal" else rd_model_ref).for_case(atoms, basis, opts)
    # the pair sum to 1e-12 of the summed magnitudes of its terms, the corrections to 1e-12 relative, the kept terms exactly
    assert abs(obs["lj_pairs"] - r["lj_pairs"]) <= 1e-12 * r["mag"], (label, obs["lj_pairs"], r)
    assert abs(obs["lrc_pair"] - r["lrc_pair"]) <= 1e-12 * abs(r["lrc_pair"]), (label, obs["lrc_pair"], r)
    assert abs(obs["lrc_self"] - r["lrc_self"]) <= 1e-12 * abs(r["lrc_self"]), (label, obs["lrc_self"], r)
    if what == "crystal":
        assert abs(info["crystal_self"] - r["crystal_self"]) <= 1e-12 * abs(r["crystal_self"]), (label, info, r)
        assert info["n_image_terms"] == r["n_image_terms"], (label, info, r["n_image_terms"])
        assert obs["rd_energy"] == ((obs["lj_pairs"] + obs["lrc_pair"]) + info["crystal_self"]) + obs["lrc_self"], label
    else:
        assert info["n_terms"] == r["n_terms"], (label, info, r["n_terms"])


def displacement_behind(S, atoms, basis, opts, what, k, seed, label):
    """a displacement trial of molecule k with no evaluation since the verdict, against a fresh context; rejected"""
    a, b = molecules(atoms)[k]
    trial = dict(atoms, pos=atoms["pos"].copy())
    trial["pos"][a:b] = util.moved(atoms, a, b - a, seed)
    S.trial_energy(a, trial["pos"][a:b])
    if what in ("model", "crystal"):
        assert not S.last_trial_was_full(), label  # these terms have a displacement delta
    obs, info = dict(S.trial_observables), term_info(S, what)
    util.check_trial_against_fresh(S, trial, basis, opts, trial["pos"], rel=1e-11, label=label)
    ref, ref_info = fresh(trial, basis, opts, what)
    bad = util.component_errors(obs, ref, ["lrc_pair", "lrc_self", "es_self"], 1e-11)
    assert not bad, (label, bad)
    for key in ("n_terms", "n_image_terms"):
        if key in info:
            assert info[key] == ref_info[key], (label, key, info[key], ref_info[key])
    S.reject()


@pytest.mark.parametrize("verdict", ["accept", "reject"])
@pytest.mark.parametrize("case", list(CASES))
def test_full_path_exchange_and_the_trial_behind_its_verdict(case, verdict, tmp_path):
    loader, what = CASES[case]
    atoms, basis, opts = loader(tmp_path)
    atoms = {k: np.array(v) for k, v in atoms.items()}
    rng = np.random.default_rng(41)
    S = energy.System(atoms, basis, opts, max_atoms=len(atoms["pos"]) + 64)
    try:
        S.energy()
        full = 0
        for kind in ("insert", "remove"):
            if kind == "insert":
                at, mol = random_insertion(rng, atoms, basis)
                trial = inserted(atoms, at, mol)
                S.trial_insert_energy(at, mol)
            else:
                a, b = molecules(atoms)[9]
                trial = removed(atoms, a, b)
                S.trial_remove_energy(a, b - a)
            label = f"{case} {kind} ({verdict})"
            full += 1
            assert S.last_trial_was_full() and util.exchange_counts(S)[:2] == (0, full), label
            obs, info = dict(S.trial_observables), term_info(S, what)
            against_fresh(obs, info, trial, basis, opts, what, label)
            against_reference(obs, info, trial, basis, opts, what, label)
            assert obs["NU"] == obs["N"] * obs["energy"], label
            if verdict == "accept":
                S.accept()
                atoms = trial
            else:
                S.reject()
            assert S.n == len(atoms["pos"]) if verdict == "accept" else True
            # no energy() here: the next trial meets whatever the verdict left
            displacement_behind(S, atoms, basis, opts, what, 23, 50 + full, label + ": displacement behind the verdict")
        S.energy()
        against_fresh(dict(S.observables), term_info(S, what), atoms, basis, opts, what, f"{case} ({verdict}): energy() at the end")
    finally:
        S.close()


# ---- the refusal -------------------------------------------------------------------------------------------------------------------------------
def _refused(fn, *args):
    with pytest.raises(energy.MpmcError) as e:
        fn(*args)
    assert e.value.code == energy.ERR_UNSUPPORTED, (e.value.code, str(e.value))
    assert str(e.value).split(":", 1)[1].strip(), str(e.value)  # a message behind the code


@pytest.mark.parametrize("term", ["axilrod_teller", "disp_expansion"])
def test_exchange_trials_are_refused_with_per_atom_coefficients(term):
    atoms, basis, opts = util.load_fixture("ion64_es")
    opts = util.nonpolar(opts)
    atoms = {k: np.array(v) for k, v in atoms.items()}
    n = len(atoms["pos"])
    rng = np.random.default_rng(3)
    if term == "disp_expansion":  # (epsilon and sigma are the term's exponent and radius: values of its own fixtures)
        atoms["epsilon"], atoms["sigma"] = rng.uniform(2.8, 3.4, n), rng.uniform(3.2, 3.6, n)
    coeff = [rng.uniform(500.0, 2000.0, n)] if term == "axilrod_teller" else [rng.uniform(50.0, 80.0, n), rng.uniform(1400.0, 1800.0, n), rng.uniform(4e4, 6e4, n)]

    def switch_on(T):
        if term == "axilrod_teller":
            T.set_axilrod_teller(True, c9=coeff[0])
        else:
            T.set_disp_expansion(True, *coeff)

    a, b = molecules(atoms)[4]
    mol = molecule(atoms, a, b, atoms["pos"][a:b] + 1.0)
    untouched = energy.System(atoms, basis, opts)
    switch_on(untouched)
    want = untouched.energy()
    want_obs = dict(untouched.observables)
    assert np.isfinite(want)
    untouched.close()
    S = energy.System(atoms, basis, opts, max_atoms=n + 64)
    try:
        plain = S.energy()
        switch_on(S)
        # straight behind the switch (the accepted totals are gone): still the refusal, not "call mpmc_energy first"
        _refused(S.trial_insert_energy, a, mol)
        _refused(S.trial_remove_energy, a, b - a)
        assert S.energy() == want != plain and dict(S.observables) == want_obs  # the bits of a context that never saw the refused calls
        _refused(S.trial_insert_energy, a, mol)
        _refused(S.trial_remove_energy, a, b - a)
        assert S.energy() == want and dict(S.observables) == want_obs and S.n == n
        trial = dict(atoms, pos=atoms["pos"].copy())
        trial["pos"][a:b] += 0.25
        S.trial_energy(a, trial["pos"][a:b])
        assert not S.last_trial_was_full()
        T = energy.System(trial, basis, opts)
        switch_on(T)
        T.energy()
        bad = util.component_errors(S.trial_observables, T.observables, util.TRIAL_KEYS + ["three_body_energy"], 1e-11)
        T.close()
        assert not bad, bad
        S.accept()
        assert util.exchange_counts(S) == (0, 0, 0)
    finally:
        S.close()
