"""GPU (MI355X): trial-move (delta) energies against full re-evaluation and the oracle.

A Metropolis-like sequence of molecule displacements: every trial energy must equal a stateless full evaluation of the
same configuration (fresh context) to rounding, rejected moves must leave no trace, and after the whole sequence the
accumulated totals must still agree with the oracle at 1e-9."""
import numpy as np
import pytest

import util
from mpmcxx_amd import energy

pytestmark = pytest.mark.gpu


molecules = util.molecules
nonpolar = util.nonpolar


@pytest.mark.parametrize("name,polar", [("lj64", False), ("ion64_es", False), ("water64_polar", False), ("ion216_triclinic", False),
                                        ("ion216_frozen", False), ("water64_polar", True), ("ion216_wolf", False), ("water64_fh2", False),
                                        ("ion216_polar", True), ("ion216_polar_nopbc", True), ("ion216_triclinic", True), ("ion216_framework", True),
                                        ("ion1000_polar", True), ("ion216_precision", True), ("water64_fh4", False), ("ion216_fh4_polar", True),
                                        ("ion216_fh4_polar", False)])
def test_trial_moves_track_full_evaluations(name, polar):
    from oracle import OracleSystem

    # Per component: 1e-11 relative against a fresh context, 1e-9 relative against the oracle, no absolute floor (util.component_errors)
    atoms, basis, opts = util.load_fixture(name)
    if not polar:
        opts = nonpolar(opts)
    rng = np.random.default_rng(11)
    S = energy.System(atoms, basis, opts)
    e_acc = S.energy()
    pos = atoms["pos"].copy()
    mols = molecules(atoms)
    n_steps = 6 if polar else 40
    n_acc = 0
    for step in range(n_steps):
        a, b = mols[rng.integers(len(mols))]
        trial = pos[a:b] + rng.normal(scale=0.4, size=(b - a, 3))
        e_trial = S.trial_energy(a, trial)
        # per-move delta energies, not a full evaluation in disguise -- Wolf and Feynman-Hibbs included (round 3); the one combination
        # that keeps the full evaluation is a polarizable box under Wolf, which no fixture holds
        assert not S.last_trial_was_full(), name
        full_pos = pos.copy()
        full_pos[a:b] = trial
        util.check_trial_against_fresh(S, atoms, basis, opts, full_pos, rel=1e-11, label=f"{name} step {step}")
        # ... and the ORACLE on the same trial configuration, every step (1e-9 per component, counts bit-exact)
        ref_t = util.check_trial_against_oracle(S.trial_observables, atoms, basis, opts, full_pos, label=f"{name} step {step}")
        assert util.close(e_trial, ref_t["energy"])
        if rng.random() < 0.5:
            S.accept()
            pos = full_pos
            e_acc = e_trial
            n_acc += 1
        else:
            S.reject()
    assert 0 < n_acc < n_steps
    # a stateless full evaluation of the final resident state, and the oracle on the same positions
    e_final = S.energy()
    at3 = dict(atoms)
    at3["pos"] = pos
    ref = OracleSystem(at3, basis, opts).energy()
    assert util.close(e_final, ref["energy"]) and util.close(e_acc, ref["energy"], 1e-10)
    S.close()


def test_trial_protocol_errors():
    atoms, basis, opts = util.load_fixture("lj64")
    S = energy.System(atoms, basis, opts)
    with pytest.raises(energy.MpmcError):  # no accepted configuration yet
        S.trial_energy(0, atoms["pos"][0:1])
    S.energy()
    S.trial_energy(0, atoms["pos"][0:1] + 0.1)
    with pytest.raises(energy.MpmcError):  # a trial is already open
        S.trial_energy(1, atoms["pos"][1:2])
    S.reject()
    with pytest.raises(energy.MpmcError):
        S.reject()
    S.close()


@pytest.mark.parametrize("name,polar", [("ion64_es", False), ("water64_polar", True)])
def test_a_trial_that_moves_nothing_costs_nothing_and_returns_the_accepted_totals(name, polar):
    """Trial positions equal to the accepted ones: no kernel runs, the totals are the accepted ones, accept and reject both leave the
    context as it was -- also in between real moves."""
    atoms, basis, opts = util.load_fixture(name)
    if not polar:
        opts = nonpolar(opts)
    S = energy.System(atoms, basis, opts)
    e0 = S.energy()
    obs0 = dict(S.observables)
    a, b = molecules(atoms)[3]
    S.set_profiling(True)
    S.timings(reset=True)
    for verdict in ("accept", "reject"):
        assert S.trial_energy(a, atoms["pos"][a:b]) == e0
        assert S.trial_observables == obs0
        getattr(S, verdict)()
    assert sum(v["launches"] for v in S.timings().values()) == 0  # nothing was launched
    S.set_profiling(False)
    # a real move, then a no-op on top of the NEW accepted state
    trial = atoms["pos"][a:b] + 0.3
    e1 = S.trial_energy(a, trial)
    S.accept()
    assert S.trial_energy(a, trial) == e1
    S.reject()
    pos = atoms["pos"].copy()
    pos[a:b] = trial
    F = energy.System(dict(atoms, pos=pos), basis, opts)
    assert util.close(F.energy(), e1, 1e-11) and util.close(S.energy(), e1, 1e-11)
    S.close()
    F.close()
