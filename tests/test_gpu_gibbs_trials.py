"""The Gibbs driver with every move as a device trial (`gibbs_nvt INPUT.in --trials`, GibbsSettings::device_trials): displacements through
energy_trial_async, transfers through energy_trial_insert_async / energy_trial_remove_async, volume exchanges through
energy_trial_volume_async, no energy() after the initial one.  Against the reference-made trajectories of tests/golden/gibbs_* with the
comparison and the 1e-9 of tests/test_gibbs_driver.py: every decision, atom count and volume equal.  (One documented deviation: a rejected
volume trial keeps the accepted bits where the reference's revert leaves a round trip's rounding, 1e-16 relative.)"""
import os
import subprocess

import pytest

import util
from test_gibbs_driver import LIBDIR, compare, golden, parse

pytestmark = pytest.mark.gpu

CASES = ["gibbs_lj", "gibbs_water", "gibbs_water_polar", "gibbs_lj_rc2"]
VOLUME = 5


@pytest.fixture(scope="module")
def gibbs_nvt(tmp_path_factory):
    from mpmcxx_amd import build as mbuild

    mbuild.build_library()
    exe = str(tmp_path_factory.mktemp("gibbs_trials") / "gibbs_nvt")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(util.ROOT, "include"),
                           os.path.join(util.ROOT, "examples", "gibbs_nvt.cpp"), "-L", LIBDIR, "-lmpmc_energy", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib",
                           "-o", exe])
    return exe


def run(exe, name, *flags):
    out = subprocess.run([exe, os.path.join(util.GOLDEN, name, "input.in")] + list(flags), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-500:] + out.stderr[-500:]
    return out.stdout


@pytest.mark.parametrize("name", CASES)
def test_trial_mode_reproduces_the_reference_made_trajectory(gibbs_nvt, name):
    ref = golden(name)
    ours = parse(run(gibbs_nvt, name, "--trials"))
    compare(ours, ref, 1e-9, 1e-9)
    assert ours["energy_calls"] == 2 and ours["device_trials"] == 1  # the initial evaluation of the two boxes and nothing after it
    n_volume = sum(1 for s in ref["steps"] if s["movetype"] == [VOLUME, VOLUME])
    n_volume_accepted = sum(1 for s in ref["steps"] if s["movetype"] == [VOLUME, VOLUME] and s["accepted"] == [1, 1])
    evaluated, accepted, rejected, reject_evaluations = ours["volume_trial_counts"]
    assert n_volume > 0 and (evaluated, accepted, rejected) == (2 * n_volume, 2 * n_volume_accepted, 2 * (n_volume - n_volume_accepted))
    assert reject_evaluations == 0
    n_transfer = sum(1 for s in ref["steps"] if sorted(s["movetype"]) == [0, 1])
    delta, full, _ = ours["exchange_counts"]
    assert n_transfer > 0 and delta + full == 2 * n_transfer
    if name in ("gibbs_lj", "gibbs_water"):  # no polarization, no rd_crystal: every transfer is an O(m N) delta
        assert delta > 0 and full == 0
    else:  # the dipole solve and the lattice sum have no exchange delta
        assert delta == 0


def test_without_the_flag_the_two_modes_decide_alike_and_the_old_path_keeps_its_output(gibbs_nvt):
    plain = parse(run(gibbs_nvt, "gibbs_lj"))
    trials = parse(run(gibbs_nvt, "gibbs_lj", "--trials"))
    assert "device_trials" not in plain and "volume_trial_counts" not in plain and plain["energy_calls"] == 2 * (len(plain["steps"]) + 1)
    assert [(s["movetype"], s["accepted"], s["natoms"], s["N"]) for s in plain["steps"]] == [(s["movetype"], s["accepted"], s["natoms"], s["N"]) for s in trials["steps"]]
    compare(plain, golden("gibbs_lj"), 1e-9, 1e-9)
