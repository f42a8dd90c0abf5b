"""`rd_crystal on` through the Gibbs-ensemble driver (include/mpmc_gibbs.hpp, examples/gibbs_nvt.cpp) on the HIP path.

tests/golden/gibbs_lj_rc2/ is the two-box input of tests/golden/gibbs_lj with `rd_crystal on`, `rd_crystal_order 2` and 60 steps; its
trajectory.json was made by oracle/_ref/ref_gibbs_traj (the reference's own pick_Gibbs_move / make_move_Gibbs / energy /
boltzmann_factor_NVT_Gibbs / restore, as for the other gibbs_* goldens: `ref_gibbs_traj input.in 60` in that directory).  The run holds
displacements, particle transfers in both directions (the atom lists change, the setting stays) and accepted and rejected volume
exchanges (the image table, the cutoff, the corrections and the self term follow the cell through the C++ facade)."""
import os
import subprocess

import pytest

import util
from test_gibbs_driver import compare, golden, parse

pytestmark = pytest.mark.gpu
NAME = "gibbs_lj_rc2"


def test_gibbs_driver_reproduces_the_reference_made_trajectory(tmp_path):
    from mpmcxx_amd import build as mbuild

    mbuild.build_library()
    lib = os.path.join(util.ROOT, "mpmcxx_amd")
    exe = str(tmp_path / "gibbs_nvt")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-I", os.path.join(util.ROOT, "include"), os.path.join(util.ROOT, "examples", "gibbs_nvt.cpp"),
                           "-L", lib, "-lmpmc_energy", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    ref = golden(NAME)
    out = subprocess.run([exe, os.path.join(util.GOLDEN, NAME, "input.in")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-500:] + out.stderr[-500:]
    kinds = compare(parse(out.stdout), ref, 1e-9, 1e-9)
    moves = {k[0] for k in kinds}
    assert {(2, 2), (0, 1), (1, 0), (5, 5)} <= moves  # displacements, transfers both ways, volume exchanges
    assert ((5, 5), (1, 1)) in kinds and ((5, 5), (0, 0)) in kinds  # a volume exchange accepted and one rejected
    # the term is really on: the plain box's trajectory starts from other energies
    assert ref["initial_energy"] != golden("gibbs_lj")["initial_energy"]
