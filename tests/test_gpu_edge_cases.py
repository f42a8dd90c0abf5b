"""Inputs that stress the geometry bookkeeping of the HIP path against the oracle: unwrapped coordinates, anisotropic cells, boxes far
from the origin, coordinates on a coarse grid (hundreds of pairs exactly on the half-box tie of the minimum image, where the reference's
answer depends on rint's tie rule applied to the RAW displacement), and a cell smaller than one atom tile."""
import numpy as np
import pytest

import util
from mpmcxx_amd import energy

pytestmark = pytest.mark.gpu


def build(case):
    atoms, basis, opts = util.load_fixture("ion1000_polar")
    rng = np.random.default_rng(3)
    a = dict(atoms)
    if case == "unwrapped":
        a["pos"] = atoms["pos"] + rng.integers(-3, 4, size=atoms["pos"].shape) * basis[0, 0]
    elif case == "anisotropic":
        basis = np.diag([40.0, 25.0, 70.0])
        a["pos"] = atoms["pos"] * np.array([1.0, 25 / 40, 70 / 40])
    elif case == "far_from_origin":
        a["pos"] = atoms["pos"] + np.array([1234.5, -987.25, 55.125])
    elif case == "integer_grid_ties":
        a["pos"] = np.round(atoms["pos"], 0)
    elif case == "cell_smaller_than_a_tile":
        basis = np.diag([12.0, 12.0, 12.0])
        a = {k: v[:200] for k, v in atoms.items()}
        a["pos"] = rng.uniform(-6, 6, size=(200, 3))
        a["mol_id"] = np.arange(200, dtype=np.int32)
    return a, basis, opts


def nearest_neighbour_field(a, basis):
    """max |q_j| / d_nn^2: the field of the closest ion, the size of the largest term of any atom's static field in this orthorhombic cell"""
    L = np.diag(basis)
    f = (a["pos"][:, None, :] - a["pos"][None, :, :]) / L
    r = np.linalg.norm((f - np.rint(f)) * L, axis=2)
    np.fill_diagonal(r, np.inf)
    return float(np.abs(a["charge"]).max() / r.min() ** 2)


@pytest.mark.parametrize("solver", ["compact", "matrix_free"])
@pytest.mark.parametrize("case", ["unwrapped", "anisotropic", "far_from_origin", "integer_grid_ties", "cell_smaller_than_a_tile"])
def test_geometry_edge_cases(case, solver):
    a, basis, opts = build(case)
    ref = util.oracle_energy(a, basis, opts)
    S = energy.System(a, basis, dict(opts, solver=solver))
    try:
        S.energy()
        mu = S.dipoles()[0]
        fields = absolute = None
        if case == "integer_grid_ties":
            # the perfect grid cancels the static field almost completely: |E_i| ~ 2e-6 on every ion, against terms up to the nearest
            # neighbour's field q / d_nn^2 ~ 2.6.  What is left of E_i is the rounding residue of ~10^3 such terms (~10^3 x 1.1e-16 of
            # the largest); measured on the MI355X: 1e-14 (5e-9 of |E_i| on 913 of the 1000 ions).  Held at 1e-13 q / d_nn^2 absolute on
            # top of the standard bound.
            # The induced field (|F_i| 2.8e-7 .. 5.0e-7) is a linear function of the static field after the fixed number of iterations,
            # so it inherits E's relative uncertainty: delta_E = 1e-13 q / d_nn^2 / min|E_i| (1.3e-7 here) of max|F|, on top of the
            # standard 1e-9 |F_i|.  Measured on the MI355X: max |d_i| = 1.6e-15, 5e-9 of |F_i| (delta_E max|F| = 6.4e-14).
            # The dipoles keep the global 1e-9 max|mu| + 1e-13 this test held before.
            s_nn = nearest_neighbour_field(a, basis)
            delta_e = 1e-13 * s_nn / float(np.abs(ref["ef_static"]).max(axis=1).min())
            fields = {"mu": (0.0, 1e-9), "ef_induced": (util.REL_TOL, delta_e)}
            absolute = {"ef_static": 1e-13 * s_nn, "mu": 1e-13}
        util.assert_matches_oracle(S.observables, S.dipoles(), ref, a, opts, label=(case, solver), fields=fields, absolute=absolute)
        assert np.abs(mu - ref["mu"]).max() <= 1e-9 * np.abs(ref["mu"]).max() + 1e-13  # (the global bound this test held before, kept)
    finally:
        S.close()
