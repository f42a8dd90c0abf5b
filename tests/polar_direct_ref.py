"""numpy restatement of the reference's `polar_iterative off` path (System::polar: thole_field, thole_bmatrix, thole_bmatrix_dipoles):
the yardstick of tests/test_polar_direct.py and tests/test_gpu_polar_direct.py.

A is the matrix of thole_amatrix restricted to the polarizable atoms -- 1/alpha on the diagonal, the exponentially damped dipole tensor
off it, all pairs at their minimum image, no cutoff -- assembled here with numpy from the same formulas (`amatrix`; test_polar_direct
holds it to the oracle's orc_thole_amatrix_block block by block); E0 is the oracle's orc_thole_field.  mu = numpy.linalg.solve(A, E0)
plus ONE step of iterative refinement whose residual is accumulated in numpy.longdouble, so that the result carries an error of the order
of eps rather than cond(A) eps.  Atoms with alpha == 0 are left out of the system and get mu = 0 (the reference gives them a diagonal of
1e40 and dipoles of the order 1e-40 E0).
"""
import numpy as np

from oracle import OracleSystem, pbc_update
from three_body_ref import min_image


def minimum_image(pos, basis):
    """d[i, j] = minimum image of pos[i] - pos[j] the reference's way: d - basis^T rint(recip^T d) (System.cpp:1231-1241), each sum in
    the reference's association order (three_body_ref.min_image).  A matrix product leaves the order, and whether the sums are fused,
    to the BLAS: at a half-cell tie of a skewed cell that is another image (test_lattice_tie_preconditions)."""
    R, _, _ = pbc_update(basis)
    b = np.asarray(basis, dtype=np.float64).reshape(3, 3)
    return min_image(b, np.asarray(R, dtype=np.float64).reshape(3, 3), pos[:, None, :] - pos[None, :, :])


def amatrix(atoms, basis, opts, dtype=np.float64):
    """(A of the polarizable atoms [3 n_pol, 3 n_pol], their indices [n_pol]) -- thole_amatrix, System.Energy.cpp:2661-2781"""
    alpha = np.asarray(atoms["polarizability"], dtype=np.float64)
    idx = np.nonzero(alpha != 0.0)[0]
    pos = np.asarray(atoms["pos"], dtype=np.float64).reshape(-1, 3)[idx]
    n = idx.size
    lam = float(opts["polar_damp"])
    d = minimum_image(pos, basis).astype(dtype)
    r2 = (d * d).sum(axis=2)
    r = np.sqrt(r2)
    np.fill_diagonal(r, 1.0)
    ir = 1.0 / r
    ir3 = ir * ir * ir
    ir5 = ir3 * ir * ir
    explr = np.exp(-lam * r)
    damp1 = 1.0 - explr * (0.5 * lam * lam * r * r + lam * r + 1.0)
    damp2 = damp1 - explr * (lam ** 3 * r * r * r / 6.0)
    ta = damp1 * ir3
    tb = 3.0 * damp2 * ir5
    A = -tb[:, :, None, None] * d[:, :, :, None] * d[:, :, None, :]
    for p in range(3):
        A[:, :, p, p] += ta
    off = ~np.eye(n, dtype=bool)
    A = A * off[:, :, None, None]
    for p in range(3):
        A[np.arange(n), np.arange(n), p, p] = 1.0 / alpha[idx].astype(dtype)
    return A.transpose(0, 2, 1, 3).reshape(3 * n, 3 * n), idx


def static_field(atoms, basis, opts):
    """E0 of every atom [n, 3]: the oracle's thole_field (Ewald or no-PBC as the options say)"""
    return OracleSystem(atoms, basis, dict(opts, polar_iterative=1)).thole_field()


def solve(atoms, basis, opts, E0=None):
    """{"mu" [n, 3], "ef_static" [n, 3], "polarization_energy", "residual": max|E0 - A mu| / max|E0| in long double, "A", "idx"}"""
    n = int(np.asarray(atoms["pos"]).reshape(-1, 3).shape[0])
    E0 = static_field(atoms, basis, opts) if E0 is None else np.asarray(E0, dtype=np.float64).reshape(n, 3)
    A, idx = amatrix(atoms, basis, opts)
    mu = np.zeros((n, 3))
    res = 0.0
    if idx.size:
        b = E0[idx].reshape(-1)
        x = np.linalg.solve(A, b)
        Al, bl = A.astype(np.longdouble), b.astype(np.longdouble)
        r = bl - Al @ x.astype(np.longdouble)
        x = x + np.linalg.solve(A, r.astype(np.float64))
        r = bl - Al @ x.astype(np.longdouble)
        res = float(np.abs(r).max() / np.abs(bl).max()) if np.abs(bl).max() > 0 else 0.0
        mu[idx] = x.reshape(-1, 3)
    u = np.float64(-0.5 * (mu.astype(np.longdouble) * E0.astype(np.longdouble)).sum())
    return {"mu": mu, "ef_static": E0, "polarization_energy": float(u), "residual": res, "A": A, "idx": idx}
