"""A numpy restatement of the Axilrod-Teller three-body energy (reference System::axilrod_teller, src/System.Energy.cpp:1653-1770).

Written from the contract, not from the kernels: every unordered triple of distinct atoms that are not all in one molecule, no cutoff,
frozen atoms included; each pair vector is that pair's own minimum image (System::minimum_image, src/System.cpp:1202-1279, with the
reference's association order); the angle at each corner between the two vectors that leave it; the mixing rule and unit factor of
:1685-1709, evaluated with pow() and the reference's divisions.  O(N^3) on the host: for the small golden boxes and for checking GPU results.
"""
from __future__ import annotations

import atexit
import os
import shutil
import tempfile

import numpy as np

A_SCALE = 6.7483345  # alpha -> a.u. (:1693)
UNIT = 0.0032539449 / (3.166811429 * 0.000001)  # hartree bohr^9 -> K A^9 (:1709)


def min_image(basis: np.ndarray, recip: np.ndarray, d: np.ndarray) -> np.ndarray:
    """d = r_i - r_j (any leading shape, last axis 3) -> the minimum-image vector, rounded like the reference (no FMA)."""
    B, R = basis, recip
    img = [np.rint(((R[0, p] * d[..., 0]) + R[1, p] * d[..., 1]) + R[2, p] * d[..., 2]) for p in range(3)]
    out = np.empty_like(d)
    for p in range(3):
        out[..., p] = d[..., p] - (((B[0, p] * img[0]) + B[1, p] * img[1]) + B[2, p] * img[2])
    return out


def atom_c9(alpha: np.ndarray, c6: np.ndarray, c9: np.ndarray, midzuno_kihara: bool) -> np.ndarray:
    if midzuno_kihara:
        return 3.0 / 4.0 * alpha * A_SCALE * c6
    return np.asarray(c9, dtype=np.float64)


def three_body_energy(pos, alpha, mol, c9_atom, basis, recip) -> float:
    """E3 in K.  pos [n][3], alpha [n], mol [n] (equal = same molecule), c9_atom [n] (atom_c9), basis / recip row-major as in mpmc_set_box."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    n = pos.shape[0]
    alpha = np.asarray(alpha, dtype=np.float64)
    mol = np.asarray(mol)
    a = alpha * A_SCALE
    a3 = np.power(a, 3)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv_u = 1.0 / (c9_atom / a3)  # the reference's 1 / (c9_i / a_i^3): infinite for c9_i = 0, NaN for alpha_i = 0 (overridden below)
    D = min_image(np.asarray(basis, dtype=np.float64), np.asarray(recip, dtype=np.float64), pos[:, None, :] - pos[None, :, :])  # D[i, j] = img(r_i - r_j)
    norm = np.sqrt(np.einsum("ijp,ijp->ij", D, D))
    total = 0.0
    for i in range(n - 2):
        j = np.arange(i + 1, n)
        jj, kk = np.meshgrid(j, j, indexing="ij")
        keep = kk > jj
        jj, kk = jj[keep], kk[keep]
        ok = ~((mol[jj] == mol[i]) & (mol[kk] == mol[i]))
        jj, kk = jj[ok], kk[ok]
        if jj.size == 0:
            continue
        ij, ik, jk = D[i, jj], D[i, kk], D[jj, kk]
        rij, rik, rjk = norm[i, jj], norm[i, kk], norm[jj, kk]
        with np.errstate(divide="ignore", invalid="ignore"):
            c9 = np.power(a3[i] * a3[jj] * a3[kk], 1.0 / 3.0) * 3.0 / (inv_u[i] + inv_u[jj] + inv_u[kk])
        c9 = np.where((alpha[i] == 0.0) | (alpha[jj] == 0.0) | (alpha[kk] == 0.0), 0.0, c9) * UNIT
        dot = lambda u, v: np.einsum("tp,tp->t", u, v)
        cos_part = 3.0 * (dot(-ij, -ik) / (rij * rik))  # corner i: the vectors to j and to k
        cos_part = cos_part * (dot(ij, -jk) / (rij * rjk))  # corner j
        cos_part = cos_part * (dot(ik, jk) / (rik * rjk))  # corner k
        total += float(np.sum(c9 * ((1.0 + cos_part) / np.power(rij * rik * rjk, 3))))
    return total


def for_case(atoms, basis, opts, recip=None) -> float:
    """E3 of a loaded case (mpmcxx_amd.pqr.load_case); recip defaults to the reference's own reciprocal basis (mpmc_pbc_compute)."""
    basis = np.asarray(basis, dtype=np.float64)
    if recip is None:
        from mpmcxx_amd import energy

        recip = energy.pbc_compute(basis)[0]
    c9 = atom_c9(atoms["polarizability"], atoms["c6"], atoms["c9"], bool(opts.get("midzuno_kihara_approx")))
    return three_body_energy(atoms["pos"], atoms["polarizability"], atoms["mol_id"], c9, basis, np.asarray(recip, dtype=np.float64).reshape(3, 3))


_BOXES = None


def box_dir() -> str:
    """a temporary directory holding NAME.in / NAME.pqr of every gen_box.THREE_BODY_FIXTURES box: the golden JSON keeps the reference's
    results only, the text is regenerated (gen_box.materialize writes the bytes the reference read)"""
    global _BOXES
    if _BOXES is None:
        from mpmcxx_amd import gen_box

        _BOXES = tempfile.mkdtemp(prefix="three_body_boxes_")
        atexit.register(shutil.rmtree, _BOXES, True)
        for name in gen_box.THREE_BODY_FIXTURES:
            gen_box.materialize(name, _BOXES)
    return _BOXES


def load(name: str):
    """(atoms, basis, options) of a three-body fixture, parsed from its regenerated reference-format files"""
    from mpmcxx_amd import pqr

    return pqr.load_case(os.path.join(box_dir(), f"{name}.in"))
