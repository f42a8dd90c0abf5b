"""A numpy restatement of the dispersion-expansion repulsion/dispersion term (reference System::disp_expansion,
src/System.Energy.cpp:1939-2080; mixing src/System.cpp:1139-1156; exclusions src/System.cpp:1042-1056).

Written from the contract, not from the kernels: every pair that is neither rd_excluded (same molecule, or a null epsilon / sigma with
all six c's 0) nor frozen (both atoms frozen), at its minimum-image distance, with no cutoff:
    315.775 exp(-alpha_ij (r - r0_ij)) [alpha_ij != 0 and r0_ij != 0] - t6 c6_ij / r^6 - t8 c8_ij / r^8 - t10 c10_ij / r^10
with the reference's mixing, unit factors, tt_damping (pow / factorial series, clamp at 1e-9) and expression order.  The pair LRC sums
over every non-frozen pair (excluded ones included), the self LRC over every non-frozen atom with its unconverted coefficients.
All pairs are evaluated in row chunks, so 10 000-atom boxes fit in memory.
"""
from __future__ import annotations

import atexit
import math
import os
import shutil
import tempfile

import numpy as np

from three_body_ref import min_image

REPULSION = 315.7750382111558307123944638
UNIT = 3.166811429 * 0.000001
PI = 3.141592653589793238462643383279502884


def flags(opts):
    return (bool(opts.get("damp_dispersion")), bool(opts.get("extrapolate_disp_coeffs")), bool(opts.get("schmidt_ff")))


def _mix(ai, aj, r0i, r0j, c6i, c6j, c8i, c8j, c10i, c10j, extrapolate, schmidt):
    with np.errstate(divide="ignore", invalid="ignore"):
        r0 = 0.5 * (r0i + r0j)
        alpha = 2.0 * ai * aj / (ai + aj)
        if schmidt:
            alpha = (ai + aj) * ai * aj / (ai * ai + aj * aj)
        c6 = np.sqrt(c6i * c6j) * 0.021958709 / UNIT
        c8 = np.sqrt(c8i * c8j) * 0.0061490647 / UNIT
        if extrapolate:
            c10 = np.where((c6 != 0.0) & (c8 != 0.0), 49.0 / 40.0 * c8 * c8 / c6, 0.0)
        else:
            c10 = np.sqrt(c10i * c10j) * 0.0017219135 / UNIT
    return alpha, r0, c6, c8, c10


def tt_damping(n, br):
    s = np.zeros_like(br)
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(n + 1):
            s = s + np.power(br, i) / float(math.factorial(i))
        res = 1.0 - np.exp(-br) * s
    return np.where(res > 0.000000001, res, 0.0)


def pair_energy(r, alpha, r0, c6, c8, c10, damp):
    """rd_energy of pairs at distance r (arrays), :1951-1992"""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        r2 = r * r
        r4 = r2 * r2
        r6 = r4 * r2
        r8 = r6 * r2
        r10 = r8 * r2
        rep = np.where((alpha != 0.0) & (r0 != 0.0), REPULSION * np.exp(-alpha * (r - r0)), 0.0)
        if damp:
            return -tt_damping(6, alpha * r) * c6 / r6 - tt_damping(8, alpha * r) * c8 / r8 - tt_damping(10, alpha * r) * c10 / r10 + rep
        return -c6 / r6 - c8 / r8 - c10 / r10 + rep


def lrc_term(c6, c8, c10, cutoff, volume):
    rc = cutoff
    return -4.0 * PI * (c6 / (3.0 * rc * rc * rc) + c8 / (5.0 * rc * rc * rc * rc * rc) + c10 / (7.0 * rc * rc * rc * rc * rc * rc * rc)) / volume


class Box:
    """the per-atom columns of a loaded case (mpmcxx_amd.pqr.load_case) and the cell, in the form the sums below take"""

    def __init__(self, atoms, basis, opts):
        from mpmcxx_amd import energy

        self.basis = np.asarray(basis, dtype=np.float64).reshape(3, 3)
        recip, self.volume, self.cutoff = energy.pbc_compute(self.basis)
        self.recip = np.asarray(recip, dtype=np.float64).reshape(3, 3)
        self.pos = np.asarray(atoms["pos"], dtype=np.float64).reshape(-1, 3)
        self.alpha = np.asarray(atoms["epsilon"], dtype=np.float64)
        self.r0 = np.asarray(atoms["sigma"], dtype=np.float64)
        self.c6 = np.asarray(atoms["c6"], dtype=np.float64)
        self.c8 = np.asarray(atoms["c8"], dtype=np.float64)
        self.c10 = np.asarray(atoms["c10"], dtype=np.float64)
        self.mol = np.asarray(atoms["mol_id"])
        self.frozen = np.asarray(atoms["frozen"]) != 0
        self.null = (self.alpha == 0.0) | (self.r0 == 0.0)
        self.disp = (self.c6 != 0.0) | (self.c8 != 0.0) | (self.c10 != 0.0)
        self.damp, self.extrapolate, self.schmidt = flags(opts)
        self.rd_lrc = bool(opts.get("rd_lrc", 1))

    def rows(self, i, j, pos_i=None, pos_j=None):
        """pair terms of atoms i against atoms j (index arrays of one length), 0 where the exclusions drop the pair"""
        pi = self.pos[i] if pos_i is None else pos_i
        pj = self.pos[j] if pos_j is None else pos_j
        d = min_image(self.basis, self.recip, pi - pj)
        r = np.sqrt(((d[..., 0] * d[..., 0]) + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
        alpha, r0, c6, c8, c10 = _mix(self.alpha[i], self.alpha[j], self.r0[i], self.r0[j], self.c6[i], self.c6[j], self.c8[i], self.c8[j],
                                      self.c10[i], self.c10[j], self.extrapolate, self.schmidt)
        e = pair_energy(r, alpha, r0, c6, c8, c10, self.damp)
        excluded = (self.mol[i] == self.mol[j]) | ((self.null[i] | self.null[j]) & ~(self.disp[i] | self.disp[j]))
        keep = ~excluded & ~(self.frozen[i] & self.frozen[j]) & (i != j)
        return np.where(keep, e, 0.0)

    def pair_sum(self, chunk=256):
        """(sum of the pair terms, sum of their magnitudes) over all unordered pairs"""
        n = len(self.pos)
        total, mag = 0.0, 0.0
        for a in range(0, n, chunk):
            ii = np.arange(a, min(n, a + chunk))
            I, J = np.meshgrid(ii, np.arange(n), indexing="ij")
            sel = J > I
            e = self.rows(I[sel], J[sel])
            total += float(np.sum(e))
            mag += float(np.sum(np.abs(e)))
        return total, mag

    def lrc(self):
        """(pair LRC, self LRC)"""
        if not self.rd_lrc:
            return 0.0, 0.0
        n = len(self.pos)
        lp = 0.0
        for a in range(0, n, 512):
            ii = np.arange(a, min(n, a + 512))
            I, J = np.meshgrid(ii, np.arange(n), indexing="ij")
            sel = J > I
            I, J = I[sel], J[sel]
            _, _, c6, c8, c10 = _mix(self.alpha[I], self.alpha[J], self.r0[I], self.r0[J], self.c6[I], self.c6[J], self.c8[I], self.c8[J],
                                     self.c10[I], self.c10[J], self.extrapolate, self.schmidt)
            t = lrc_term(c6, c8, c10, self.cutoff, self.volume)
            lp += float(np.sum(np.where(self.frozen[I] & self.frozen[J], 0.0, t)))
        c10 = self.c10
        if self.extrapolate:
            with np.errstate(divide="ignore", invalid="ignore"):
                c10 = np.where((self.c6 != 0.0) & (self.c8 != 0.0), 49.0 / 40.0 * self.c8 * self.c8 / self.c6, 0.0)
        ls = float(np.sum(np.where(self.frozen, 0.0, lrc_term(self.c6, self.c8, c10, self.cutoff, self.volume))))
        return lp, ls

    def delta(self, first, new):
        """(change of the pair sum when atoms [first, first + m) move to `new`, sum of the magnitudes of the old and new terms)"""
        new = np.asarray(new, dtype=np.float64).reshape(-1, 3)
        m = len(new)
        n = len(self.pos)
        pos_new = self.pos.copy()
        pos_new[first:first + m] = new
        everyone = np.arange(n)
        d, mag = 0.0, 0.0
        for t in range(m):
            i = first + t
            j = everyone[~((everyone >= first) & (everyone <= i))]  # (a pair of two moved atoms once)
            ii = np.full(len(j), i)
            eo = self.rows(ii, j)
            en = self.rows(ii, j, pos_new[ii], pos_new[j])
            d += float(np.sum(en - eo))
            mag += float(np.sum(np.abs(eo)) + np.sum(np.abs(en)))
        return d, mag


def for_case(atoms, basis, opts):
    """{'lj_pairs', 'lrc_pair', 'lrc_self', 'rd', 'mag'} of a loaded case"""
    b = Box(atoms, basis, opts)
    e, mag = b.pair_sum()
    lp, ls = b.lrc()
    return {"lj_pairs": e, "lrc_pair": lp, "lrc_self": ls, "rd": (e + lp) + ls, "mag": mag}


_BOXES = None


def box_dir() -> str:
    """a temporary directory holding NAME.in / NAME.pqr of every gen_box.DISP_FIXTURES box (the goldens keep the reference's results only)"""
    global _BOXES
    if _BOXES is None:
        from mpmcxx_amd import gen_box

        _BOXES = tempfile.mkdtemp(prefix="disp_boxes_")
        atexit.register(shutil.rmtree, _BOXES, True)
        for name in gen_box.DISP_FIXTURES:
            gen_box.materialize(name, _BOXES)
    return _BOXES


def load(name: str):
    """(atoms, basis, options) of a disp-expansion fixture, parsed from its regenerated reference-format files"""
    from mpmcxx_amd import pqr

    return pqr.load_case(os.path.join(box_dir(), f"{name}.in"))
