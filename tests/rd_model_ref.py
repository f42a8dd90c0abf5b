"""A numpy restatement of the rd model (mpmc_set_rd_model): the pair sum inside the cutoff with the reference's other mixing rules
(System::pair_exclusions, src/System.cpp:1069-1177) and other functions of r / sigma (System::lj src/System.Energy.cpp:897-1032,
lj_buffered_14_7 :1212-1248, dreiding :2098-2215).

Written from the contract, not from the kernels.
  - a pair is excluded when both atoms belong to one molecule, or when either has epsilon = 0 or sigma = 0 and neither carries dispersion
    coefficients; it is frozen when both atoms are; rimg is the minimum-image distance;
  - mixing (sigma >= 0, epsilon >= 0):
      lb   sigma = (s_i + s_j) / 2, 0 when either is 0;                         eps = sqrt(e_i e_j)
      wh   sigma = ((s_i^6 + s_j^6) / 2)^(1/6), 0 when either is 0;             eps = sqrt(e_i e_j) 2 s_i^3 s_j^3 / (s_i^6 + s_j^6) (sqrt(e_i e_j) for sigma = 0)
      hal  sigma = (s_i^3 + s_j^3) / (s_i^2 + s_j^2) when both > 0, else 0;     eps = 4 e_i e_j / (sqrt e_i + sqrt e_j)^2 when both > 0, else 0
      c6   sigma = (s_i + s_j) / 2;                                             eps = 64 sqrt(e_i e_j) s_i^3 s_j^3 / (s_i + s_j)^6, 0 for sigma = 0
  - forms, for a pair that is neither excluded nor frozen:
      lj    rimg - 1e-12 < cutoff:   4 eps (t12 - t6), s = sigma / rimg, t6 = (s s s)^2, t12 = t6^2, + lj_fh_corr(eps, t12, t6) under feynman_hibbs
      b147  not rimg > cutoff:       eps (1.07 / (rho + 0.07))^7 (1.12 / (rho^7 + 0.12) - 2), rho = rimg / sigma
      drd   not rimg > cutoff:       eps (termexp - 2 rho^-6), termexp = exp(12 (1 - rho)), 1e40 for rimg < 0.4 sigma
    a pair with sigma = 0 or eps = 0 contributes 0;
  - lj: lrc_pair = sum of lj_lrc_corr(sigma, eps) over every pair that is not frozen and has eps != 0 and sigma != 0 (excluded pairs too),
    lrc_self over the atoms, rd = (lj_pairs + lrc_pair) + lrc_self;  b147, drd: no corrections, rd = lj_pairs.
"""
from __future__ import annotations

import atexit
import os
import shutil
import tempfile

import numpy as np

from rd_crystal_ref import AMU2KG, HBAR2, HBAR4, KB, KB2, M2A2, M2A4, SMALL_DR, lrc_term
from three_body_ref import min_image

MAXVALUE = 1.0e40
GAMMA = 12.0
FORMS = ("lj", "b147", "drd")   # MPMC_RD_FORM_*
RULES = ("lb", "wh", "hal", "c6")  # MPMC_RD_MIX_*


def model_of(opts):
    """(form, rule) names of a loaded case's options: dreiding wins over lj_buffered_14_7, which does not switch Halgren mixing on"""
    form = "drd" if opts.get("dreiding") else "b147" if opts.get("lj_buffered_14_7") else "lj"
    rule = "wh" if opts.get("waldmanhagler") else "hal" if opts.get("halgren_mixing") else "c6" if opts.get("c6_mixing") else "lb"
    return form, rule


def mix(rule, si, ei, sj, ej):
    """(sigma_ij, eps_ij) of arrays of atom parameters"""
    si, ei, sj, ej = (np.asarray(v, dtype=np.float64) for v in (si, ei, sj, ej))
    zero = (si == 0.0) | (sj == 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        if rule == "wh":
            si3, sj3 = si * si * si, sj * sj * sj
            si6, sj6 = si3 * si3, sj3 * sj3
            sig = np.where(zero, 0.0, np.power(0.5 * (si6 + sj6), 1.0 / 6.0))
            eps = np.where(zero, np.sqrt(ei * ej), np.sqrt(ei * ej) * 2.0 * si3 * sj3 / (si6 + sj6))
        elif rule == "hal":
            sig = np.where((si > 0.0) & (sj > 0.0), (si * si * si + sj * sj * sj) / (si * si + sj * sj), 0.0)
            eps = np.where((ei > 0.0) & (ej > 0.0), 4.0 * ei * ej / np.power(np.sqrt(ei) + np.sqrt(ej), 2), 0.0)
        elif rule == "c6":
            sig = 0.5 * (si + sj)
            eps = np.where(sig != 0.0, 64.0 * np.sqrt(ei * ej) * np.power(si, 3.0) * np.power(sj, 3.0) / np.power(si + sj, 6.0), 0.0)
        else:
            sig = np.where(zero, 0.0, 0.5 * (si + sj))
            eps = np.sqrt(ei * ej)
    return sig, eps


def pair_mag(form, sig, eps, r):
    """the sum of the magnitudes of the two terms the form's function is the difference of (repulsion and attraction), 0 where sigma_ij or
    eps_ij is 0: the scale its rounding error is measured against"""
    sig, eps, r = (np.asarray(v, dtype=np.float64) for v in (sig, eps, r))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if form == "lj":
            sor = sig / r
            t6 = sor * sor * sor
            t6 = t6 * t6
            m = 4.0 * eps * (t6 * t6 + t6)
        elif form == "b147":
            rho = r / sig
            m = eps * np.power(1.07 / (rho + 0.07), 7) * (1.12 / (np.power(rho, 7) + 0.12) + 2.0)
        else:
            rho = r / sig
            m = eps * (np.where(r < 0.4 * sig, MAXVALUE, np.exp(GAMMA * (1.0 - rho)) * (6.0 / (GAMMA - 6.0))) + np.power(rho, -6.0) * (GAMMA / (GAMMA - 6.0)))
    return np.where((sig == 0.0) | (eps == 0.0), 0.0, m)


def pair_energy(form, sig, eps, r, fh=0, temperature=0.0, mi=None, mj=None):
    """the form's function of arrays (sigma_ij, eps_ij, r); 0 where sigma_ij or eps_ij is 0.  fh, temperature, mi, mj: Feynman-Hibbs order,
    temperature and the two molecule masses (lj only)"""
    sig, eps, r = (np.asarray(v, dtype=np.float64) for v in (sig, eps, r))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if form == "lj":
            sor = sig / r  # (the reference's own products, :965-968: sigma / r enters at the twelfth power)
            t6 = sor * sor * sor
            t6 = t6 * t6
            t12 = t6 * t6
            e = 4.0 * eps * (t12 - t6)
            if fh:
                ir = 1.0 / r
                ir2 = ir * ir
                ir3 = ir2 * ir
                ir4 = ir3 * ir
                mu = AMU2KG * mi * mj / (mi + mj)
                dE = -24.0 * eps * (2.0 * t12 - t6) * ir
                d2E = 24.0 * eps * (26.0 * t12 - 7.0 * t6) * ir2
                corr = M2A2 * (HBAR2 / (24.0 * KB * temperature * mu)) * (d2E + 2.0 * dE / r)
                if fh >= 4:
                    d3E = -1344.0 * eps * (6.0 * t12 - t6) * ir3
                    d4E = 12096.0 * eps * (10.0 * t12 - t6) * ir4
                    corr = corr + M2A4 * (HBAR4 / (1152.0 * KB2 * temperature * temperature * mu * mu)) * (15.0 * dE * ir3 + 4.0 * d3E * ir + d4E)
                e = e + corr
        elif form == "b147":
            rho = r / sig
            e = eps * np.power(1.07 / (rho + 0.07), 7) * (1.12 / (np.power(rho, 7) + 0.12) - 2.0)
        else:
            rho = r / sig
            term6 = np.power(rho, -6.0) * (GAMMA / (GAMMA - 6.0))
            termexp = np.where(r < 0.4 * sig, MAXVALUE, np.exp(GAMMA * (1.0 - rho)) * (6.0 / (GAMMA - 6.0)))
            e = eps * (termexp - term6)
    return np.where((sig == 0.0) | (eps == 0.0), 0.0, e)


class Box:
    def __init__(self, atoms, basis, opts, form=None, rule=None):
        from mpmcxx_amd import energy

        f, r = model_of(opts)
        self.form, self.rule = form or f, rule or r
        self.basis = np.asarray(basis, dtype=np.float64).reshape(3, 3)
        recip, self.volume, self.cutoff = energy.pbc_compute(self.basis)
        self.recip = np.asarray(recip, dtype=np.float64).reshape(3, 3)
        self.pos = np.asarray(atoms["pos"], dtype=np.float64).reshape(-1, 3)
        self.sigma = np.asarray(atoms["sigma"], dtype=np.float64)
        self.eps = np.asarray(atoms["epsilon"], dtype=np.float64)
        self.mol = np.asarray(atoms["mol_id"])
        self.frozen = np.asarray(atoms["frozen"]) != 0
        self.null = (self.eps == 0.0) | (self.sigma == 0.0)
        self.disp = np.asarray(atoms["has_disp"]) != 0 if "has_disp" in atoms else np.zeros(len(self.sigma), dtype=bool)
        self.rd_lrc = bool(opts.get("rd_lrc", 1))
        self.fh = (4 if int(opts.get("feynman_hibbs_order") or 0) == 4 else 2) if opts.get("feynman_hibbs") else 0
        self.temperature = float(opts.get("temperature") or 0.0)
        self.molmass = np.zeros(len(self.sigma))
        if self.fh:
            mass = np.asarray(atoms["mass"], dtype=np.float64)
            molmass = {}
            for m, w in zip(self.mol.tolist(), mass.tolist()):
                molmass[m] = molmass.get(m, 0.0) + w
            self.molmass = np.array([molmass[m] for m in self.mol.tolist()])

    def rows(self, i, j, pos_i=None, pos_j=None):
        """(pair energies, pairs kept, pairs inside the LJ test, smallest |rimg - cutoff| / cutoff) of atoms i against atoms j"""
        pi = self.pos[i] if pos_i is None else pos_i
        pj = self.pos[j] if pos_j is None else pos_j
        dm = min_image(self.basis, self.recip, pi - pj)
        rimg = np.sqrt(((dm[..., 0] * dm[..., 0]) + dm[..., 1] * dm[..., 1]) + dm[..., 2] * dm[..., 2])
        excluded = (self.mol[i] == self.mol[j]) | ((self.null[i] | self.null[j]) & ~(self.disp[i] | self.disp[j]))
        allowed = ~excluded & ~(self.frozen[i] & self.frozen[j]) & (i != j)
        lj_in = allowed & (rimg - SMALL_DR < self.cutoff)
        keep = lj_in if self.form == "lj" else allowed & ~(rimg > self.cutoff)
        sig, eps = mix(self.rule, self.sigma[i], self.eps[i], self.sigma[j], self.eps[j])
        e = pair_energy(self.form, sig, eps, rimg, self.fh if self.form == "lj" else 0, self.temperature, self.molmass[i], self.molmass[j])
        e = np.where(keep, e, 0.0)
        gap = np.abs(rimg - self.cutoff) / self.cutoff
        return e, int(np.sum(keep)), int(np.sum(lj_in)), float(np.min(np.where(allowed, gap, np.inf))) if len(i) else np.inf

    def pair_sum(self):
        """(pair sum, sum of the magnitudes of the pair terms, pairs kept, pairs inside the LJ test, smallest relative distance from the cutoff)"""
        n = len(self.pos)
        chunk = max(1, min(512, 4_000_000 // n))
        total, mag, terms, n_lj, gap = 0.0, 0.0, 0, 0, np.inf
        for a in range(0, n, chunk):
            ii = np.arange(a, min(n, a + chunk))
            I, J = np.meshgrid(ii, np.arange(n), indexing="ij")
            sel = J > I
            if not sel.any():
                continue
            e, t, l, g = self.rows(I[sel], J[sel])
            total += float(np.sum(e))
            mag += float(np.sum(np.abs(e)))
            terms += t
            n_lj += l
            gap = min(gap, g)
        return total, mag, terms, n_lj, gap

    def lrc(self):
        """(pair LRC, self LRC): the LJ form's, with the mixed parameters; none under the other forms"""
        if not self.rd_lrc or self.form != "lj":
            return 0.0, 0.0
        n = len(self.pos)
        lp = 0.0
        for a in range(0, n, 512):
            ii = np.arange(a, min(n, a + 512))
            I, J = np.meshgrid(ii, np.arange(n), indexing="ij")
            sel = J > I
            I, J = I[sel], J[sel]
            sig, eps = mix(self.rule, self.sigma[I], self.eps[I], self.sigma[J], self.eps[J])
            t = lrc_term(np.abs(sig), eps, self.cutoff, self.volume)
            lp += float(np.sum(np.where((eps != 0.0) & (sig != 0.0) & ~(self.frozen[I] & self.frozen[J]), t, 0.0)))
        t = lrc_term(np.abs(self.sigma), self.eps, self.cutoff, self.volume)
        self.lrc_self_terms = np.where((self.sigma != 0.0) & (self.eps != 0.0) & ~self.frozen, t, 0.0)
        return lp, float(np.sum(self.lrc_self_terms))

    def delta(self, first, new):
        """(change of the pair sum, sum of the magnitudes of the old and new terms, change of the kept terms) when atoms [first, first + m)
        move to `new`"""
        new = np.asarray(new, dtype=np.float64).reshape(-1, 3)
        m, n = len(new), len(self.pos)
        pos_new = self.pos.copy()
        pos_new[first:first + m] = new
        everyone = np.arange(n)
        d, mag, dterms = 0.0, 0.0, 0
        for t in range(m):
            i = first + t
            j = everyone[~((everyone >= first) & (everyone <= i))]  # (a pair of two moved atoms once)
            ii = np.full(len(j), i)
            eo, to, _, _ = self.rows(ii, j)
            en, tn, _, _ = self.rows(ii, j, pos_new[ii], pos_new[j])
            d += float(np.sum(en - eo))
            mag += float(np.sum(np.abs(eo)) + np.sum(np.abs(en)))
            dterms += tn - to
        return d, mag, dterms


def for_case(atoms, basis, opts, form=None, rule=None):
    """{'lj_pairs', 'mag', 'lrc_pair', 'lrc_self', 'rd', 'n_terms', 'n_lj_in_cutoff', 'gap', 'form', 'rule'} of a loaded case"""
    b = Box(atoms, basis, opts, form, rule)
    e, mag, terms, n_lj, gap = b.pair_sum()
    lp, ls = b.lrc()
    rd = e
    if b.form == "lj" and b.rd_lrc:  # (lj() adds the self terms atom by atom behind the pairs, :1025-1028)
        rd = e + lp
        for t in b.lrc_self_terms.tolist():
            rd += t
    return {"lj_pairs": e, "mag": mag, "lrc_pair": lp, "lrc_self": ls, "rd": rd, "n_terms": terms, "n_lj_in_cutoff": n_lj, "gap": gap,
            "form": b.form, "rule": b.rule}


_BOXES = None


def box_dir() -> str:
    """a temporary directory holding NAME.in / NAME.pqr of every gen_box.RD_MODEL_FIXTURES box (the goldens keep the reference's results only)"""
    global _BOXES
    if _BOXES is None:
        from mpmcxx_amd import gen_box

        _BOXES = tempfile.mkdtemp(prefix="rd_model_boxes_")
        atexit.register(shutil.rmtree, _BOXES, True)
        for name in gen_box.RD_MODEL_FIXTURES:
            gen_box.materialize(name, _BOXES)
    return _BOXES


def load(name: str):
    """(atoms, basis, options) of an rd-model fixture, parsed from its regenerated reference-format files"""
    from mpmcxx_amd import pqr

    return pqr.load_case(os.path.join(box_dir(), f"{name}.in"))


_RESTATED = {}


def restated(name: str):
    """for_case of a fixture, computed once per process and shared by the tests that need it"""
    if name not in _RESTATED:
        _RESTATED[name] = for_case(*load(name))
    return _RESTATED[name]
