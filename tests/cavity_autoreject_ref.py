"""A numpy restatement of cavity_autoreject (mpmc_set_cavity_autoreject): brute-force contact counts with the minimum image.

Written from the contract, not from the kernels.
  - rimg is the minimum-image distance (three_body_ref.min_image: the reference's rounding), sqrt of the sum of squares in x, y, z order;
  - sigma rule: a pair that is neither rd_excluded (same molecule; or epsilon = 0 or sigma = 0 on either atom with no dispersion coefficient on
    either) nor frozen (both atoms frozen), inside the form's distance test (lj: rimg - 1e-12 < cutoff; b147, drd: not rimg > cutoff), with
    rimg < scale * sigma_ij (|sigma_ij| for lj) is REPLACED: its rd_energy is MAXVALUE = 1e40;  lj_pairs = S + n_replaced * 1e40;
  - absolute rule: every pair of atoms of different molecules with rimg < scale counts, excluded or not, whatever the cutoff -- except that
    without polarization a pair of two frozen atoms is never measured: it keeps rimg = 0 and always trips the test (n_unmeasured_frozen);
    any hit adds 1e40 to the value energy() RETURNS, and to nothing else.
  - under `disp_expansion on` the sigma rule is disp_expansion()'s: every pair that is neither rd_excluded nor frozen, with NO cutoff,
    sigma_ij = (s_i + s_j) / 2 (the r0 of the term), and with cavity_autoreject_repulsion != 0 a second test replaces the pair when
    315.775... exp(-eps_ij (rimg - sigma_ij)) > cavity_autoreject_repulsion, eps_ij = 2 e_i e_j / (e_i + e_j) (schmidt_ff:
    (e_i + e_j) e_i e_j / (e_i^2 + e_j^2)); the repulsion is 0 when eps_ij or sigma_ij is 0.
The mixing rules are rd_model_ref.mix (lb, wh, hal, c6); the plain term is (lj, lb) with |sigma|.
"""
from __future__ import annotations

import json
import os

import numpy as np

import rd_model_ref
from three_body_ref import min_image

MAXVALUE = 1.0e40
SMALL_DR = 1.0e-12
SIGMA, ABSOLUTE = 1, 2  # MPMC_AUTOREJECT_*
KEYS = ("cavity_autoreject", "cavity_autoreject_absolute", "cavity_autoreject_scale", "cavity_autoreject_repulsion")


def rules_of(opts):
    """(rules, scale) of the reference keywords in an options dict"""
    on = lambda v: v not in (None, 0, False, "off", "")
    return (SIGMA if on(opts.get("cavity_autoreject")) else 0) | (ABSOLUTE if on(opts.get("cavity_autoreject_absolute")) else 0), \
        float(opts.get("cavity_autoreject_scale") or 0.0)


def without_keys(opts):
    return {k: v for k, v in opts.items() if k not in KEYS}


REPULSION = 315.7750382111558307123944638  # K, System.Energy.cpp:1974


def counts(atoms, basis, opts, rules, scale, pos=None, repulsion=None):
    """{'n_replaced', 'n_absolute', 'n_unmeasured_frozen', 'replaced_pairs', 'absolute_pairs'} of one configuration"""
    from mpmcxx_amd import energy

    form, rule = rd_model_ref.model_of(opts)
    basis = np.asarray(basis, dtype=np.float64).reshape(3, 3)
    recip, _, cutoff = energy.pbc_compute(basis)
    recip = np.asarray(recip, dtype=np.float64).reshape(3, 3)
    pos = np.asarray(atoms["pos"] if pos is None else pos, dtype=np.float64).reshape(-1, 3)
    n = len(pos)
    sigma = np.asarray(atoms["sigma"], dtype=np.float64)
    eps = np.asarray(atoms["epsilon"], dtype=np.float64)
    mol = np.asarray(atoms["mol_id"])
    frozen = np.asarray(atoms["frozen"]) != 0
    null = (eps == 0.0) | (sigma == 0.0)
    disp = np.asarray(atoms["has_disp"]) != 0 if "has_disp" in atoms else np.zeros(n, dtype=bool)
    polar = bool(opts.get("polarization"))
    disp_term = bool(opts.get("disp_expansion"))
    repulsion = float(opts.get("cavity_autoreject_repulsion") or 0.0) if repulsion is None else float(repulsion)
    replaced, absolute = [], []
    for a in range(0, n, 256):
        ii = np.arange(a, min(n, a + 256))
        I, J = np.meshgrid(ii, np.arange(n), indexing="ij")
        sel = J > I
        I, J = I[sel], J[sel]
        dm = min_image(basis, recip, pos[I] - pos[J])
        rimg = np.sqrt(((dm[:, 0] * dm[:, 0]) + dm[:, 1] * dm[:, 1]) + dm[:, 2] * dm[:, 2])
        intra = mol[I] == mol[J]
        both_frozen = frozen[I] & frozen[J]
        if rules & SIGMA:
            excluded = intra | ((null[I] | null[J]) & ~(disp[I] | disp[J]))
            inside = (rimg - SMALL_DR < cutoff) if form == "lj" else ~(rimg > cutoff)
            if disp_term:  # disp_expansion(): no cutoff, sigma as mixed, the repulsion test beside the sigma test
                inside = np.ones(len(I), dtype=bool)
                sij = 0.5 * (sigma[I] + sigma[J])
                if repulsion != 0.0:
                    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                        ei, ej = eps[I], eps[J]
                        eij = (ei + ej) * ei * ej / (ei * ei + ej * ej) if opts.get("schmidt_ff") else 2.0 * ei * ej / (ei + ej)
                        rep = np.where((eij != 0.0) & (sij != 0.0), REPULSION * np.exp(-eij * (rimg - sij)), 0.0)
                else:
                    rep = np.zeros(len(I))
                hit = ~excluded & ~both_frozen & ((rimg < scale * sij) | ((repulsion != 0.0) & (rep > repulsion)))
                replaced += list(zip(I[hit].tolist(), J[hit].tolist()))
            elif form == "lj" and rule == "lb":  # the plain term: |sigma|, 0 when either is 0 and none is negative
                neg = (sigma[I] < 0.0) | (sigma[J] < 0.0)
                sij = np.where(((sigma[I] == 0.0) | (sigma[J] == 0.0)) & ~neg, 0.0, 0.5 * (np.abs(sigma[I]) + np.abs(sigma[J])))
            else:
                sij, _ = rd_model_ref.mix(rule, sigma[I], eps[I], sigma[J], eps[J])
                sij = np.abs(sij) if form == "lj" else sij
            if not disp_term:
                hit = ~excluded & ~both_frozen & inside & (rimg < scale * sij)
                replaced += list(zip(I[hit].tolist(), J[hit].tolist()))
        if rules & ABSOLUTE:
            measured = ~intra & (~both_frozen if not polar else True)
            hit = measured & (rimg < scale)
            absolute += list(zip(I[hit].tolist(), J[hit].tolist()))
    unmeasured = 0
    if (rules & ABSOLUTE) and not polar:
        f = np.nonzero(frozen)[0]
        unmeasured = sum(int(np.sum(mol[f[k + 1:]] != mol[f[k]])) for k in range(len(f)))
    return {"n_replaced": len(replaced), "n_absolute": len(absolute), "n_unmeasured_frozen": unmeasured, "replaced_pairs": replaced,
            "absolute_pairs": absolute}


def penalised(plain, c, form="lj"):
    """the contract's energies from the unpenalised observables `plain` (keys of mpmc_result) and the counts c: lj_pairs = S + n 1e40 in this
    order, rd_energy and energy follow, the absolute penalty is on the returned value alone"""
    r = dict(plain)
    r["lj_pairs"] = plain["lj_pairs"] + float(c["n_replaced"]) * MAXVALUE
    r["rd_energy"] = r["lj_pairs"] if form != "lj" else (r["lj_pairs"] + plain["lrc_pair"]) + plain["lrc_self"]
    r["energy"] = r["rd_energy"] + plain["coulombic_energy"] + plain["polarization_energy"] + plain.get("vdw_energy", 0.0) + plain.get("three_body_energy", 0.0)
    r["absolute_penalty"] = MAXVALUE if c["n_absolute"] + c["n_unmeasured_frozen"] > 0 else 0.0
    r["returned_energy"] = r["energy"] + r["absolute_penalty"]
    return r


# ---- the goldens: tests/golden/autoreject_cases.json (tools/make_autoreject_golden.py) ------------------------------------------------------
def cases():
    import util

    with open(os.path.join(util.GOLDEN, "autoreject_cases.json")) as f:
        return json.load(f)


_LOADED = {}


def load(name):
    """(atoms, basis, options with the case's keywords, the case) -- the box parsed from reference-format files, the keywords from the JSON"""
    import util
    from mpmcxx_amd import pqr

    if name not in _LOADED:
        case = cases()[name]
        if case["box"]:
            atoms, basis, opts = pqr.load_case(os.path.join(util.GOLDEN, case["box"] + ".in"))
        elif os.path.exists(os.path.join(util.GOLDEN, case["base"] + ".in")):
            atoms, basis, opts = util.load_fixture(case["base"])
        elif case["base"].endswith("_disp"):
            import disp_expansion_ref

            atoms, basis, opts = disp_expansion_ref.load(case["base"])
        else:
            atoms, basis, opts = rd_model_ref.load(case["base"])
        opts = dict(opts)
        for k, v in case["options"].items():
            opts[k] = {"on": 1, "off": 0}.get(v, v) if isinstance(v, str) else v
        _LOADED[name] = (atoms, basis, opts, case)
    atoms, basis, opts, case = _LOADED[name]
    return {k: np.array(v) for k, v in atoms.items()}, np.array(basis), dict(opts), case


_COUNTS = {}


def restated(name):
    """counts() of a golden case, computed once per process and shared"""
    if name not in _COUNTS:
        atoms, basis, opts, _ = load(name)
        rules, scale = rules_of(opts)
        _COUNTS[name] = counts(atoms, basis, opts, rules, scale)
    return _COUNTS[name]
