"""Arbitrary-precision references of the pair functions, point by point (no device, no import of the library's GPU side).

Every energy of the library is a sum of functions of one distance.  This module restates those functions from the reference's formulas
(the ones oracle/mpmc_oracle.c and tests/*_ref.py restate in fp64) in mpmath at 50 digits, and builds the grids the scans walk:
tests/test_pair_scan_ref.py holds the references to the fp64 restatements on the CPU, tests/test_gpu_pair_scans.py holds the kernels to the
references on the device.

A point value is (ref, scale): `ref` the value at 50 digits, `scale` the sum of the ABSOLUTE values of the terms the formula adds, so that a
zero crossing (LJ, Silvera-Goldman) or a cancellation (the erf form) does not inflate a relative error.  Predicates (cutoff tests, x < RM,
r < 0.4 sigma) are taken in fp64 exactly as the reference takes them: they decide which formula applies, they are not values.
Where the reference's expression is odd on purpose (Silvera-Goldman's 110 C10 / x^10 in V'', the FH Coulomb term that carries no charges)
the reference is restated, not the textbook.

k-space sums run in numpy.longdouble where it has a 64-bit mantissa (eps <= 1.1e-19), in mpmath on every 8th point otherwise.
"""
from __future__ import annotations

import mpmath as mp
import numpy as np

mp.mp.dps = 50
M = mp.mpf

B_DEFAULT = 1e-12  # the margin the README and test_gpu_parity_margin claim for the HIP path
TABLE_PIECES, TABLE_H = 512, 1.0 / 128.0  # csrc/erfc_table.inc: alpha r in [0, 4) in pieces of 1 / 128
LONGDOUBLE_OK = bool(np.finfo(np.longdouble).eps <= 1.1e-19)

# reference constants.h, as the doubles the reference holds
HBAR2, HBAR4, KB, KB2 = 1.11211999e-68, 1.23681087e-136, 1.3806503e-23, 1.90619525e-46
M2A2, M2A4, AMU2KG = 1.0e20, 1.0e40, 1.66053873e-27
PI = mp.pi
SQRT_PI = mp.sqrt(mp.pi)


class Terms:
    """a sum of terms and the sum of their magnitudes"""

    def __init__(self):
        self.v, self.s = M(0), M(0)

    def add(self, *ts):
        for t in ts:
            self.v += t
            self.s += abs(t)
        return self

    def pair(self):
        return self.v, self.s


# An fp64 computation whose terms pass below the smallest normal double loses up to all of 2.2e-308 there (gradual underflow, or a flush),
# which is eps times 1.0e-292: no scale counts below that, so exp(-1849) is held to "0 or next to it" and not to its 300th digit.
UNDERFLOW_SCALE = M(2.2250738585072014e-308) / M(2.220446049250313e-16)


def err(value, ref, scale):
    """|value - ref| / scale at 50 digits (0 / 0 = 0: a term that is identically zero must be exactly 0.0)"""
    d = abs(M(float(value)) - ref)
    if scale == 0:
        return 0.0 if d == 0 else float("inf")
    return float(d / (scale + UNDERFLOW_SCALE))


# ---- the pair functions ---------------------------------------------------------------------------------------------------------------------
def lj(r, sigma_i, eps_i, sigma_j, eps_j, fh_order=0, temperature=0.0, mass_i=0.0, mass_j=0.0):
    """System::lj :965-999 with Lorentz-Berthelot mixing: 4 eps (s^12 - s^6) [+ lj_fh_corr :1100-1148]"""
    r = M(r)
    sig, eps = (M(sigma_i) + M(sigma_j)) / 2, mp.sqrt(M(eps_i) * M(eps_j))
    t6 = (sig / r) ** 6
    t12 = t6 * t6
    T = Terms().add(4 * eps * t12, -4 * eps * t6)
    if fh_order:
        mu = M(AMU2KG) * M(mass_i) * M(mass_j) / (M(mass_i) + M(mass_j))
        k2 = M(M2A2) * (M(HBAR2) / (24 * M(KB) * M(temperature) * mu))
        ir = 1 / r
        # d2E + 2 dE / r, dE = -24 eps (2 t12 - t6) / r, d2E = 24 eps (26 t12 - 7 t6) / r^2
        T.add(k2 * 24 * eps * 26 * t12 * ir**2, -k2 * 24 * eps * 7 * t6 * ir**2, -k2 * 48 * eps * 2 * t12 * ir**2, k2 * 48 * eps * t6 * ir**2)
        if fh_order >= 4:
            k4 = M(M2A4) * (M(HBAR4) / (1152 * M(KB2) * M(temperature) ** 2 * mu**2))
            # 15 dE / r^3 + 4 d3E / r + d4E, d3E = -1344 eps (6 t12 - t6) / r^3, d4E = 12096 eps (10 t12 - t6) / r^4
            T.add(-k4 * 15 * 24 * eps * 2 * t12 * ir**4, k4 * 15 * 24 * eps * t6 * ir**4, -k4 * 4 * 1344 * eps * 6 * t12 * ir**4, k4 * 4 * 1344 * eps * t6 * ir**4,
                  k4 * 12096 * eps * 10 * t12 * ir**4, -k4 * 12096 * eps * t6 * ir**4)
    return T.pair()


def es_real(r, qi, qj, alpha, intra=False, fh_order=0, temperature=0.0, mass_i=0.0, mass_j=0.0):
    """coulombic_real :1490-1510: q_i q_j erfc(alpha r) / r [+ coulombic_real_FH :1521-1557, which carries no charges], or for a pair inside
    a molecule -q_i q_j erf(alpha r) / r"""
    r, a, qq = M(r), M(alpha), M(qi) * M(qj)
    if intra:
        return Terms().add(-qq * mp.erf(a * r) / r).pair()
    ec, g = mp.erfc(a * r), mp.exp(-a * a * r * r)
    T = Terms().add(qq * ec / r)
    if fh_order:
        mu = M(AMU2KG) * M(mass_i) * M(mass_j) / (M(mass_i) + M(mass_j))
        k2 = M(M2A2) * (M(HBAR2) / (24 * M(KB) * M(temperature) * mu))
        ir = 1 / r
        a3 = a**3
        # d2u + 2 du / r: du = -2 a g / (r sqrt pi) - erfc / r^2, d2u = 4 / sqrt pi g (a^3 + 1 / r^2) + 2 erfc / r^3
        T.add(k2 * 4 / SQRT_PI * g * a3, k2 * 4 / SQRT_PI * g * ir**2, k2 * 2 * ec * ir**3, -k2 * 4 * a * g * ir**2 / SQRT_PI, -k2 * 2 * ec * ir**3)
        if fh_order >= 4:
            k4 = M(M2A4) * (M(HBAR4) / (1152 * (M(KB) * M(KB) * M(temperature) ** 2 * mu**2)))
            gs = g / SQRT_PI
            # 15 du / r^3
            T.add(-k4 * 15 * 2 * a * gs * ir**4, -k4 * 15 * ec * ir**5)
            # 4 d3u / r, d3u = g / sqrt pi (-8 a^5 r - 8 a^3 / r - 12 a / r^3) - 6 erfc / r^4
            T.add(-k4 * 4 * gs * 8 * a**5, -k4 * 4 * gs * 8 * a3 * ir**2, -k4 * 4 * gs * 12 * a * ir**4, -k4 * 4 * 6 * ec * ir**5)
            # d4u = g / sqrt pi (8 a^5 + 16 a^7 r^2 + 32 a^3 / r^2 + 48 / r^4) + 24 erfc / r^5
            T.add(k4 * gs * 8 * a**5, k4 * gs * 16 * a**7 * r * r, k4 * gs * 32 * a3 * ir**2, k4 * gs * 48 * ir**4, k4 * 24 * ec * ir**5)
    return T.pair()


def wolf(r, qi, qj, alpha, cutoff):
    """coulombic_wolf :1443: q_i q_j (1 / r - erf(alpha R) / R - (R - r) / R^2)"""
    r, R, qq = M(r), M(cutoff), M(qi) * M(qj)
    return Terms().add(qq / r, -qq * mp.erf(M(alpha) * R) / R, -qq * (R - r) / (R * R)).pair()


def field_real_factor(r, alpha, intra=False):
    """real_term :2919-2934: (2 alpha r / sqrt(pi) exp(-alpha^2 r^2) + erfc(alpha r)) / r^3, the erf form (g - erf) / r^3 inside a molecule"""
    r, a = M(r), M(alpha)
    g = 2 * a / SQRT_PI * mp.exp(-a * a * r * r) * r
    return Terms().add(g / r**3, (-mp.erf(a * r) if intra else mp.erfc(a * r)) / r**3).pair()


SG = dict(ALPHA=1.713, BETA=1.5671, GAMMA=0.00993, C6=12.14, C8=215.2, C10=4813.9, C9=143.1, RM=8.321, BOHR=0.529177249, HARTREE=3.15774655e5,
          HBAR=1.054571e-34)


def sg(r, fh=False, temperature=0.0, mass=0.0):
    """System::sg :1805-1860 for one pair inside the cutoff, in K"""
    c = {k: M(v) for k, v in SG.items()}
    x = M(r) / c["BOHR"]
    below = (r / SG["BOHR"]) < SG["RM"]  # the reference's predicate, in fp64
    rep = mp.exp(c["ALPHA"] - c["BETA"] * x - c["GAMMA"] * x * x)
    ex = mp.exp(-((c["RM"] / x - 1) ** 2)) if below else M(1)
    m6, m8, m10, m9 = c["C6"] / x**6, c["C8"] / x**8, c["C10"] / x**10, -c["C9"] / x**9
    T = Terms().add(rep, -m6 * ex, -m8 * ex, -m10 * ex, -m9 * ex)
    if fh:
        mult = m6 + m8 + m10 + m9
        rr = c["RM"] / x
        t1 = (rr * rr - rr) / x
        t2 = (3 * rr * rr - 2 * rr) / (x * x)
        bg = c["BETA"] + 2 * c["GAMMA"] * x
        k = M(M2A2) * (c["HBAR"] * c["HBAR"] / (24 * M(KB) * M(temperature) * (M(AMU2KG) * M(mass))))
        d1 = [-bg * rep, 6 * c["C6"] / x**7 * ex, 8 * c["C8"] / x**9 * ex, -9 * c["C9"] / x**10 * ex, 10 * c["C10"] / x**11 * ex, -2 * mult * ex * t1]
        d2 = [bg * bg * rep, -2 * c["GAMMA"] * rep, -ex * 42 * c["C6"] / x**8, -ex * 72 * c["C8"] / x**10, ex * 90 * c["C9"] / x**11,
              -ex * 110 * c["C10"] / x**10,  # (x^10, as the reference writes it)
              ex * t1 * 12 * c["C6"] / x**7, ex * t1 * 16 * c["C8"] / x**9, -ex * t1 * 18 * c["C9"] / x**10, ex * t1 * 20 * c["C10"] / x**11,
              ex * t1 * t1 * 4 * mult, ex * t2 * 2 * mult]
        T.add(*[k * t for t in d2], *[k * 2 * t / x for t in d1])
    v, s = T.pair()
    return v * c["HARTREE"], s * c["HARTREE"]


def rd_mix(rule, si, ei, sj, ej):
    """pair_exclusions :1069-1177: the mixed (sigma, epsilon) of two atoms with positive parameters"""
    si, ei, sj, ej = M(si), M(ei), M(sj), M(ej)
    if rule == "wh":
        s6 = (si**6 + sj**6) / 2
        return s6 ** (M(1) / 6), mp.sqrt(ei * ej) * si**3 * sj**3 / s6
    if rule == "hal":
        return (si**3 + sj**3) / (si**2 + sj**2), 4 * ei * ej / (mp.sqrt(ei) + mp.sqrt(ej)) ** 2
    if rule == "c6":
        return (si + sj) / 2, 64 * mp.sqrt(ei * ej) * si**3 * sj**3 / (si + sj) ** 6
    return (si + sj) / 2, mp.sqrt(ei * ej)


def rd_model(form, rule, r, si, ei, sj, ej, sig64=None):
    """lj :965-993, lj_buffered_14_7 :1230-1233, dreiding :2129-2145 with the mixed parameters.  sig64: the fp64 mixed sigma, for DREIDING's
    r < 0.4 sigma predicate"""
    sig, eps = rd_mix(rule, si, ei, sj, ej)
    r64, r = r, M(r)
    if form == "lj":
        t6 = (sig / r) ** 6
        return Terms().add(4 * eps * t6 * t6, -4 * eps * t6).pair()
    rho = r / sig
    if form == "b147":
        a7 = (M(1.07) / (rho + M(0.07))) ** 7
        return Terms().add(eps * a7 * M(1.12) / (rho**7 + M(0.12)), -2 * eps * a7).pair()
    inner = r64 < 0.4 * (float(sig) if sig64 is None else sig64)
    texp = M(1.0e40) if inner else M(6) / 6 * mp.exp(12 * (1 - rho))
    return Terms().add(eps * texp, -eps * 2 / rho**6).pair()


# ---- k-space --------------------------------------------------------------------------------------------------------------------------------
def k_vectors(kmax):
    """the reference's half-space enumeration (coulombic_reciprocal :1577-1583, recip_term :2849-2854): l0 in [0, kmax], l1 from -kmax unless
    l0 = 0, l2 from -kmax unless l0 = l1 = 0 (then from 1), |l|^2 <= kmax^2.  (n, 3) int64; kmax <= 0 enumerates nothing"""
    out = []
    for l0 in range(0, kmax + 1):
        for l1 in range(-kmax if l0 else 0, kmax + 1):
            for l2 in range(-kmax if (l0 or l1) else 1, kmax + 1):
                if l0 * l0 + l1 * l1 + l2 * l2 <= kmax * kmax:
                    out.append((l0, l1, l2))
    return np.array(out, dtype=np.int64).reshape(-1, 3)


def recip_basis(basis):
    """PeriodicBoundary::compute_reciprocal in long double: (reciprocal[p][q], volume)"""
    b = np.asarray(basis, dtype=np.longdouble).reshape(3, 3)
    vol = b[0, 0] * (b[1, 1] * b[2, 2] - b[1, 2] * b[2, 1]) + b[0, 1] * (b[1, 2] * b[2, 0] - b[1, 0] * b[2, 2]) + b[0, 2] * (b[1, 0] * b[2, 1] - b[1, 1] * b[2, 0])
    R = np.array([[b[1, 1] * b[2, 2] - b[1, 2] * b[2, 1], b[0, 2] * b[2, 1] - b[0, 1] * b[2, 2], b[0, 1] * b[1, 2] - b[0, 2] * b[1, 1]],
                  [b[1, 2] * b[2, 0] - b[1, 0] * b[2, 2], b[0, 0] * b[2, 2] - b[0, 2] * b[2, 0], b[0, 2] * b[1, 0] - b[0, 0] * b[1, 2]],
                  [b[1, 0] * b[2, 1] - b[1, 1] * b[2, 0], b[0, 1] * b[2, 0] - b[0, 0] * b[2, 1], b[0, 0] * b[1, 1] - b[0, 1] * b[1, 0]]], dtype=np.longdouble) / vol
    return R, vol


def recip_longdouble(pos, charge, basis, alpha, kmax, field_alpha=None):
    """coulombic_reciprocal :1561-1622 and recip_term :2834-2896 in numpy.longdouble: {"es_recip": (ref, scale), "field": ((n, 3) ref, (n, 3)
    scale)}.  The phase of an atom is k . pos with the atom's own position (1000 cells out included: that is what the reference sums)"""
    ld = np.longdouble
    pos, q = np.asarray(pos, dtype=ld).reshape(-1, 3), np.asarray(charge, dtype=ld)
    R, vol = recip_basis(basis)
    pi = ld(mp.nstr(mp.pi, 25))
    L = k_vectors(kmax).astype(ld)
    n = len(q)
    if not len(L):
        return {"es_recip": (ld(0), ld(0)), "field": (np.zeros((n, 3), ld), np.zeros((n, 3), ld))}
    K = 2 * pi * (L @ R.T)  # k[p] = 2 pi sum_q recip[p][q] l[q]
    k2 = (K * K).sum(axis=1)
    # cos and sin of k . pos = 2 pi sum_q l_q (sum_p recip[p][q] pos_p), as products of one factor per axis (each factor evaluated directly
    # at l_q times the axis' angle: (2 kmax + 1) 3 n evaluations instead of one per k-vector and atom; three roundings more per phase)
    ang = 2 * pi * (pos @ R)  # (n, 3)
    li = np.arange(-kmax, kmax + 1).astype(ld)
    fc = [np.cos(li[:, None] * ang[None, :, ax]) for ax in range(3)]  # (2 kmax + 1, n) per axis
    fs = [np.sin(li[:, None] * ang[None, :, ax]) for ax in range(3)]
    ix = k_vectors(kmax) + kmax
    c01 = fc[0][ix[:, 0]] * fc[1][ix[:, 1]] - fs[0][ix[:, 0]] * fs[1][ix[:, 1]]
    s01 = fs[0][ix[:, 0]] * fc[1][ix[:, 1]] + fc[0][ix[:, 0]] * fs[1][ix[:, 1]]
    c = c01 * fc[2][ix[:, 2]] - s01 * fs[2][ix[:, 2]]  # (nk, n)
    s = s01 * fc[2][ix[:, 2]] + c01 * fs[2][ix[:, 2]]
    f1, f2 = (c * q).sum(axis=1), (s * q).sum(axis=1)
    a = ld(alpha)
    w = np.exp(-k2 / (4 * a * a)) / k2
    e = (w * (f1 * f1 + f2 * f2)).sum() * 4 * pi / vol
    qa = np.abs(q).sum()  # a phase factor counts with its amplitude: the rounding of k . r moves sin and cos by ulp(k . r), whatever their values
    e_scale = (w * qa * qa).sum() * 4 * pi / vol
    fa = a if field_alpha is None else ld(field_alpha)
    kw = K / k2[:, None] * np.exp(-k2 / (4 * fa * fa))[:, None]  # (nk, 3)
    t = s * f1[:, None] - c * f2[:, None]  # (nk, n)
    F = (t.T @ kw) * 8 * pi / vol
    Fs = np.tile(np.abs(kw).sum(axis=0) * qa, (n, 1)) * 8 * pi / vol
    return {"es_recip": (e, e_scale), "field": (F, Fs)}


def recip_mp(pos, charge, basis, alpha, kmax, field_alpha=None):
    """recip()'s sums term by term in mpmath, for machines whose long double is a double"""
    b = mp.matrix(np.asarray(basis, dtype=np.float64).reshape(3, 3).tolist())
    vol = mp.det(b)
    R = b**-1  # the reference's reciprocal_basis
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3).tolist()
    q = [M(float(v)) for v in np.asarray(charge, dtype=np.float64)]
    n = len(q)
    fa = M(alpha if field_alpha is None else field_alpha)
    T, S, qabs = M(0), M(0), sum(abs(v) for v in q)
    F, Fs = [[M(0)] * 3 for _ in range(n)], [[M(0)] * 3 for _ in range(n)]
    for l in k_vectors(kmax).tolist():
        k = [2 * PI * sum(R[p, q_] * l[q_] for q_ in range(3)) for p in range(3)]
        k2 = sum(x * x for x in k)
        ph = [sum(k[d] * M(p[d]) for d in range(3)) for p in pos]
        c, s = [mp.cos(x) for x in ph], [mp.sin(x) for x in ph]
        f1, f2 = sum(qa * ca for qa, ca in zip(q, c)), sum(qa * sa for qa, sa in zip(q, s))
        w = mp.exp(-k2 / (4 * M(alpha) ** 2)) / k2
        T, S = T + w * (f1 * f1 + f2 * f2), S + w * qabs * qabs
        kw = [k[d] / k2 * mp.exp(-k2 / (4 * fa * fa)) for d in range(3)]
        for a in range(n):
            for d in range(3):
                F[a][d] += kw[d] * (s[a] * f1 - c[a] * f2)
                Fs[a][d] += abs(kw[d]) * qabs
    e = 4 * PI / vol
    f = 8 * PI / vol
    return {"es_recip": (T * e, S * e), "field": ([[v * f for v in row] for row in F], [[v * f for v in row] for row in Fs])}


# ---- grids ----------------------------------------------------------------------------------------------------------------------------------
REST_R = 5.0  # where the moved atom of a trial scan rests: a point of every grid


def both_sides(x, inside_only=False):
    """the doubles 1 ulp and 1e-9 relative on either side of the branch point x"""
    pts = [float(np.nextafter(x, 0.0)), x * (1.0 - 1e-9)]
    if not inside_only:
        pts += [float(np.nextafter(x, np.inf)), x * (1.0 + 1e-9), float(x)]
    return pts


def piece_boundaries(alpha, lo, hi):
    """every boundary x = j / 128 of the erfc table as distances: the two doubles on either side of r = j / (128 alpha), and the piece midpoint"""
    pts = []
    for j in range(1, TABLE_PIECES):
        exact = M(j) / (128 * M(alpha))
        f = float(exact)
        below = f if M(f) < exact else float(np.nextafter(f, 0.0))  # (a double ON the boundary belongs to the upper piece)
        above = float(np.nextafter(below, np.inf))
        pts += [below, above, float((M(j) + M(1) / 2) / (128 * M(alpha)))]
    return [p for p in pts if lo <= p < hi]


def half_integer_points(arg, lo, hi, max_points=64):
    """distances r in [lo, hi) where arg(r) log2(e) is within 1e-12 of a half-integer (where exp_fast's rint switches): arg is monotonic on
    the interval; found by bisection at 50 digits, the nearest double and its two neighbours are returned"""
    log2e = 1 / mp.log(2)
    a, b = arg(M(lo)) * log2e, arg(M(hi)) * log2e
    first, last = int(mp.floor(min(a, b))), int(mp.ceil(max(a, b)))
    targets = [m + M(1) / 2 for m in range(first, last) if min(a, b) < m + M(1) / 2 < max(a, b)]
    if len(targets) > max_points:
        targets = targets[:: max(1, len(targets) // max_points)]
    pts = []
    for t in targets:
        r = _bisect(lambda x: arg(x) * log2e - t, M(lo), M(hi))
        f = float(r)
        pts += [float(np.nextafter(f, 0.0)), f, float(np.nextafter(f, np.inf))]
    return [p for p in pts if lo <= p < hi]


def _bisect(f, a, b):
    fa = f(a)
    for _ in range(140):
        m = (a + b) / 2
        fm = f(m)
        if (fm > 0) == (fa > 0):
            a, fa = m, fm
        else:
            b = m
    return (a + b) / 2


def make_grid(lo, cutoff, n_log=400, seed=0, alpha=None, exp_args=(), branch_points=(), past_cutoff=True):
    """the distances of one scan, sorted and without duplicates:
    n_log log-spaced from lo to the cutoff; 200 seeded random ones; with `alpha` every piece boundary of the erfc table (piece_boundaries);
    for every monotonic exponent in exp_args its half-integer points; both sides (1 ulp, 1e-9 relative) of the cutoff and of every branch point"""
    rng = np.random.default_rng(seed)
    inside = float(np.nextafter(cutoff, 0.0))
    pts = list(np.geomspace(lo, inside, n_log)) + list(rng.uniform(lo, inside, 200))
    if alpha is not None:
        pts += piece_boundaries(alpha, lo, cutoff)
    for arg in exp_args:
        pts += half_integer_points(arg, lo, inside)
    pts += both_sides(cutoff, inside_only=not past_cutoff)
    if lo <= REST_R < cutoff:
        pts.append(REST_R)
    for bp in branch_points:
        if lo < bp < cutoff:
            pts += both_sides(bp)
    pts = sorted({float(p) for p in pts if p >= lo})
    return np.array(pts, dtype=np.float64)


# ---- the scans' boxes -----------------------------------------------------------------------------------------------------------------------
BOX_L = 24.0
CUBIC = np.diag([BOX_L, BOX_L, BOX_L]).astype(np.float64)
TRICLINIC = BOX_L * np.array([[1.0, 0.0, 0.0], [0.13, 1.0, 0.0], [-0.09, 0.18, 1.0]])
CUTOFF = 12.0  # half the shortest lattice vector of either cell
Q, SIGMA, EPS, MASS = (36.5, -44.25), (3.1, 2.7), (40.0, 65.0), (2.016, 2.016)


def cell(name):
    return CUBIC if name == "cubic" else TRICLINIC


def pair_atoms(r, intra=False, charge=Q, sigma=SIGMA, eps=EPS, mass=MASS, polarizability=(0.0, 0.0)):
    """atom 0 at the origin, atom 1 at (r, 0, 0): the distance is the double r itself in either cell (fractional (r / L, 0, 0), no image)"""
    return {"pos": np.array([[0.0, 0.0, 0.0], [float(r), 0.0, 0.0]]), "charge": np.array(charge, dtype=np.float64),
            "polarizability": np.array(polarizability, dtype=np.float64), "epsilon": np.array(eps, dtype=np.float64),
            "sigma": np.array(sigma, dtype=np.float64), "mass": np.array(mass, dtype=np.float64),
            "mol_id": np.array([0, 0] if intra else [0, 1], dtype=np.int32), "frozen": np.zeros(2, np.int32), "has_disp": np.zeros(2, np.int32)}


def in_lj(r, cutoff=CUTOFF):
    return (r - 1.0e-12) < cutoff  # lj :934


def in_es(r, cutoff=CUTOFF):
    return not (r > cutoff)  # coulombic_real :1490, real_term :2917


ALPHAS = {"default": 3.5 / CUTOFF,  # update_pbc, reference System.cpp:871-874
          "table_end": 3.99 / CUTOFF}  # the last pieces of the sweep's table (alpha r < 4)
POLAR_DAMP = 2.1304
POLARIZABILITY = (1.6411, 0.9)


def options(alpha="default", polar_alpha=None, fh_order=0, temperature=0.0, polar=False, wolf=False, kmax=7, polar_ewald=1, max_iter=1, **more):
    """the options of a scan's context (and of the oracle's system)"""
    o = {"rd_only": 0, "rd_lrc": 1, "polarization": int(polar), "polar_iterative": int(polar), "polar_ewald": int(polar and polar_ewald), "polar_max_iter": max_iter,
         "polar_gs": 0, "polar_rrms": 0, "ewald_kmax": kmax, "polar_precision": 0.0, "polar_gamma": 1.0, "polar_damp": POLAR_DAMP if polar else 0.0,
         "damp_type": "exponential" if polar else None, "ewald_alpha": None if alpha == "default" else ALPHAS[alpha],
         "polar_ewald_alpha": None if polar_alpha is None else float(polar_alpha), "wolf": int(wolf), "feynman_hibbs": int(bool(fh_order)),
         "feynman_hibbs_order": fh_order, "temperature": temperature}
    o.update(more)
    return o


def oracle_system(atoms, basis, opts):
    import util  # noqa: F401  (puts oracle/ on the path)
    from oracle import OracleSystem

    return OracleSystem(atoms, basis, opts)


def geometry(atoms, basis, i=0, j=1):
    """(rimg, dimg, r) of a pair as the reference's minimum_image gives them in fp64: the geometry decides WHICH distance the pair function
    sees (a pair pushed past half a lattice vector comes back as its image), it is not part of the function"""
    rimg, d, r = oracle_system(atoms, basis, options()).minimum_image(i, j)
    return float(rimg), np.array(d, dtype=np.float64), float(r)


def ewald_point(rimg, r, alpha, intra=False, fh_order=0, temperature=0.0, cutoff=CUTOFF):
    """{"lj_pairs", "es_real", "field_factor"}: (ref, scale) of the ion pair at the image distance rimg (plain distance r)"""
    zero = (M(0), M(0))
    out = {"lj_pairs": zero, "es_real": zero, "field_factor": zero}
    if not intra and in_lj(rimg, cutoff):
        out["lj_pairs"] = lj(rimg, SIGMA[0], EPS[0], SIGMA[1], EPS[1], fh_order, temperature, MASS[0], MASS[1])
    if intra:
        out["es_real"] = es_real(r, Q[0], Q[1], alpha, intra=True)  # (:1503: the plain distance, no cutoff)
    elif in_es(rimg, cutoff):
        out["es_real"] = es_real(rimg, Q[0], Q[1], alpha, False, fh_order, temperature, MASS[0], MASS[1])
    if in_es(rimg, cutoff) and rimg != 0.0:
        out["field_factor"] = field_real_factor(rimg, alpha, intra)
    return out


def ewald_grid(alpha, lo=0.8, seed=1):
    """the real-space scans' distances: the pieces' boundaries, the half-integer points of exp(-alpha^2 r^2), both sides of the cutoff"""
    return make_grid(lo, CUTOFF, n_log=120, seed=seed, alpha=alpha, exp_args=[lambda x: -(M(alpha) * x) ** 2])


def fh_grid(alpha, lo=0.8, seed=3):
    return make_grid(lo, CUTOFF, n_log=300, seed=seed, exp_args=[lambda x: -(M(alpha) * x) ** 2])


def sg_grid(lo=0.3, seed=2):
    c = SG
    return make_grid(lo, CUTOFF, n_log=500, seed=seed, exp_args=[lambda x: M(c["ALPHA"]) - M(c["BETA"]) * (x / M(c["BOHR"])) - M(c["GAMMA"]) * (x / M(c["BOHR"])) ** 2],
                     branch_points=[c["RM"] * c["BOHR"]], past_cutoff=True)


def thin(grid, n):
    """at most n points of a grid, keeping its first and last ones"""
    if len(grid) <= n:
        return grid
    idx = np.unique(np.round(np.linspace(0, len(grid) - 1, n)).astype(int))
    return grid[idx]


def ld_to_mp(x):
    """a long double as an mpf, exactly"""
    hi = float(x)
    return M(hi) + M(float(x - np.longdouble(hi)))


class Scan:
    """One scan: its points and, per observable, the 50-digit values, their scales, the fp64 restatement's values and the bound B (a number,
    or one per point).  check() is the assertion of every scan: e_gpu <= max(B, 4 e_cpu) at every point."""

    def __init__(self, name, points):
        self.name, self.points = name, list(points)
        self.ref, self.scale, self.cpu, self.bound, self.extra = {}, {}, {}, {}, {}

    def put(self, key, ref_scale, cpu, bound=None):
        self.ref.setdefault(key, []).append(ref_scale[0])
        self.scale.setdefault(key, []).append(ref_scale[1])
        self.cpu.setdefault(key, []).append(float(cpu))
        if bound is not None:
            self.bound.setdefault(key, []).append(bound)

    def keys(self):
        return list(self.ref)

    def e_cpu(self, key):
        return np.array([err(c, r, s) for c, r, s in zip(self.cpu[key], self.ref[key], self.scale[key])])

    def bounds(self, key):
        return self.bound.get(key) or [B_DEFAULT] * len(self.points)

    def share_within(self, key):
        """the share of the points where e_cpu <= B / 4: the 4 e_cpu branch of check() must not swallow a scan"""
        e, b = self.e_cpu(key), np.array(self.bounds(key))
        return float((e <= b / 4.0).mean())

    def check(self, key, gpu, label="", index=None):
        """gpu: the device's values at the points (or at points[index]).  Returns (points, max e_gpu, max e_cpu, point of max e_gpu)"""
        idx = range(len(self.points)) if index is None else index
        assert len(gpu) == len(idx), (label, len(gpu), len(idx))
        worst, worst_cpu, where, bad = 0.0, 0.0, None, []
        bounds = self.bounds(key)
        for g, k in zip(gpu, idx):
            eg, ec = err(g, self.ref[key][k], self.scale[key][k]), err(self.cpu[key][k], self.ref[key][k], self.scale[key][k])
            if eg > worst or where is None:
                worst, where = eg, self.points[k]
            worst_cpu = max(worst_cpu, ec)
            if not eg <= max(bounds[k], 4.0 * ec):
                bad.append((self.points[k], eg, ec, bounds[k]))
        print(f"SCAN|{self.name}|{label}|{key}|{len(idx)}|{worst:.3e}|{worst_cpu:.3e}|{where!r}")
        assert not bad, (f"{self.name} {label} {key}: {len(bad)} of {len(idx)} points beyond max(B, 4 e_cpu); worst (point, e_gpu, e_cpu, B) "
                         f"{max(bad, key=lambda t: t[1])}")
        return len(idx), worst, worst_cpu, where


_SCANS = {}


def cached(fn):
    """one computation of a scan per process: the references are shared by every test that walks the scan, and never changed"""
    def wrapper(*a):
        key = (fn.__name__,) + a
        if key not in _SCANS:
            _SCANS[key] = fn(*a)
        return _SCANS[key]
    wrapper.__name__ = fn.__name__
    return wrapper


# ---- (a), (b), (c): the ion pair under Ewald ------------------------------------------------------------------------------------------------------
@cached
def ewald_scan(alpha_name, intra, cellname, fh_order=0, temperature=0.0):
    """lj_pairs and es_real of the ion pair over ewald_grid (fh_grid under Feynman-Hibbs)"""
    alpha = ALPHAS[alpha_name]
    grid = fh_grid(alpha) if fh_order else ewald_grid(alpha)
    sc = Scan(f"ewald[{alpha_name},{'intra' if intra else 'inter'},{cellname},fh{fh_order}@{temperature:g}]", grid)
    opts = options(alpha_name, fh_order=fh_order, temperature=temperature)
    for r in grid:
        atoms = pair_atoms(r, intra)
        rimg, _, rr = geometry(atoms, cell(cellname))
        o = ewald_point(rimg, rr, alpha, intra, fh_order, temperature)
        c = oracle_system(atoms, cell(cellname), opts).energy(False)
        sc.put("lj_pairs", o["lj_pairs"], c["lj_pairs"])
        sc.put("es_real", o["es_real"], c["es_real"])
    sc.extra["opts"] = opts
    return sc


FIELD_KEYS = [f"E{i}{c}" for i in (0, 1) for c in "xyz"]


def sweep_field_bound(x):
    """the table's pinned host bounds on the field factor (tests/test_erfc_table.py): 5e-13 for alpha r < 2, 1e-10 up to 4"""
    return 5e-13 if x < 2.0 else 1e-10


def recip(pos, charge, basis, alpha, kmax, field_alpha=None):
    """the k-space sums as mpf values: {"es_recip": (ref, scale), "field": (ref, scale) as (n, 3) nested lists}; summed in long double, or
    (where a long double is a double) term by term in mpmath: callers thin their grids to every 8th point then"""
    if not LONGDOUBLE_OK:
        return recip_mp(pos, charge, basis, alpha, kmax, field_alpha)
    k = recip_longdouble(pos, charge, basis, alpha, kmax, field_alpha)
    conv = lambda A: [[ld_to_mp(v) for v in row] for row in A]
    return {"es_recip": (ld_to_mp(k["es_recip"][0]), ld_to_mp(k["es_recip"][1])), "field": (conv(k["field"][0]), conv(k["field"][1]))}


def field_rows(atoms, basis, alpha, field_alpha, kmax, rows, sweep=False, k=None):
    """the static field under polar_ewald on the atoms `rows`: {(i, c): (ref, scale, B)}.  real_term :2900-2940 at 50 digits over the pairs of
    atom i (the reference's fp64 minimum image says which distance each pair function sees) plus recip_term in long double.  The scale of a
    component is that of its real-space terms plus that of its k-space terms.  Under `sweep` B is the table's pinned bound (sweep_field_bound)
    on the real-space share of the scale, plus 1e-12 of the whole for the arithmetic around the table."""
    osys = oracle_system(atoms, basis, options())
    q, mol, n = atoms["charge"], atoms["mol_id"], len(atoms["charge"])
    if k is None:
        k = recip(atoms["pos"], q, basis, alpha, kmax, field_alpha)["field"]
    out = {}
    for i in rows:
        v, s, tb = [M(0)] * 3, [M(0)] * 3, [M(0)] * 3
        for j in range(n):
            if j == i:
                continue
            rimg, d, _ = osys.minimum_image(i, j)  # d = r_i - r_j
            if rimg > CUTOFF or rimg == 0.0:
                continue
            f, fs = field_real_factor(rimg, field_alpha, intra=bool(mol[i] == mol[j]) or q[i] == 0.0 or q[j] == 0.0)
            for c in range(3):
                w = M(float(q[j])) * M(float(d[c]))
                v[c] += f * w
                s[c] += fs * abs(w)
                tb[c] += sweep_field_bound(field_alpha * rimg) * abs(f * w)
        for c in range(3):
            tot_s = s[c] + k[1][i][c]
            b = float((tb[c] + M(B_DEFAULT) * tot_s) / tot_s) if (sweep and tot_s != 0) else B_DEFAULT
            out[(i, c)] = (v[c] + k[0][i][c], tot_s, b)
    return out


@cached
def field_scan(alpha_name, intra, cellname, polar_alpha=None, sweep=False):
    """both rows of the static field of the polarizable ion pair under polar_ewald over ewald_grid"""
    alpha = ALPHAS[alpha_name]
    fa = ALPHAS["default"] if polar_alpha is None else polar_alpha  # (update_pbc defaults each alpha on its own)
    grid = ewald_grid(alpha)
    if not LONGDOUBLE_OK:
        grid = grid[::8]
    sc = Scan(f"field[{alpha_name},{'intra' if intra else 'inter'},{cellname},pa={polar_alpha}{',sweep' if sweep else ''}]", grid)
    opts = options(alpha_name, polar_alpha=polar_alpha, polar=True)
    basis = cell(cellname)
    for r in grid:
        atoms = pair_atoms(r, intra, polarizability=POLARIZABILITY)
        rows = field_rows(atoms, basis, alpha, fa, 7, (0, 1), sweep)
        cpu = oracle_system(atoms, basis, opts).thole_field()
        for i in (0, 1):
            for c in range(3):
                ref, scale, b = rows[(i, c)]
                sc.put(FIELD_KEYS[3 * i + c], (ref, scale), cpu[i, c], b)
    sc.extra["opts"] = opts
    return sc


# ---- (d) Wolf -------------------------------------------------------------------------------------------------------------------------------------
@cached
def wolf_scan(cellname):
    """coulombic_energy of the ion pair under wolf = 1: pairs with rimg < cutoff (strict)"""
    alpha = ALPHAS["default"]
    grid = make_grid(0.8, CUTOFF, n_log=300, seed=4)
    sc = Scan(f"wolf[{cellname}]", grid)
    opts = options(wolf=True)
    for r in grid:
        atoms = pair_atoms(r)
        rimg, _, _ = geometry(atoms, cell(cellname))
        o = wolf(rimg, Q[0], Q[1], alpha, CUTOFF) if rimg < CUTOFF else (M(0), M(0))
        sc.put("coulombic_energy", o, oracle_system(atoms, cell(cellname), opts).energy(False)["coulombic_energy"])
    sc.extra["opts"] = opts
    return sc


# ---- (f) the other rd terms -----------------------------------------------------------------------------------------------------------------------
def h2_pair(r, mass=(2.016, 2.016)):
    a = pair_atoms(r, charge=(0.0, 0.0), sigma=(2.96, 2.96), eps=(34.2, 34.2), mass=mass)
    return a


@cached
def sg_scan(fh, temperature=0.0):
    """rd_energy of two H2 sites under `sg`, 0.3 A to the cutoff: pairs with rimg < cutoff (strict); FH takes the first atom's molecule mass"""
    import sg_ref

    grid = sg_grid()
    sc = Scan(f"sg[fh{int(fh)}@{temperature:g}]", grid)
    for r in grid:
        rimg, _, _ = geometry(h2_pair(r), CUBIC)
        if rimg < CUTOFF:
            sc.put("rd_energy", sg(rimg, bool(fh), temperature, MASS[0]), sg_ref.pair_energy(rimg, bool(fh), temperature, MASS[0]))
        else:
            sc.put("rd_energy", (M(0), M(0)), 0.0)
    sc.extra["opts"] = {"sg": 1, "feynman_hibbs": int(fh), "temperature": temperature}
    return sc


RD_FORMS = {"lj": "lj", "b147": "lj_buffered_14_7", "drd": "dreiding"}
RD_RULES = {"lb": "lb", "wh": "waldmanhagler", "hal": "halgren_mixing", "c6": "c6_mixing"}


@cached
def rd_model_scan(form, rule):
    """lj_pairs of the pair (unequal sigmas and epsilons) under every form x mixing rule of set_rd_model"""
    import rd_model_ref

    sig64, eps64 = (float(v) for v in rd_model_ref.mix(rule, SIGMA[0], EPS[0], SIGMA[1], EPS[1]))
    exp_args, branch = [], []
    if form == "drd":
        exp_args, branch = [lambda x: 12 * (1 - x / M(sig64))], [0.4 * sig64]
    grid = make_grid(0.8, CUTOFF, n_log=300, seed=5, exp_args=exp_args, branch_points=branch)
    sc = Scan(f"rd_model[{form},{rule}]", grid)
    for r in grid:
        rimg, _, _ = geometry(pair_atoms(r), CUBIC)
        keep = in_lj(rimg) if form == "lj" else in_es(rimg)
        if keep:
            sc.put("lj_pairs", rd_model(form, rule, rimg, SIGMA[0], EPS[0], SIGMA[1], EPS[1], sig64), float(rd_model_ref.pair_energy(form, sig64, eps64, rimg)))
        else:
            sc.put("lj_pairs", (M(0), M(0)), 0.0)
    sc.extra["opts"] = options(rd_only=1)
    return sc


# ---- (g) reciprocal space ---------------------------------------------------------------------------------------------------------------------------
KMAXES = (0, 1, 7, 15, 16)  # (15 and 16 lie on either side of kRecipTabMaxK)


def recip_positions(n_atoms, cellname, unwrapped, n_points=64, seed=6):
    """n_points configurations of n_atoms charges: fractional coordinates in [-1/2, 1/2)^3, and under `unwrapped` every atom moved by a lattice
    vector of its own: up to +-1 cell per axis in the first configuration, up to +-1000 in the last (a phase of 1e4 rad costs the fp64
    restatement itself 1e-12 rad; with the three k-vectors of kmax = 1 nothing averages that out)"""
    rng = np.random.default_rng(seed + 17 * n_atoms + (1 if unwrapped else 0))
    basis = cell(cellname)
    out = []
    for p in range(n_points):
        f = rng.uniform(-0.5, 0.5, size=(n_atoms, 3))
        if unwrapped:
            reach = int(round(10.0 ** (3.0 * p / (n_points - 1))))  # 1 .. 1000 cells, log-spaced over the configurations
            f = f + rng.integers(-reach, reach + 1, size=(n_atoms, 3))
        out.append(f @ basis)
    return out


def recip_atoms(pos):
    n = len(pos)
    q = np.where(np.arange(n) % 2 == 0, Q[0], Q[1]).astype(np.float64)
    q[-1] = -q[:-1].sum() if n > 2 else q[-1]
    return {"pos": np.array(pos, dtype=np.float64), "charge": q, "polarizability": np.full(n, POLARIZABILITY[0]), "epsilon": np.full(n, EPS[0]),
            "sigma": np.full(n, SIGMA[0]), "mass": np.full(n, MASS[0]), "mol_id": np.arange(n, dtype=np.int32), "frozen": np.zeros(n, np.int32),
            "has_disp": np.zeros(n, np.int32)}


@cached
def recip_scan(n_atoms, kmax, cellname, unwrapped):
    """es_recip and the static field (real_term + recip_term) on atom 0 and on the last atom, of n_atoms polarizable charges at 64
    configurations; with kmax = 0 the k-space sums have no term at all"""
    poss = recip_positions(n_atoms, cellname, unwrapped)
    if not LONGDOUBLE_OK:
        poss = poss[::8]
    sc = Scan(f"recip[n={n_atoms},kmax={kmax},{cellname},{'unwrapped' if unwrapped else 'in cell'}]", range(len(poss)))
    opts = options(kmax=kmax, polar=True)
    basis = cell(cellname)
    alpha = ALPHAS["default"]
    rows = (0, n_atoms - 1)
    for pos in poss:
        atoms = recip_atoms(pos)
        k = recip(atoms["pos"], atoms["charge"], basis, alpha, kmax)
        osys = oracle_system(atoms, basis, opts)
        sc.put("es_recip", k["es_recip"], oracle_system(atoms, basis, options(kmax=kmax)).energy(False)["es_recip"])
        fr = field_rows(atoms, basis, alpha, alpha, kmax, rows, k=k["field"])
        cpu = osys.thole_field()
        for t, i in enumerate(rows):
            for c in range(3):
                ref, scale, b = fr[(i, c)]
                sc.put(FIELD_KEYS[3 * t + c], (ref, scale), cpu[i, c], b)
    sc.extra["opts"], sc.extra["positions"], sc.extra["rows"] = opts, poss, rows
    return sc


# ---- (a) 65 ions: the pair in an off-diagonal tile pair ---------------------------------------------------------------------------------------------
def line_atoms(t=0.0):
    """64 ions on a jittered 4 x 4 x 4 lattice of the cubic cell (one tile) and a 65th (the second tile's only atom) on the line that passes
    atom 0 at 0.9 A: pos_0 + (t, 0.9, 0)"""
    rng = np.random.default_rng(11)
    g = np.stack(np.meshgrid(*[np.arange(4)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    pos = (g + 0.5) * (BOX_L / 4) - BOX_L / 2 + rng.uniform(-0.4, 0.4, size=(64, 3))
    pos = np.vstack([pos, pos[0] + np.array([t, 0.9, 0.0])])
    n = 65
    q = np.where(g.sum(axis=1) % 2 == 0, Q[0], Q[1]).astype(np.float64)
    q = np.append(q, -q.sum() if q.sum() != 0 else Q[1])
    return {"pos": pos, "charge": q, "polarizability": np.zeros(n), "epsilon": np.where(np.arange(n) % 2 == 0, EPS[0], EPS[1]).astype(np.float64),
            "sigma": np.where(np.arange(n) % 3 == 0, SIGMA[0], SIGMA[1]).astype(np.float64), "mass": np.full(n, MASS[0]),
            "mol_id": np.arange(n, dtype=np.int32), "frozen": np.zeros(n, np.int32), "has_disp": np.zeros(n, np.int32)}


def _pair_sums(atoms, osys, i, js, alpha):
    """(lj_pairs, es_real) Terms of the pairs (i, j in js), each at the reference's fp64 image distance"""
    L, E = Terms(), Terms()
    for j in js:
        rimg, _, _ = osys.minimum_image(i, j)
        if in_lj(rimg):
            v, s = lj(rimg, atoms["sigma"][i], atoms["epsilon"][i], atoms["sigma"][j], atoms["epsilon"][j])
            L.v, L.s = L.v + v, L.s + s
        if in_es(rimg):
            v, s = es_real(rimg, atoms["charge"][i], atoms["charge"][j], alpha)
            E.v, E.s = E.v + v, E.s + s
    return L, E


@cached
def line_scan():
    """lj_pairs and es_real of the 65 ions while atom 64 moves on its line, 300 points: the sum over the 64 fillers' pairs once, the moving
    atom's 64 pairs at every point, all at 50 digits"""
    alpha = ALPHAS["default"]
    ts = np.linspace(-6.0, 6.0, 300)
    sc = Scan("line[65 ions]", ts)
    opts = options()
    base = line_atoms()
    osys = oracle_system(base, CUBIC, opts)
    FL, FE = Terms(), Terms()
    for i in range(63):
        l, e = _pair_sums(base, osys, i, range(i + 1, 64), alpha)
        FL.v, FL.s, FE.v, FE.s = FL.v + l.v, FL.s + l.s, FE.v + e.v, FE.s + e.s
    for t in ts:
        atoms = line_atoms(t)
        osys = oracle_system(atoms, CUBIC, opts)
        l, e = _pair_sums(atoms, osys, 64, range(64), alpha)
        c = osys.energy(False)
        sc.put("lj_pairs", (FL.v + l.v, FL.s + l.s), c["lj_pairs"])
        sc.put("es_real", (FE.v + e.v, FE.s + e.s), c["es_real"])
    sc.extra["opts"] = opts
    return sc


# ---- (f) disp_expansion -----------------------------------------------------------------------------------------------------------------------------
DISP = {"alpha": (1.9, 2.3), "r0": (3.1, 2.7), "c6": (12.0, 17.5), "c8": (210.0, 160.0), "c10": (3900.0, 5200.0)}
DISP_UNIT = 3.166811429 * 0.000001
DISP_K = (0.021958709 / DISP_UNIT, 0.0061490647 / DISP_UNIT, 0.0017219135 / DISP_UNIT)
DISP_REPULSION = 315.7750382111558307123944638


def disp_pair(r, damp, schmidt, extrapolate):
    """disp_expansion :1939-2053 for the pair of DISP: -sum f_n c_n / r^n + 315.775 exp(-alpha (r - r0)), Tang-Toennies f_n under `damp`
    (0 unless > 1e-9), mixing System.cpp:1139-1156 (c_n = sqrt(c_n,i c_n,j) in K A^n, c10 = 49 / 40 c8^2 / c6 under `extrapolate`)"""
    ai, aj = M(DISP["alpha"][0]), M(DISP["alpha"][1])
    alpha = ((ai + aj) * ai * aj / (ai * ai + aj * aj)) if schmidt else 2 * ai * aj / (ai + aj)
    r0 = (M(DISP["r0"][0]) + M(DISP["r0"][1])) / 2
    c = [mp.sqrt(M(DISP[k][0]) * M(DISP[k][1])) * M(kk) for k, kk in zip(("c6", "c8", "c10"), DISP_K)]
    if extrapolate:
        c[2] = M(49) / 40 * c[1] * c[1] / c[0]
    r = M(r)
    T = Terms().add(M(DISP_REPULSION) * mp.exp(-alpha * (r - r0)))
    for n, cn in zip((6, 8, 10), c):
        if damp:
            x = alpha * r
            ser = [x**i / mp.factorial(i) for i in range(n + 1)]
            f = 1 - mp.exp(-x) * sum(ser)
            if not f > M("1e-9"):
                continue
            T.add(-cn / r**n)
            T.add(*[mp.exp(-x) * t * cn / r**n for t in ser])
        else:
            T.add(-cn / r**n)
    return T.pair()


def disp_atoms(r):
    a = pair_atoms(r, charge=(0.0, 0.0), sigma=DISP["r0"], eps=DISP["alpha"])
    return a


DISP_FLAGS = [(d, s, e) for d in (False, True) for s in (False, True) for e in (False, True)]


@cached
def disp_scan(damp, schmidt, extrapolate):
    """lj_pairs of the pair under disp_expansion with every flag combination, 0.8 A to past half the cell (the term has no cutoff)"""
    import disp_expansion_ref as D

    alpha64 = float(D._mix(*[np.float64(v) for k in ("alpha", "r0", "c6", "c8", "c10") for v in DISP[k]], extrapolate, schmidt)[0])
    grid = make_grid(0.8, CUTOFF, n_log=300, seed=7, exp_args=[lambda x: -M(alpha64) * x])
    sc = Scan(f"disp_expansion[damp={int(damp)},schmidt={int(schmidt)},extrapolate={int(extrapolate)}]", grid)
    for r in grid:
        rimg, _, _ = geometry(disp_atoms(r), CUBIC)
        mixed = D._mix(*[np.float64(v) for k in ("alpha", "r0", "c6", "c8", "c10") for v in DISP[k]], extrapolate, schmidt)
        sc.put("lj_pairs", disp_pair(rimg, damp, schmidt, extrapolate), float(D.pair_energy(np.float64(rimg), *mixed, damp)))
    sc.extra["opts"] = options(rd_only=1, rd_lrc=0)
    return sc


# ---- (e) the Thole tensor: dipoles of a polarizable pair under the no-PBC static field ------------------------------------------------------------
THOLE_BASIS = np.diag([40.0, 40.0, 40.0]).astype(np.float64)  # cutoff 20 A: lambda r = 35 lies inside it, no pair ever comes back as an image
THOLE_ALPHA = (0.4, 0.3)  # sqrt(a_0 a_1) |T| <= 0.35 lambda^3 / 6 = 0.56 at every distance: Jacobi converges, the direct system is positive definite
THOLE_MODES = ("compact", "matrix_free", "dense", "gs", "direct")
THOLE_ITERS = (1, 2, 10)


def thole_far_x():
    """kTholeFarX of csrc/kernels.h: lambda r beyond which the kernels drop the damping"""
    import re

    import util

    found = re.findall(r"\bkTholeFarX\s*=\s*([0-9.]+)\s*;", util.csrc_text("kernels.h"))
    assert len(found) == 1, found
    return float(found[0])


def thole_grid():
    """lambda r from 0.01 to 35: log-spaced and random distances, the half-integer points of exp(-lambda r), both sides (1 ulp, 1e-9) of
    lambda r = kTholeFarX"""
    lam = POLAR_DAMP
    return make_grid(0.01 / lam, 35.0 / lam, n_log=300, seed=8, exp_args=[lambda x: -M(lam) * x], branch_points=[thole_far_x() / lam], past_cutoff=False)


def thole_options(mode, max_iter):
    return options(polar=True, polar_ewald=0, max_iter=max_iter, polar_gs=int(mode == "gs"), polar_iterative=int(mode != "direct"),
                   solver="auto" if mode in ("gs", "direct") else mode)


def thole_atoms(r):
    return pair_atoms(r, polarizability=THOLE_ALPHA)


def thole_xx(r):
    """(T_xx, scale) of thole_amatrix :2731-2757 for a pair on the x axis: damp1 / r^3 - 3 x^2 damp2 / r^5"""
    r, l = M(r), M(POLAR_DAMP)
    e = mp.exp(-l * r)
    d1 = [M(1), -e * l * l * r * r / 2, -e * l * r, -e]
    d2 = d1 + [-e * l**3 * r**3 / 6]
    return Terms().add(*[t / r**3 for t in d1], *[-3 * t / r**3 for t in d2]).pair()


def thole_dipoles(r, mode, max_iter):
    """{"mu0x", "mu1x"}: (ref, scale) after max_iter iterations of thole_iterative :3450-3543 (Jacobi, or Gauss-Seidel in list order), or the
    solution of A mu = E for the direct solve; E = thole_field_nopbc :3300-3333.  The scale of a dipole carries the scales of what it is made of"""
    rr = M(r)
    a = [M(THOLE_ALPHA[0]), M(THOLE_ALPHA[1])]
    E = [-M(Q[1]) / (rr * rr), M(Q[0]) / (rr * rr)]  # E_0 = q_1 d / r^3, E_1 = -q_0 d / r^3, d = r_0 - r_1 = (-r, 0, 0)
    T, Ts = thole_xx(r)
    if mode == "direct":
        det, dets = 1 / (a[0] * a[1]) - T * T, 1 / (a[0] * a[1]) + T * T
        out = []
        for i in (0, 1):
            num = [E[i] / a[1 - i], -T * E[1 - i]]
            v = (num[0] + num[1]) / det
            s = (abs(num[0]) + abs(num[1]) + Ts * abs(E[1 - i])) / abs(det) + abs(v) * (dets + 2 * abs(T) * Ts) / abs(det)
            out.append((v, s))
        return {"mu0x": out[0], "mu1x": out[1]}
    mu = [a[i] * E[i] for i in (0, 1)]
    ms = [abs(v) for v in mu]
    for _ in range(max_iter):
        new, news = list(mu), list(ms)
        for i in (0, 1):
            src, srcs = (new, news) if (mode == "gs" and i == 1) else (mu, ms)
            new[i] = a[i] * (E[i] - T * src[1 - i])
            news[i] = a[i] * (abs(E[i]) + Ts * abs(src[1 - i]) + abs(T) * srcs[1 - i])
        mu, ms = new, news
    return {"mu0x": (mu[0], ms[0]), "mu1x": (mu[1], ms[1])}


@cached
def thole_scan(mode, max_iter):
    """the dipoles' x components over thole_grid; B = 1e-12, and 1e-9 from lambda r = kTholeFarX on (the dropped damping is 4.7e-10 by
    design, csrc/kernels.h; tests/test_gpu_edge_cases.py pins that allowance)"""
    grid = thole_grid()
    far = thole_far_x()
    sc = Scan(f"thole[{mode},{max_iter}]", grid)
    opts = thole_options(mode, max_iter)
    for r in grid:
        atoms = thole_atoms(r)
        ref = thole_dipoles(r, mode, max_iter)
        osys = oracle_system(atoms, THOLE_BASIS, dict(opts, polar_iterative=1))
        if mode == "direct":  # the fp64 solution of the 2 x 2 system of the x components, from the restatement's own field and tensor
            E, T = osys.thole_field()[:, 0], osys.amatrix_block(0, 1)[0]
            a0, a1 = THOLE_ALPHA
            det = 1.0 / (a0 * a1) - T * T
            cpu = [(E[0] / a1 - T * E[1]) / det, (E[1] / a0 - T * E[0]) / det]
        else:
            cpu = osys.energy()["mu"][:, 0]
        b = 1e-9 if POLAR_DAMP * r >= far else B_DEFAULT
        sc.put("mu0x", ref["mu0x"], cpu[0], b)
        sc.put("mu1x", ref["mu1x"], cpu[1], b)
    sc.extra["opts"] = opts
    return sc


# ---- (d) the Wolf static field (polar_wolf) ----------------------------------------------------------------------------------------------------------
WOLF_BASIS = np.diag([90.0, 90.0, 90.0]).astype(np.float64)  # cutoff 45 A: polar_wolf_alpha = 1 reaches a r = 43, exp(-1849)
WOLF_CUTOFF = 45.0
WOLF_ALPHAS = (0.0, 0.13, 1.0)


def wolf_field_factor(r, a, R=WOLF_CUTOFF):
    """thole_field_wolf :3337-3396: f(r) = erfc(a r) / r^2 + 2 a / sqrt(pi) exp(-a^2 r^2) / r - (the same at R); 1 / r^2 - 1 / R^2 for a = 0"""
    r, a, R = M(r), M(a), M(R)
    if a == 0:
        return Terms().add(1 / (r * r), -1 / (R * R)).pair()
    return Terms().add(mp.erfc(a * r) / (r * r), 2 * a / SQRT_PI * mp.exp(-a * a * r * r) / r, -mp.erfc(a * R) / (R * R),
                       -2 * a / SQRT_PI * mp.exp(-a * a * R * R) / R).pair()


@cached
def wolf_field_scan(a):
    """the x components of the Wolf static field on both atoms of the polarizable pair, 0.8 A to the cutoff of 45 A: E_i = q_j f(r) d_ij / r
    for pairs with r - 1e-12 < R"""
    import util  # noqa: F401
    import polar_wolf_ref

    exp_args = [lambda x: -(M(a) * x) ** 2] if a else []
    grid = make_grid(0.8, WOLF_CUTOFF, n_log=300, seed=9, exp_args=exp_args, past_cutoff=False)
    sc = Scan(f"wolf_field[a={a:g}]", grid)
    for r in grid:
        atoms = thole_atoms(r)
        f, fs = wolf_field_factor(r, a) if in_lj(r, WOLF_CUTOFF) else (M(0), M(0))
        cpu = polar_wolf_ref.wolf_field(atoms, WOLF_BASIS, a)
        sc.put("E0x", (-M(Q[1]) * f, abs(M(Q[1])) * fs), cpu[0, 0])  # d_01 / r = (-1, 0, 0)
        sc.put("E1x", (M(Q[0]) * f, abs(M(Q[0])) * fs), cpu[1, 0])
    sc.extra["opts"] = options(polar=True, polar_ewald=0, max_iter=1)
    return sc


# ---- (f) rd_crystal, order 2 ---------------------------------------------------------------------------------------------------------------------------
@cached
def crystal_scan():
    """lj_pairs of the ion pair under rd_crystal order 2 (System::lj :916-963): the 27 images n in [-1, 1]^3 of the RAW displacement, each kept
    unless |S(n) + d| > 2 cutoff (order - 1 / 2) = 36 A, S6 and S12 summed over them, 4 eps (S12 - S6)"""
    import rd_crystal_ref

    grid = make_grid(0.8, CUTOFF, n_log=300, seed=10)
    sc = Scan("rd_crystal[order 2]", grid)
    opts = dict(options(rd_only=1), rd_crystal=1, rd_crystal_order=2)
    shifts, _ = rd_crystal_ref.image_shifts(CUBIC, 2)
    cut = 2.0 * CUTOFF * 1.5
    sig, eps = (M(SIGMA[0]) + M(SIGMA[1])) / 2, mp.sqrt(M(EPS[0]) * M(EPS[1]))
    for r in grid:
        atoms = pair_atoms(r)
        d = atoms["pos"][0] - atoms["pos"][1]
        T = Terms()
        for S in shifts:
            a = S + d  # (the reference's own fp64 sum: it decides which images are kept)
            r64 = float(np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]))
            if r64 > cut:
                continue
            rr = mp.sqrt(sum((M(float(S[p])) + M(float(d[p]))) ** 2 for p in range(3)))
            T.add(4 * eps * (sig / rr) ** 12, -4 * eps * (sig / rr) ** 6)
        sc.put("lj_pairs", T.pair(), rd_crystal_ref.for_case(atoms, CUBIC, opts)["lj_pairs"])
    sc.extra["opts"] = options(rd_only=1)
    return sc


# ---- the case lists that the CPU guard (test_pair_scan_ref.py) and the GPU scans (test_gpu_pair_scans.py) both walk ---------------------------------
# (kernel asked for, cell, intramolecular, ewald alpha, polar_ewald_alpha).  polar_ewald_alpha != ewald_alpha lies outside the sweep's domain
# (pair_sweep_covers): asked for the sweep, the fused kernel must run
FIELD_CASES = [(k, c, i, a, None if a == "default" else ALPHAS[a]) for k in ("sweep", "fused") for c in ("cubic", "triclinic") for i in (False, True)
               for a in ("default", "table_end")]
FIELD_CASES += [("fused", c, i, "default", 0.21) for c in ("cubic", "triclinic") for i in (False, True)] + [("sweep", "cubic", False, "default", 0.21)]
RECIP_CASES = [(2, k, c, u) for k in KMAXES for c in ("cubic", "triclinic") for u in (False, True)]
RECIP_CASES += [(65, k, c, u) for k in KMAXES for c, u in (("cubic", False), ("triclinic", True))]
THOLE_CASES = [(m, k) for m in THOLE_MODES if m != "direct" for k in THOLE_ITERS] + [("direct", 10)]


def field_kernel_that_runs(kernel, alpha, polar_alpha):
    return kernel if polar_alpha in (None, ALPHAS[alpha]) else "fused"


# The trial, exchange and batch kernels take 1 / r from fast_rsqrt, which pair_math.h claims to ~1 ulp.  With 2 ulp for it, s = sigma / r is
# within 3.5 ulp, twelve powers of it within 42 ulp, the five products and the mixing within 8 more, the squared distance within 2 ulp (12 in
# s^12): 62 ulp = 6.9e-15 of the larger LJ term.  Three times that is the bound for `lj_pairs` through those routes; fast_rsqrt with ONE
# Newton step (2e-14, twelve powers 2.4e-13) does not fit in it, while it does fit in the 1e-12 of the other observables.
B_TRIAL_LJ = 2e-14


def delta_terms(sc, key, k, k0):
    """(ref, scale, e_cpu) of the difference between point k and the resting point k0 of a scan: what a displacement trial is held to"""
    ref = sc.ref[key][k] - sc.ref[key][k0]
    scale = sc.scale[key][k] + sc.scale[key][k0]
    return ref, scale, err(sc.cpu[key][k] - sc.cpu[key][k0], ref, scale)


def rest_index(sc):
    k0 = int(np.argmin(np.abs(np.array(sc.points, dtype=np.float64) - REST_R)))
    assert sc.points[k0] == REST_R
    return k0
