// pair_math.h -- per-pair arithmetic of the energy hot path, shared by every HIP kernel.
//
// These are the ONLY places where the physics formulas live.  They are __host__ __device__ (plain C++ without hipcc) so the same
// expressions can be compiled for the host by a sanitizer build (tools/host_asan.sh); the product library only instantiates them
// in device code.
//
// Build contract: this translation unit is compiled with -ffp-contract=off.  The minimum-image distance
// decides pair inclusion and must round exactly like the reference's x86-64 build (no FMA): SURVEY §7
// "bit-exact pair inclusion".  Where a fused multiply-add is wanted for speed it is spelled fma().
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MPMC_HD __host__ __device__ __forceinline__
#else
#define MPMC_HD inline
#endif

namespace mpmc {

constexpr double kPi = 3.141592653589793238462643383279502884;      // reference constants.h:13
constexpr double kOneOverSqrtPi = 0.5641895835477562869480794515607725858440506293289988; // constants.h:48
constexpr double kSmallDR = 1.0e-12;                                  // constants.h:54
constexpr double kMaxValue = 1.0e40;                                  // constants.h:53
constexpr double kDebye2SKA = 85.10597636;                            // constants.h:41
constexpr int kMaxIterationCount = 128;                               // constants.h:52

// per-atom flag bits (host packs them in mpmc_set_atoms)
enum : int {
	AF_FROZEN = 1,     // Atom::frozen
	AF_NULL_RD = 2,    // epsilon == 0 || sigma == 0   (System.cpp:1050)
	AF_HAS_DISP = 4,   // any of c6,c8,c10 != 0        (System.cpp:1052)
	AF_NEG_SIGMA = 8,  // sigma < 0  -> attractive_only (System.cpp:1167)
	AF_ZERO_SIGMA = 16,// sigma == 0                   (System.cpp:1170)
	AF_ZERO_Q = 32,    // charge == 0                  (System.cpp:1059)
	AF_ZERO_ALPHA = 64,// polarizability == 0
	AF_PAD = 128,      // padding slot beyond n (never a real atom)
	AF_DISP_RD = 256   // AF_HAS_DISP of a context whose disp-expansion term replaces LJ: the same exclusion role, but lj_mix no longer
	                   // matters (the LJ sums are not used there), so the fast pair sweep keeps these tile pairs (context.cpp: upload_atoms)
};
// Atoms whose flags change the MIXING of lj_mix (sigma < 0: attractive only; dispersion coefficients), not just the masks of
// pair_exclusions: a tile pair that contains one is left to k_pair_fused.  ONE definition for the host list (context.cpp: upload_atoms)
// and the sweep's skip test (kernels_pair.hip) -- a tile pair must be served by exactly one of the two kernels.
constexpr int kAtomFlagsMixing = AF_HAS_DISP | AF_NEG_SIGMA;

// box constants, passed by value to kernels
struct Box {
	double b[9];   // pbc.basis[q][p]           row-major
	double r[9];   // pbc.reciprocal_basis[q][p] row-major
	double volume, cutoff;
	// squared-distance forms of the reference's cutoff predicates, found on the host by bisection over doubles
	// with a correctly rounded sqrt, so the device never needs an exactly rounded sqrt to decide inclusion:
	//   ri2 <= t_lj   <=>   sqrt(ri2) - 1e-12 < cutoff      (lj :934, thole_field_nopbc :3319)
	//   ri2 <= t_es   <=>   !(sqrt(ri2) > cutoff)           (coulombic_real :1490, real_term :2917)
	double t_lj, t_es;
	double t_wolf; //   ri2 <= t_wolf <=>   sqrt(ri2) < cutoff              (coulombic_wolf :1443)
	int ortho;     // 1 when basis (and therefore reciprocal) is diagonal
};

// ---- minimum_image, reference System.cpp:1202-1279 -----------------------------------------------------
// d = r_i - r_j (caller), returns rimg and dimg; association order as in the reference:
//   img[p] = rint(((0 + R[0][p] d0) + R[1][p] d1) + R[2][p] d2) ; di[p] = d[p] - (((0 + B[0][p] i0) + B[1][p] i1) + B[2][p] i2)
// For a diagonal box the off-diagonal products are exact zeros, so the short form below returns the same
// bits for every finite input.
template <bool ORTHO>
MPMC_HD double min_image(const Box &bx, double dx, double dy, double dz, double &ox, double &oy, double &oz) {
	double ix, iy, iz, tx, ty, tz;
	if (ORTHO) {
		ix = rint(bx.r[0] * dx);
		iy = rint(bx.r[4] * dy);
		iz = rint(bx.r[8] * dz);
		tx = bx.b[0] * ix;
		ty = bx.b[4] * iy;
		tz = bx.b[8] * iz;
	} else {
		ix = rint(((bx.r[0] * dx) + bx.r[3] * dy) + bx.r[6] * dz);
		iy = rint(((bx.r[1] * dx) + bx.r[4] * dy) + bx.r[7] * dz);
		iz = rint(((bx.r[2] * dx) + bx.r[5] * dy) + bx.r[8] * dz);
		tx = ((bx.b[0] * ix) + bx.b[3] * iy) + bx.b[6] * iz;
		ty = ((bx.b[1] * ix) + bx.b[4] * iy) + bx.b[7] * iz;
		tz = ((bx.b[2] * ix) + bx.b[5] * iy) + bx.b[8] * iz;
	}
	double ex = dx - tx, ey = dy - ty, ez = dz - tz;
	double ri2 = ((ex * ex) + ey * ey) + ez * ez;
	double ri = sqrt(ri2);
	if (ri != ri) { // isnan guard, System.cpp:1265
		ox = dx; oy = dy; oz = dz;
		return sqrt(((dx * dx) + dy * dy) + dz * dz);
	}
	ox = ex; oy = ey; oz = ez;
	return ri;
}

// same displacement, squared length only (no sqrt): the inclusion predicates are applied on ri2 (Box::t_lj/t_es)
template <bool ORTHO>
MPMC_HD double min_image_sq(const Box &bx, double dx, double dy, double dz, double &ox, double &oy, double &oz) {
	double ix, iy, iz, tx, ty, tz;
	if (ORTHO) {
		ix = rint(bx.r[0] * dx);
		iy = rint(bx.r[4] * dy);
		iz = rint(bx.r[8] * dz);
		tx = bx.b[0] * ix;
		ty = bx.b[4] * iy;
		tz = bx.b[8] * iz;
	} else {
		ix = rint(((bx.r[0] * dx) + bx.r[3] * dy) + bx.r[6] * dz);
		iy = rint(((bx.r[1] * dx) + bx.r[4] * dy) + bx.r[7] * dz);
		iz = rint(((bx.r[2] * dx) + bx.r[5] * dy) + bx.r[8] * dz);
		tx = ((bx.b[0] * ix) + bx.b[3] * iy) + bx.b[6] * iz;
		ty = ((bx.b[1] * ix) + bx.b[4] * iy) + bx.b[7] * iz;
		tz = ((bx.b[2] * ix) + bx.b[5] * iy) + bx.b[8] * iz;
	}
	ox = dx - tx;
	oy = dy - ty;
	oz = dz - tz;
	return ((ox * ox) + oy * oy) + oz * oz;
}

// 1/sqrt(x) to ~1 ulp: hardware seed (v_rsq_f64, ~2^-23) + two Newton steps.  Values only, never predicates.
MPMC_HD double fast_rsqrt(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
	double y = __builtin_amdgcn_rsq(x);
	double e = fma(-(x * y), y, 1.0);
	y = fma(0.5 * y, e, y);
	e = fma(-(x * y), y, 1.0);
	y = fma(0.5 * y, e, y);
	return y;
#else
	return 1.0 / sqrt(x);
#endif
}

// one Newton step only (~2e-14 relative): enough for the far-field dipole tensor, whose entries feed sums that are
// compared at 1e-9
MPMC_HD double fast_rsqrt_1(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
	double y = __builtin_amdgcn_rsq(x);
	const double e = fma(-(x * y), y, 1.0);
	return fma(0.5 * y, e, y);
#else
	return 1.0 / sqrt(x);
#endif
}

// ---- pair_exclusions, reference System.cpp:1035-1197 (Lorentz-Berthelot branch) --------------------------
struct PairFlags {
	bool intra, frozen, rd_excluded, es_excluded, attractive_only;
};
MPMC_HD PairFlags pair_flags(int mol_i, int fl_i, int mol_j, int fl_j) {
	PairFlags f;
	int any = fl_i | fl_j;
	f.intra = (mol_i == mol_j);
	f.frozen = (fl_i & fl_j & AF_FROZEN) != 0;
	f.rd_excluded = f.intra || ((any & AF_NULL_RD) && !(any & (AF_HAS_DISP | AF_DISP_RD)));
	f.es_excluded = f.intra || (any & AF_ZERO_Q);
	f.attractive_only = (any & AF_NEG_SIGMA) != 0;
	return f;
}
// mixed LJ parameters.  sabs = |sigma|, sqe = sqrt(epsilon) per atom (host precomputes).
// sqrt(ei)*sqrt(ej) replaces the reference's sqrt(ei*ej): <= 1 ulp apart, energies only (never a predicate).
MPMC_HD void lj_mix(int fl_i, int fl_j, double sabs_i, double sqe_i, double sabs_j, double sqe_j, double &sigma, double &epsilon) {
	int any = fl_i | fl_j;
	sigma = (any & AF_ZERO_SIGMA) && !(any & AF_NEG_SIGMA) ? 0.0 : 0.5 * (sabs_i + sabs_j);
	epsilon = (any & AF_NEG_SIGMA) ? 0.0 : sqe_i * sqe_j; // epsilon is never assigned on the sigma<0 branch (System.cpp:1167-1169)
}

// lj_lrc_corr / lj_lrc_self, reference System.Energy.cpp:1036-1096
MPMC_HD double lrc_term(double sigma_abs, double epsilon, double cutoff, double volume) {
	double sig_cut = sigma_abs / cutoff;
	double sig3 = sigma_abs * sigma_abs * sigma_abs;
	double sig_cut3 = sig_cut * sig_cut * sig_cut;
	double sig_cut9 = sig_cut3 * sig_cut3 * sig_cut3;
	return ((16.0 / 3.0) * kPi * epsilon * sig3) * ((1.0 / 3.0) * sig_cut9 - sig_cut3) / volume;
}

// lj pair term, reference System.Energy.cpp:965-993 (caller has applied the inclusion predicate :934-937)
MPMC_HD double lj_term(double sigma_abs, double epsilon, double rimg, bool attractive_only) {
	double s = sigma_abs / rimg;
	double s6 = s * s * s;
	s6 *= s6;
	double s12 = s6 * s6;
	double t12 = attractive_only ? 0.0 : s12;
	return 4.0 * epsilon * (t12 - s6);
}

// ---- the rd model (mpmc_set_rd_model): another mixing rule (pair_exclusions, System.cpp:1069-1177) and another function of r / sigma
// (System::lj :897-1032, lj_buffered_14_7 :1212-1248, dreiding :2098-2215) for the pair sum inside the cutoff ------------------------------
// The values mirror MPMC_RD_FORM_* / MPMC_RD_MIX_* of the public header (context.cpp asserts it).
enum : int { RD_FORM_LJ = 0, RD_FORM_BUFFERED_14_7 = 1, RD_FORM_DREIDING = 2, RD_FORM_COUNT = 3 };
enum : int { RD_MIX_LB = 0, RD_MIX_WALDMAN_HAGLER = 1, RD_MIX_HALGREN = 2, RD_MIX_C6 = 3, RD_MIX_COUNT = 4 };
constexpr double kDreidingGamma = 12.0; // DREIDING_GAMMA, System.Energy.cpp:2094

// Per atom (host, context.cpp: rd_model_ready): sp = (sigma, sigma^2, sigma^3, sigma^6), sqe = sqrt(epsilon) and e = epsilon, sigma >= 0
// and epsilon >= 0 (anything else is refused before a kernel runs, so no pair is ever attractive_only here).
struct RdAtom {
	double s, s2, s3, s6, sqe, e;
};
// The pair's mixed parameters.  No pow: Waldman-Hagler's sixth root is a square root and a cube root (DREIDING: and one correction, rd_sixth_root); one division (Halgren: one each for
// sigma and epsilon, which keeps both within a few ulp of the reference's expressions); sqrt(e_i) sqrt(e_j) stands for the reference's
// sqrt(e_i e_j) as in lj_mix.  A pair with a sigma of 0 gets sigma = 0 (rd_pair_energy returns 0 for it), never a division by zero.
struct RdMixed {
	double sigma, eps;
};
// Waldman-Hagler's sigma as the reference gets it, pow(s6, 1. / 6.), from y = cbrt(sqrt(s6)): DREIDING tests r < 0.4 sigma (:2139), so a
// sigma one ulp off moves a branch between MAXVALUE and a finite term.  y alone (two roundings, and the exact sixth root where the
// reference's exponent is the double below 1 / 6) differs from pow in 64 % of 2e7 random pairs; one Newton step on y^6 = s6 with the
// residual carried in two doubles, and the exponent's 9.25e-18 as a first-order factor, differs in 0.08 % (glibc's pow is not correctly
// rounded either).  Only DREIDING takes it (rd_mix's FORM), the one FORM with a branch on sigma: under the LJ and 14-7 forms sigma stays y,
// a value within an ulp of the reference's like every other mixed parameter here.  (Still open: the sigma rule of cavity_autoreject,
// kernels_contact.hip, tests r < scale sigma with the LJ form's sigma, so under Waldman-Hagler that test can sit one ulp from the reference's.)
MPMC_HD double rd_sixth_root(double x, double y) {
	const double y2 = y * y, e2 = fma(y, y, -y2);
	const double y3 = y2 * y, e3 = fma(y2, y, -y3) + e2 * y;
	const double y6 = y3 * y3, e6 = fma(y3, y3, -y6) + 2.0 * (y3 * e3);
	// x^(fl(1/6)) = x^(1/6) exp(-(1/6 - fl(1/6)) ln x): that factor is 6e-17 from 1, so a single-precision log2 is plenty (one instruction);
	// 6 y^6 by additions and one literal in all: the triclinic walks have no scalar register to spare
#if defined(__HIP_DEVICE_COMPILE__)
	const double l2 = (double)__log2f((float)x);
#else
	const double l2 = (double)log2f((float)x);
#endif
	const double corr = y * (((x - y6) - e6) / (((y6 + y6) + y6) * 2.0) - 6.412899660930516e-18 * l2); // (1/6 - fl(1/6)) ln 2
	return y + corr;
}
template <int MIX, int FORM = RD_FORM_LJ>
MPMC_HD RdMixed rd_mix(const RdAtom &a, const RdAtom &b) {
	RdMixed m;
	const bool zero = (a.s == 0.0) || (b.s == 0.0);
	const double ee = a.sqe * b.sqe;
	if (MIX == RD_MIX_WALDMAN_HAGLER) { // :1072-1091: sigma^6 = (s_i^6 + s_j^6) / 2, eps = sqrt(e_i e_j) 2 s_i^3 s_j^3 / (s_i^6 + s_j^6)
		const double s6 = 0.5 * (a.s6 + b.s6);
		const double y = cbrt(sqrt(s6));
		m.sigma = zero ? 0.0 : (FORM == RD_FORM_DREIDING ? rd_sixth_root(s6, y) : y);
		m.eps = zero ? ee : (ee * (a.s3 * b.s3)) / s6;
	} else if (MIX == RD_MIX_HALGREN) { // :1093-1106: sigma = (s_i^3 + s_j^3) / (s_i^2 + s_j^2), eps = 4 e_i e_j / (sqrt e_i + sqrt e_j)^2
		const bool ezero = (a.e == 0.0) || (b.e == 0.0);
		const double D = a.sqe + b.sqe;
		m.sigma = zero ? 0.0 : (a.s3 + b.s3) / (a.s2 + b.s2);
		m.eps = ezero ? 0.0 : (4.0 * (a.e * b.e)) / (D * D);
	} else if (MIX == RD_MIX_C6) { // :1159-1165: sigma = (s_i + s_j) / 2, eps = 64 sqrt(e_i e_j) s_i^3 s_j^3 / (s_i + s_j)^6
		m.sigma = 0.5 * (a.s + b.s);
		const double t = a.s + b.s, t2 = t * t;
		m.eps = (m.sigma != 0.0) ? ((64.0 * ee) * (a.s3 * b.s3)) / ((t2 * t2) * t2) : 0.0;
	} else { // Lorentz-Berthelot, :1166-1177 with sigma >= 0
		m.sigma = zero ? 0.0 : 0.5 * (a.s + b.s);
		m.eps = ee;
	}
	return m;
}
// LJ form with mixed parameters (:965-993), in the reference's own order: s = sigma / r, t6 = (s s s)^2, t12 = t6^2 (sigma / r enters at
// the twelfth power: another order of the same products moves the result by tens of ulp); t12 and t6 go out for fh_lj_corr
MPMC_HD double rd_lj_term(double eps, double sigma, double r, double &t12, double &t6) {
	const double s = sigma / r;
	t6 = s * s * s;
	t6 *= t6;
	t12 = t6 * t6;
	return 4.0 * eps * (t12 - t6);
}
// Halgren's buffered 14-7 (:1230-1233): eps (1.07 / (rho + 0.07))^7 (1.12 / (rho^7 + 0.12) - 2), rho = r / sigma; the powers are products
MPMC_HD double rd_buffered_14_7_term(double eps, double sigma, double r) {
	const double rho = r / sigma;
	const double a = 1.07 / (rho + 0.07);
	const double a2 = a * a, a7 = ((a2 * a2) * a2) * a;
	const double r2 = rho * rho, r7 = ((r2 * r2) * r2) * rho;
	return (eps * a7) * (1.12 / (r7 + 0.12) - 2.0);
}
// DREIDING exponential-6 (:2129-2145): eps (6 / (g - 6) exp(g (1 - rho)) - g / (g - 6) rho^-6), g = 12; below 0.4 sigma the exponential
// term is MAXVALUE.  ex: the caller's exponential (exp on the host, exp_fast in the kernels)
template <class Exp>
MPMC_HD double rd_dreiding_term(double eps, double sigma, double r, Exp ex) {
	const double rho = r / sigma;
	const double r2 = rho * rho;
	const double term6 = (kDreidingGamma / (kDreidingGamma - 6.0)) / ((r2 * r2) * r2);
	const double termexp = (r < 0.4 * sigma) ? kMaxValue : (6.0 / (kDreidingGamma - 6.0)) * ex(kDreidingGamma * (1.0 - rho));
	return eps * (termexp - term6);
}
// One pair of the model at the squared minimum-image distance ri2 (the caller applied the exclusions and the form's distance test).  A
// pair whose mixed sigma or epsilon is 0 contributes exactly 0 (the reference gets there through 0 / r or r / 0 = inf; no NaN here).
// fh_order != 0 (LJ form only): + fh_lj_corr (below) with the mixed epsilon; imu = 1 / M_i + 1 / M_j.
MPMC_HD double fh_lj_corr(int order, double c2, double c4, double imu, double eps, double t12, double s6, double ir);
template <int FORM, class Exp>
MPMC_HD double rd_pair_energy(const RdMixed &m, double ri2, int fh_order, double fh_c2, double fh_c4, double imu, Exp ex) {
	if (m.sigma == 0.0 || m.eps == 0.0) return 0.0;
	const double r = sqrt(ri2);
	if (FORM == RD_FORM_LJ) {
		double t12, t6;
		double e = rd_lj_term(m.eps, m.sigma, r, t12, t6);
		if (fh_order) e += fh_lj_corr(fh_order, fh_c2, fh_c4, imu, m.eps, t12, t6, 1.0 / r);
		return e;
	}
	if (FORM == RD_FORM_BUFFERED_14_7) return rd_buffered_14_7_term(m.eps, m.sigma, r);
	return rd_dreiding_term(m.eps, m.sigma, r, ex);
}

// Feynman-Hibbs corrections (reference System.Energy.cpp: lj_fh_corr :1100-1148, coulombic_real_FH :1521-1557), per pair, shared by the
// pair sweep and the per-move delta kernels.  c2 = M2A2 hbar^2 / (24 kB T amu2kg), c4 = M2A4 hbar^4 / (1152 kB^2 T^2 amu2kg^2);
// imu = 1/M_i + 1/M_j (molecule masses, amu): the reduced mass enters as its inverse.
MPMC_HD double fh_lj_corr(int order, double c2, double c4, double imu, double eps, double t12, double s6, double ir) {
	const double ir2 = ir * ir;
	const double dE = -24.0 * eps * (2.0 * t12 - s6) * ir;
	const double d2E = 24.0 * eps * (26.0 * t12 - 7.0 * s6) * ir2;
	double corr = c2 * imu * (d2E + 2.0 * dE * ir);
	if (order >= 4) {
		const double ir3 = ir2 * ir;
		const double d3E = -1344.0 * eps * (6.0 * t12 - s6) * ir3;
		const double d4E = 12096.0 * eps * (10.0 * t12 - s6) * (ir2 * ir2);
		corr += c4 * (imu * imu) * (15.0 * dE * ir3 + 4.0 * d3E * ir + d4E);
	}
	return corr;
}
// (added WITHOUT the charge product, as the reference does, :1499-1500); erfc_a = erfc(alpha r), gauss_a = exp(-alpha^2 r^2)
MPMC_HD double fh_es_corr(int order, double c2, double c4, double imu, double al, double erfc_a, double gauss_a, double ri2, double r, double ir) {
	const double a2 = al * al, a3 = a2 * al;
	const double ir2 = ir * ir, ir3 = ir2 * ir, ir4 = ir2 * ir2;
	const double isp = kOneOverSqrtPi;
	const double du = -2.0 * al * gauss_a * ir * isp - erfc_a * ir2;
	const double d2u = 4.0 * isp * gauss_a * (a3 + ir2) + 2.0 * erfc_a * ir3;
	double corr = c2 * imu * (d2u + 2.0 * du * ir);
	if (order >= 4) {
		const double d3u = gauss_a * isp * (-8.0 * (a3 * a2) * r - 8.0 * a3 * ir - 12.0 * al * ir3) - 6.0 * erfc_a * ir4;
		const double d4u = gauss_a * isp * (8.0 * a3 * a2 + 16.0 * a3 * (a3 * al) * ri2 + 32.0 * a3 * ir2 + 48.0 * ir4) + 24.0 * erfc_a * (ir4 * ir);
		corr += c4 * (imu * imu) * (15.0 * du * ir3 + 4.0 * d3u * ir + d4u);
	}
	return corr;
}

// ---- disp_expansion, reference System.Energy.cpp:1939-2053 (mixing System.cpp:1139-1156) ----------------------------------------------
// Per atom: alpha (the PQR epsilon column, 1/A), r0 (sigma, A) and s_n = sqrt(k_n c_n) with the unit factors k_n below, s10 under
// extrapolate_disp_coeffs sqrt(49/40 k8^2 / k6) c8 / sqrt(c6) (0 when c6 or c8 is 0), so that c_n,ij = s_n,i s_n,j (context.cpp:
// disp_coefficients).  The mixed alpha is formed per pair, as the reference does: alpha_i = alpha_j = 0 gives 0/0 = NaN, which keeps
// the repulsion (NaN != 0) and zeroes the damping factors (NaN > 1e-9 is false) exactly like the reference.
constexpr double kDispRepulsion = 315.7750382111558307123944638; // K (= 1e-3 hartree), System.Energy.cpp:1974
constexpr double kDispUnit = 3.166811429 * 0.000001;             // hartree -> K
constexpr double kDispK6 = 0.021958709 / kDispUnit;             // hartree bohr^6 -> K A^6
constexpr double kDispK8 = 0.0061490647 / kDispUnit;
constexpr double kDispK10 = 0.0017219135 / kDispUnit;

MPMC_HD double disp_mix_alpha(double a_i, double a_j, bool schmidt) {
	return schmidt ? ((a_i + a_j) * a_i * a_j) / (a_i * a_i + a_j * a_j) : (2.0 * a_i * a_j) / (a_i + a_j);
}

// the constants of the series below: 1/2 .. 1/10, the repulsion prefactor and the clamp.  A kernel may keep them in vector registers (a
// loop that holds a skewed cell's 18 box doubles in scalar registers has no room for eleven more literals there)
struct DispConst {
	double inv[9], rep, tiny;
};
MPMC_HD DispConst disp_const() {
	return DispConst{{0.5, 1.0 / 3.0, 0.25, 0.2, 1.0 / 6.0, 1.0 / 7.0, 0.125, 1.0 / 9.0, 0.1}, kDispRepulsion, 0.000000001};
}

// tt_damping for n = 6, 8, 10 at once (System.Energy.cpp:2037-2053): 1 - e^{-x} sum_{i<=n} x^i / i!, 0 unless > 1e-9
MPMC_HD void disp_tt_damping(const DispConst &k, double x, double &f6, double &f8, double &f10) {
	const double ex = exp(-x);
	double t = x, s = 1.0 + x; // x^0 / 0! + x^1 / 1!
	double s6 = 0.0, s8 = 0.0;
	for (int i = 0; i < 9; i++) { // x^(i+2) / (i+2)!
		t = (t * x) * k.inv[i];
		s += t;
		if (i == 4) s6 = s;
		if (i == 6) s8 = s;
	}
	const double d6 = 1.0 - ex * s6, d8 = 1.0 - ex * s8, d10 = 1.0 - ex * s;
	f6 = (d6 > k.tiny) ? d6 : 0.0;
	f8 = (d8 > k.tiny) ? d8 : 0.0;
	f10 = (d10 > k.tiny) ? d10 : 0.0;
}

// one pair's rd_energy at the minimum-image distance r (caller applied rd_excluded / frozen; there is no cutoff).  One reciprocal of r^2
// serves the three powers (the reference divides three times: a few ulp apart, and r = 0 or c_n = 0 give the same infinities and NaNs)
MPMC_HD double disp_expansion_pair(const DispConst &k, double r, double alpha_ij, double r0_ij, double c6, double c8, double c10, bool damp) {
	const double ir2 = 1.0 / (r * r);
	const double ir6 = (ir2 * ir2) * ir2;
	const double ir8 = ir6 * ir2;
	const double ir10 = ir8 * ir2;
	const double rep = (alpha_ij != 0.0 && r0_ij != 0.0) ? k.rep * exp(-alpha_ij * (r - r0_ij)) : 0.0;
	double f6 = 1.0, f8 = 1.0, f10 = 1.0;
	if (damp) disp_tt_damping(k, alpha_ij * r, f6, f8, f10);
	return ((-(f6 * c6) * ir6 - (f8 * c8) * ir8) - (f10 * c10) * ir10) + rep;
}

// disp_expansion_lrc / disp_expansion_lrc_self (:2022-2034, :2056-2080) with the coefficients c6, c8, c10 of a pair or of one atom
MPMC_HD double disp_lrc_term(double c6, double c8, double c10, double cutoff, double volume) {
	const double rc3 = cutoff * cutoff * cutoff, rc5 = rc3 * cutoff * cutoff, rc7 = rc5 * cutoff * cutoff;
	return -4.0 * kPi * ((c6 / (3.0 * rc3) + c8 / (5.0 * rc5)) + c10 / (7.0 * rc7)) / volume;
}

// Thole exponential damping, reference System.Energy.cpp:2731-2757:  T = a*I - b*(d (x) d),
//   a = damp1/r^3, b = 3*damp2/r^5.  r == 0 gives the reference's MAXVALUE guard (:2704-2705).
MPMC_HD void thole_ab(double r, double lambda, double &a, double &b) {
	double ir3, ir5;
	if (r == 0.0) {
		ir3 = ir5 = kMaxValue;
	} else {
		double ir = 1.0 / r;
		ir3 = ir * ir * ir;
		ir5 = ir3 * ir * ir;
	}
	double r2 = r * r;
	double l2 = lambda * lambda, l3 = l2 * lambda;
	double explr = exp(-lambda * r);
	double damp1 = 1.0 - explr * (0.5 * l2 * r2 + lambda * r + 1.0);
	double damp2 = damp1 - explr * (l3 * r2 * r / 6.0);
	a = damp1 * ir3;
	b = 3.0 * damp2 * ir5;
}

// real_term factor, reference System.Energy.cpp:2919-2934 (caller applied  !(r > rc || r == 0) and !frozen)
MPMC_HD double field_real_factor(double r, double alpha, bool es_excluded) {
	double r2 = r * r;
	double g = 2.0 * alpha * kOneOverSqrtPi * exp(-alpha * alpha * r2) * r;
	return es_excluded ? (g - erf(alpha * r)) / (r * r2) : (g + erfc(alpha * r)) / (r2 * r);
}

} // namespace mpmc
