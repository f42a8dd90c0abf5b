// kernels_crystal.hip -- `rd_crystal on`: the lattice-summed Lennard-Jones of the reference's System::lj (src/System.Energy.cpp:916-963).
//
//   E = sum over every unordered pair that is not frozen and whose minimum-image distance passes rimg - 1e-12 < cut of
//       4 eps_ij (t12 - S6) [+ lj_fh_corr(t12, S6, 1 / rimg)],   S6 = sum_n (|sigma_ij| / |a_n|)^6,  S12 = sum_n (|sigma_ij| / |a_n|)^12
// over the images n in [-(order-1), order-1]^3 with a_n = S(n) + (pos_i - pos_j) at the RAW positions and |a_n| <= cut; rd_excluded pairs
// (same molecule, null sigma / epsilon) only lose n = 0.  cut = 2 * box cutoff * (order - 0.5).  crystal_self and the two long-range
// corrections depend on the cell and the atom parameters only: the host keeps them (context.cpp: crystal_ready, evaluate.cpp: lrc_box).
//
// The image loop: the trip count and the shifts S(n) are wave-uniform (read with a uniform index from a read-only table: scalar loads),
// the displacement d = pos_i - pos_j is per lane.  a_n = S(n) + d and r2 = ((ax ax) + ay ay) + az az round like the reference (this file is
// built without contraction); the decision |a_n| > cut is r2 > t_img with the host's threshold, so no device square root decides anything.
// A term needs no root and no division by r: sum r^-6 and sum r^-12 are accumulated per pair and scaled by sigma^6 and sigma^12 once.
// Per image term (counted in the gfx950 code object): 3 v_add_f64 (a_n), 3 v_mul_f64 + 2 v_add_f64 (r2), 1 v_cmp, v_rcp_f64 + 4 fma
// (1 / r2 to ~1 ulp), 2 v_mul_f64 (r^-6), 1 v_fma_f64 + 1 v_add_f64 (the two sums), 5 v_cndmask_b32 (the selects), 1 v_add_u32 (the
// count): 24 vector instructions, 17 of them fp64 arithmetic; the terms that fail the cutoff test pay for all of them.
//
// The two walks are pair_term_walk.h's: CrystalTerm states the payload (|sigma|, sqrt(epsilon), 1 / molecule mass), the admission (every
// pair that is not frozen: same-molecule partners count) and the pair function, and sums two quantities, the energy and the image terms
// kept.  Small tables give every tile pair to `jsplit` waves that share its j range (crystal_jsplit).
#include "pair_term_walk.h"

namespace mpmc {

static_assert(S_CRYSTAL_TERMS == S_CRYSTAL + 1 && S_CRYSTAL_TERMS < S_COUNT, "the scalar block holds the two rd_crystal slots side by side");

// 1 / x to ~1 ulp: hardware seed + two Newton steps.  Values only, never predicates.
__device__ __forceinline__ double crystal_rcp(double x) {
	double y = __builtin_amdgcn_rcp(x);
	double e = fma(-x, y, 1.0);
	y = fma(y, e, y);
	e = fma(-x, y, 1.0);
	return fma(y, e, y);
}

// one pair at the raw displacement d = pos_i - pos_j: its rd_energy; cnt += the image terms that passed
template <bool ORTHO>
__device__ __forceinline__ double crystal_pair(const Box &bx, const CrystalParams &cp, const double4 *__restrict__ shift, double dx, double dy, double dz,
                                               const PairFlags &f, double sig, double eps, double imu, int &cnt) {
	double ox, oy, oz;
	const double ri2 = min_image_sq<ORTHO>(bx, dx, dy, dz, ox, oy, oz);
	if (!(ri2 <= cp.t_pair)) return 0.0;
	double s6 = 0.0, s12 = 0.0;
	int c = 0;
	for (int n = 0; n < cp.n_img; ++n) {
		const double4 S = shift[n];
		const double ax = S.x + dx, ay = S.y + dy, az = S.z + dz;
		const double r2 = ((ax * ax) + ay * ay) + az * az;
		const bool ok = !(r2 > cp.t_img) && !(f.rd_excluded && n == cp.centre);
		const double ir2 = crystal_rcp(r2);
		const double ir6 = (ir2 * ir2) * ir2;
		s6 += ok ? ir6 : 0.0;
		s12 = ok ? fma(ir6, ir6, s12) : s12;
		c += ok ? 1 : 0;
	}
	cnt += c;
	const double sig2 = sig * sig, sig6 = (sig2 * sig2) * sig2;
	const double S6 = sig6 * s6;
	const double t12 = f.attractive_only ? 0.0 : (sig6 * sig6) * s12;
	double e = 4.0 * eps * (t12 - S6);
	if (cp.fh_order) e += fh_lj_corr(cp.fh_order, cp.fh_c2, cp.fh_c4, imu, eps, t12, S6, fast_rsqrt(ri2));
	return e;
}

struct CrystalTerm {
	static constexpr int kDoubles = 3, kSums = 2, kBlocks = kCrystalBlocks; // (|sigma|, sqrt(epsilon), 1 / molecule mass)
	static constexpr bool kGeometry = true, kJSplit = true, kClassSkip = false, kPins = false;
	const double2 *lj;
	const double *inv_molmass;
	const double4 *shift;
	CrystalParams cp;
	__device__ __forceinline__ void prepare() {}
	__device__ __forceinline__ void load(int slot, double *v) const {
		const double2 l = lj[slot];
		v[0] = l.x, v[1] = l.y, v[2] = cp.fh_order ? inv_molmass[slot] : 0.0;
	}
	__device__ __forceinline__ static bool admits(const PairFlags &f) { return !f.frozen; }
	template <bool ORTHO>
	__device__ __forceinline__ double pair(const Box &bx, double dx, double dy, double dz, const double *a, const double *b, int fl_a, int fl_b, const PairFlags &f,
	                                       int &cnt) const {
		double sig, eps;
		lj_mix(fl_a, fl_b, a[0], a[1], b[0], b[1], sig, eps);
		return crystal_pair<ORTHO>(bx, cp, shift, dx, dy, dz, f, sig, eps, a[2] + b[2], cnt);
	}
};

int crystal_jsplit(int n_tile_pairs) {
	int s = 1;
	while (s < 16 && (long long)n_tile_pairs * s < kCrystalMinItems) s *= 2;
	return s;
}

void launch_crystal(hipStream_t st, const AtomsDev &at, const Box &bx, const CrystalParams &cp, const double4 *shift, const int2 *tile_pairs,
                    int n_tile_pairs, double *part, double *out2) {
	launch_pair_term_sum(st, CrystalTerm{at.lj, at.inv_molmass, shift, cp}, at, tile_pairs, nullptr, n_tile_pairs, crystal_jsplit(n_tile_pairs), bx, part, out2);
}

void launch_crystal_delta(hipStream_t st, const AtomsDev &at, const Box &bx, const CrystalParams &cp, const double4 *shift, const int *mv_slot,
                          const double4 *mv_new, int m, int *moved_idx, double *part, double *out2) {
	launch_pair_term_delta(st, CrystalTerm{at.lj, at.inv_molmass, shift, cp}, at, bx, mv_slot, mv_new, m, moved_idx, part, out2);
}

} // namespace mpmc
