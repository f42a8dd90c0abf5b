// kernels_sg.hip -- the Silvera-Goldman H2 potential (mpmc_set_silvera_goldman), reference System::sg (src/System.Energy.cpp:1763-1867),
// which replaces lj() when `sg on` (:115-116).
//
//   E = 3.15774655e5 K * sum over EVERY pair i < j of the atom list with rimg < cutoff (strict: Box::t_wolf) of V [+ V_FH],
//       V = exp(ALPHA - BETA x - GAMMA x^2) - (C6 / x^6 + C8 / x^8 + C10 / x^10 - C9 / x^9) f(x),   x = rimg / 0.529177249,
//       f = exp(-(RM / x - 1)^2) for x < RM, 1 otherwise
// at the minimum-image distance (min_image_sq, pair_math.h: the reference's bits in any cell).  sg() tests neither rd_excluded nor frozen:
// intramolecular pairs and sites without sigma or epsilon count, and sigma, epsilon and the charge play no part.  V_FH is the expression of
// :1831-1845 as written: 110 C10 / x^10 in the second derivative, derivatives in bohr under a prefactor in Angstrom^2, and the mass of the
// molecule of the atom that comes FIRST in the caller's list -- so the FH payload is (1 / molecule mass, index in the caller's list), and the
// spatial order of the slots never shows.  Without FH there is no payload at all.
//
// The two walks are pair_term_walk.h's.  SgTerm<FH> admits every pair and sums two quantities (energy, kept terms; the count as a double:
// exact).  The powers come by multiplication from one reciprocal, the two exponentials are exp_fast (device_math.h).
//
// Registers (hipcc -O3, gfx950, --save-temps), orthorhombic / triclinic: the FH delta instantiation, whose moved atom's payload is pinned
// into vector registers, takes 71 / 95 VGPRs; the delta without FH 53 / 79; the sums 63 / 63 with FH and 40 / 43 without.  No scratch, no
// spill; 2 KiB of LDS without FH (the payload rows are gone), 3 KiB with.
#include "pair_term_walk.h"

namespace mpmc {

static_assert(S_SG_TERMS < S_COUNT, "the scalar block holds the Silvera-Goldman slots");

// one pair at the distance x (bohr), inside the cutoff: V, or V + V_FH with fh = M2A^2 hBar^2 / (24 kB T amu mass)
template <bool FH>
__device__ __forceinline__ double sg_pair(double x, double fh) {
	constexpr double ALPHA = 1.713, BETA = 1.5671, GAMMA = 0.00993, C6 = 12.14, C8 = 215.2, C10 = 4813.9, C9 = 143.1, RM = 8.321;
	const double rep = exp_fast(ALPHA - BETA * x - GAMMA * x * x);
	const double i1 = 1.0 / x, i2 = i1 * i1, i4 = i2 * i2, i6 = i4 * i2, i8 = i4 * i4, i9 = i8 * i1, i10 = i8 * i2;
	const double mult = C6 * i6 + C8 * i8 + C10 * i10 - C9 * i9;
	const double r_rm = RM * i1, d = r_rm - 1.0;
	const double ex = (x < RM) ? exp_fast(-(d * d)) : 1.0;
	double v = rep - mult * ex;
	if (FH) {
		const double i7 = i6 * i1, i11 = i10 * i1;
		const double bg = BETA + 2.0 * GAMMA * x;
		const double diff1 = (r_rm * r_rm - r_rm) * i1;
		double d1 = -bg * rep;
		d1 += (6.0 * C6 * i7 + 8.0 * C8 * i9 - 9.0 * C9 * i10 + 10.0 * C10 * i11) * ex;
		d1 += -2.0 * mult * ex * diff1;
		double d2 = (bg * bg - 2.0 * GAMMA) * rep;
		d2 += (-ex) * (42.0 * C6 * i8 + 72.0 * C8 * i10 - 90.0 * C9 * i11 + 110.0 * C10 * i10); // (x^10, as the reference writes it)
		d2 += ex * diff1 * (12.0 * C6 * i7 + 16.0 * C8 * i9 - 18.0 * C9 * i10 + 20.0 * C10 * i11);
		d2 += ex * (diff1 * diff1) * 4.0 * mult;
		const double diff2 = (3.0 * r_rm * r_rm - 2.0 * r_rm) * i2;
		d2 += ex * diff2 * 2.0 * mult;
		v += fh * (d2 + 2.0 * d1 * i1);
	}
	return v;
}

template <bool FH>
struct SgTerm {
	static constexpr int kDoubles = FH ? 2 : 0, kSums = 2, kBlocks = kSgBlocks; // (1 / molecule mass, index in the caller's list)
	static constexpr bool kGeometry = true, kJSplit = false, kClassSkip = false, kPins = true;
	const double *inv_molmass;
	const int *perm; // slot -> index in the caller's list
	SgParams sp;
	__device__ __forceinline__ void prepare() {}
	__device__ __forceinline__ void load(int slot, double *v) const {
		if (FH) v[0] = inv_molmass[slot], v[1] = (double)perm[slot];
	}
	__device__ __forceinline__ static bool admits(const PairFlags &) { return true; }
	template <bool ORTHO>
	__device__ __forceinline__ double pair(const Box &bx, double dx, double dy, double dz, const double *a, const double *b, int, int, const PairFlags &,
	                                       int &cnt) const {
		double ox, oy, oz;
		const double ri2 = min_image_sq<ORTHO>(bx, dx, dy, dz, ox, oy, oz);
		if (!(ri2 <= bx.t_wolf)) return 0.0; // (rimg < cutoff, :1805)
		cnt += 1;
		double fh = 0.0;
		if (FH) fh = sp.fh_c * ((a[1] < b[1]) ? a[0] : b[0]);
		return sg_pair<FH>(sqrt(ri2) / kBohr, fh) * kHartreeK;
	}
	static constexpr double kBohr = 0.529177249, kHartreeK = 3.15774655e5;
};

void launch_sg(hipStream_t st, const AtomsDev &at, const int *perm, const int2 *tile_pairs, int n_tile_pairs, const Box &bx, const SgParams &sp, double *part,
               double *out2) {
	with_flag(sp.fh != 0, [&](auto F) { launch_pair_term_sum(st, SgTerm<F.value>{at.inv_molmass, perm, sp}, at, tile_pairs, nullptr, n_tile_pairs, 1, bx, part, out2); });
}

void launch_sg_delta(hipStream_t st, const AtomsDev &at, const int *perm, const Box &bx, const SgParams &sp, const int *mv_slot, const double4 *mv_new, int m,
                     int *moved_idx, double *part, double *out2) {
	with_flag(sp.fh != 0, [&](auto F) { launch_pair_term_delta(st, SgTerm<F.value>{at.inv_molmass, perm, sp}, at, bx, mv_slot, mv_new, m, moved_idx, part, out2); });
}

} // namespace mpmc
