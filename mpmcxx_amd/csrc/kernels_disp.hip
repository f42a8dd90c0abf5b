// kernels_disp.hip -- the dispersion-expansion repulsion/dispersion term, reference System::disp_expansion (src/System.Energy.cpp:1939-2053),
// which replaces lj() when `disp_expansion on`.
//
//   E = sum over every pair that is neither rd_excluded nor frozen, at ANY distance (no cutoff), of
//       315.775 exp(-alpha_ij (r - r0_ij)) - f6 c6_ij / r^6 - f8 c8_ij / r^8 - f10 c10_ij / r^10
// at the minimum-image distance r (min_image, pair_math.h: the reference's bits in any cell).  The per-pair physics is disp_expansion_pair
// (pair_math.h); the per-atom coefficients co[slot] = (alpha, r0, s6, s8) and t10[slot] = s10, with c_n,ij = s_n,i s_n,j, follow the spatial
// order (context.cpp: disp_coefficients, disp_ready).  The long-range corrections depend on the coefficients, the frozen flags, the cutoff and the volume only: the host keeps them
// (context.cpp: disp_lrc) and the sum kernel writes them next to the pair sum.
//
// The two walks are pair_term_walk.h's: DispTerm states the payload (co and t10: five doubles), the admission (neither rd_excluded nor
// frozen) and the pair function; the sum writes the two corrections next to its pair sum, unscaled, so a repeated evaluation is bit-identical.
#include "pair_term_walk.h"

namespace mpmc {

// the series constants in vector registers (DispConst, pair_math.h)
__device__ __forceinline__ DispConst disp_const_v() {
	DispConst k = disp_const();
	for (int i = 0; i < 9; i++) asm volatile("" : "+v"(k.inv[i]));
	asm volatile("" : "+v"(k.rep));
	asm volatile("" : "+v"(k.tiny));
	return k;
}

template <bool DAMP>
struct DispTerm {
	static constexpr int kDoubles = 5, kSums = 1, kBlocks = kDispBlocks; // (alpha, r0, s6, s8, s10)
	static constexpr bool kGeometry = true, kJSplit = false, kClassSkip = false, kPins = true;
	const double4 *co;
	const double *t10;
	DispParams dp;
	DispConst k; // (filled by prepare)
	__device__ __forceinline__ void prepare() { k = disp_const_v(); }
	__device__ __forceinline__ void load(int slot, double *v) const {
		const double4 c = co[slot];
		v[0] = c.x, v[1] = c.y, v[2] = c.z, v[3] = c.w, v[4] = t10[slot];
	}
	__device__ __forceinline__ static bool admits(const PairFlags &f) { return !f.rd_excluded && !f.frozen; }
	template <bool ORTHO>
	__device__ __forceinline__ double pair(const Box &bx, double dx, double dy, double dz, const double *a, const double *b, int, int, const PairFlags &, int &) const {
		double ox, oy, oz;
		const double r = min_image<ORTHO>(bx, dx, dy, dz, ox, oy, oz);
		const double a_ij = disp_mix_alpha(a[0], b[0], dp.schmidt != 0);
		const double r0_ij = 0.5 * (a[1] + b[1]);
		return disp_expansion_pair(k, r, a_ij, r0_ij, a[2] * b[2], a[3] * b[3], a[4] * b[4], DAMP);
	}
};

void launch_disp_expansion(hipStream_t st, const AtomsDev &at, const double4 *co, const double *t10, const int2 *tile_pairs, int n_tile_pairs,
                           const Box &bx, const DispParams &dp, double lrc_pair, double lrc_self, double *part, double *out) {
	with_flag(dp.damp != 0, [&](auto D) {
		launch_pair_term_sum(st, DispTerm<D.value>{co, t10, dp, {}}, at, tile_pairs, nullptr, n_tile_pairs, 1, bx, part, out, 1, lrc_pair, lrc_self); // (+ the corrections)
	});
}

void launch_disp_expansion_delta(hipStream_t st, const AtomsDev &at, const double4 *co, const double *t10, const Box &bx, const DispParams &dp,
                                 const int *mv_slot, const double4 *mv_new, int m, int *moved_idx, double *part, double *out) {
	with_flag(dp.damp != 0, [&](auto D) { launch_pair_term_delta(st, DispTerm<D.value>{co, t10, dp, {}}, at, bx, mv_slot, mv_new, m, moved_idx, part, out); });
}

} // namespace mpmc
