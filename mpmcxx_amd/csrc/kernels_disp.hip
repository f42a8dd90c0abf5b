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
// k_disp_expansion: all tile pairs I <= J of the 64-atom tiles, one wave per tile pair, lanes own the i-atoms, the j-tile in LDS read at
// wave-uniform addresses; equal tiles keep i < j.  Workgroups take tile pairs in a fixed stride and leave one fp64 partial each;
// k_sum_partials (trial_kernels.h) adds them in a fixed order, unscaled, so a repeated evaluation is bit-identical.
//
// k_disp_expansion_delta: the change under a trial move of m atoms (slots mv_slot, new positions mv_new; old positions resident).  One wave
// per (moved atom t, tile J), lanes own j; a pair of two moved atoms belongs to the one earlier in the move list: O(m N).
#include "kernels.h"
#include "device_math.h"
#include "trial_kernels.h"

namespace mpmc {

// the series constants in vector registers (DispConst, pair_math.h)
__device__ __forceinline__ DispConst disp_const_v() {
	DispConst k = disp_const();
	for (int i = 0; i < 9; i++) asm volatile("" : "+v"(k.inv[i]));
	asm volatile("" : "+v"(k.rep));
	asm volatile("" : "+v"(k.tiny));
	return k;
}

template <bool ORTHO, bool DAMP>
__device__ __forceinline__ double disp_pair(const DispConst &k, const Box &bx, const DispParams &dp, double dx, double dy, double dz, const double4 &ci, double ti,
                                            double a_j, double r0_j, double s6_j, double s8_j, double t10_j) {
	double ox, oy, oz;
	const double r = min_image<ORTHO>(bx, dx, dy, dz, ox, oy, oz);
	const double a_ij = disp_mix_alpha(ci.x, a_j, dp.schmidt != 0);
	const double r0_ij = 0.5 * (ci.y + r0_j);
	return disp_expansion_pair(k, r, a_ij, r0_ij, ci.z * s6_j, ci.w * s8_j, ti * t10_j, DAMP);
}

template <bool ORTHO, bool DAMP>
__global__ __launch_bounds__(64) void k_disp_expansion(const double4 *__restrict__ xyzq, const int2 *__restrict__ mf, const double4 *__restrict__ co,
                                                       const double *__restrict__ t10, const int2 *__restrict__ tile_pairs, int n, int n_tile_pairs,
                                                       Box bx, DispParams dp, double *__restrict__ part) {
	__shared__ double s_x[kTile], s_y[kTile], s_z[kTile];
	__shared__ double s_a[kTile], s_r0[kTile], s_6[kTile], s_8[kTile], s_10[kTile];
	__shared__ int s_mol[kTile], s_fl[kTile];
	const int l = threadIdx.x;
	const DispConst k = disp_const_v();
	double acc = 0.0;
	for (int p = blockIdx.x; p < n_tile_pairs; p += gridDim.x) {
		const int2 tp = tile_pairs[p];
		const int I = tp.x, J = tp.y;
		const int i = I * kTile + l, jl = J * kTile + l;
		const bool i_in = i < n;
		const double4 pi = xyzq[i];
		const int2 mi = mf[i];
		const double4 ci = co[i];
		const double ti = t10[i];
		const double4 pj = xyzq[jl];
		const int2 mj = mf[jl];
		const double4 cj = co[jl];
		const double tj = t10[jl];
		const int nj = min(kTile, n - J * kTile);
		__syncthreads(); // (the previous tile pair's readers are done)
		s_x[l] = pj.x, s_y[l] = pj.y, s_z[l] = pj.z;
		s_a[l] = cj.x, s_r0[l] = cj.y, s_6[l] = cj.z, s_8[l] = cj.w, s_10[l] = tj;
		s_mol[l] = mj.x, s_fl[l] = mj.y;
		__syncthreads();
		for (int jj = 0; jj < nj; ++jj) {
			const PairFlags f = pair_flags(mi.x, mi.y, s_mol[jj], s_fl[jj]);
			const double e = disp_pair<ORTHO, DAMP>(k, bx, dp, pi.x - s_x[jj], pi.y - s_y[jj], pi.z - s_z[jj], ci, ti, s_a[jj], s_r0[jj], s_6[jj], s_8[jj],
			                                        s_10[jj]);
			const bool ok = i_in && (I != J || jj > l) && !f.rd_excluded && !f.frozen;
			acc += ok ? e : 0.0;
		}
	}
	acc = wave_sum(acc);
	if (l == 0) part[blockIdx.x] = acc;
}

// moved_idx[slot] = index of the slot in the moved list, -1 for every other slot (k_mark_moved, trial_kernels.h)
template <bool ORTHO, bool DAMP>
__global__ __launch_bounds__(64) void k_disp_expansion_delta(const double4 *__restrict__ xyzq, const int2 *__restrict__ mf, const double4 *__restrict__ co,
                                                             const double *__restrict__ t10, int n, int n_tiles, Box bx, DispParams dp,
                                                             const int *__restrict__ mv_slot, const double4 *__restrict__ mv_new, int m,
                                                             const int *__restrict__ moved_idx, double *__restrict__ part) {
	const int l = threadIdx.x;
	const DispConst k = disp_const_v();
	// a skewed cell's reciprocal basis in vector registers: with the pointers and the loop state its 18 doubles and the basis' do not all
	// fit the scalar registers of this loop
	Box b = bx;
	if (!ORTHO)
		for (int q = 0; q < 9; q++) asm volatile("" : "+v"(b.r[q]));
	double acc = 0.0;
	const int items = m * n_tiles;
	for (int w = blockIdx.x; w < items; w += gridDim.x) {
		const int t = w / n_tiles, J = w - t * n_tiles;
		const int sa = mv_slot[t];
		double4 pao = xyzq[sa], pan = mv_new[t];
		const int2 ma = mf[sa];
		double4 ca = co[sa];
		double ta = t10[sa];
		// (the moved atom's values are wave-uniform: kept in vector registers, the box and the pointers fill the scalar ones)
		asm volatile("" : "+v"(pao.x), "+v"(pao.y), "+v"(pao.z), "+v"(pan.x), "+v"(pan.y), "+v"(pan.z));
		asm volatile("" : "+v"(ca.x), "+v"(ca.y), "+v"(ca.z), "+v"(ca.w), "+v"(ta));
		const int j = J * kTile + l;
		const bool j_in = j < n;
		const int mv_j = j_in ? moved_idx[j] : -1;
		const double4 pjo = xyzq[j];
		const double4 pjn = (mv_j >= 0) ? mv_new[mv_j] : pjo;
		const int2 mj = mf[j];
		const double4 cj = co[j];
		const double tj = t10[j];
		const PairFlags f = pair_flags(ma.x, ma.y, mj.x, mj.y);
		// partners of the moved atom t: every other atom, a moved one only when it comes later in the move list
		const bool ok = j_in && (mv_j < 0 || mv_j > t) && !f.rd_excluded && !f.frozen;
		if (ok) {
			double e[2];
#pragma unroll 1
			for (int g = 0; g < 2; g++) { // old geometry, then new (one copy of the pair code: fewer live values)
				const double4 pa = g ? pan : pao, pj = g ? pjn : pjo;
				e[g] = disp_pair<ORTHO, DAMP>(k, b, dp, pa.x - pj.x, pa.y - pj.y, pa.z - pj.z, ca, ta, cj.x, cj.y, cj.z, cj.w, tj);
			}
			acc += e[1] - e[0];
		}
	}
	acc = wave_sum(acc);
	if (l == 0) part[blockIdx.x] = acc;
}

int disp_grid(long long work_items) { return (int)std::min<long long>(work_items, kDispBlocks); }

void launch_disp_expansion(hipStream_t st, const AtomsDev &at, const double4 *co, const double *t10, const int2 *tile_pairs, int n_tile_pairs,
                           const Box &bx, const DispParams &dp, double lrc_pair, double lrc_self, double *part, double *out) {
	const int grid = disp_grid(n_tile_pairs);
	with_flags(bx.ortho, dp.damp != 0, [&](auto O, auto D) {
		hipLaunchKernelGGL((k_disp_expansion<O.value, D.value>), dim3(grid), dim3(kTile), 0, st, at.xyzq, at.mf, co, t10, tile_pairs, at.n, n_tile_pairs, bx, dp,
		                   part);
	});
	hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(256), 0, st, part, grid, out, 0, 1.0, 1, lrc_pair, lrc_self, nullptr, nullptr, 0); // (+ the corrections)
}

void launch_disp_expansion_delta(hipStream_t st, const AtomsDev &at, const double4 *co, const double *t10, const Box &bx, const DispParams &dp,
                                 const int *mv_slot, const double4 *mv_new, int m, int *moved_idx, double *part, double *out) {
	const int nt = at.n_pad / kTile;
	const int grid = disp_grid((long long)m * nt);
	launch_mark_moved(st, moved_idx, mv_slot, m, 1);
	with_flags(bx.ortho, dp.damp != 0, [&](auto O, auto D) {
		hipLaunchKernelGGL((k_disp_expansion_delta<O.value, D.value>), dim3(grid), dim3(kTile), 0, st, at.xyzq, at.mf, co, t10, at.n, nt, bx, dp, mv_slot, mv_new,
		                   m, moved_idx, part);
	});
	hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(256), 0, st, part, grid, out, 0, 1.0, 0, 0.0, 0.0, moved_idx, mv_slot, m); // (clears the map)
}

} // namespace mpmc
