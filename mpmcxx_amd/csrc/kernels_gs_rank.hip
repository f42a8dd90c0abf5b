// kernels_gs_rank.hip -- `polar_gs_ranked on`: the rank pass of System::pairs() (src/System.cpp:1001-1029), the sweep order of update_ranking
// (src/System.Energy.cpp:3631-3656) and the ranked view the Gauss-Seidel pipeline of kernels_gs.hip sweeps from its second iteration on.
//
//   rmin          the smallest minimum-image distance over all pairs of polarizable atoms (same-molecule and frozen pairs too): one pass
//                 over the tile pairs, the project's exact minimum image (pair_math.h, no contraction).  A minimum does not depend on an
//                 order and a correctly rounded square root is monotone, so the smallest rimg is the root of the smallest rimg^2: the
//                 kernel keeps the squares (atomicMin on their bit patterns, which order like the non-negative doubles they are) and the
//                 count kernel takes ONE root -- the reference's double, bit for bit.
//   rank_metric   per polarizable atom, the polarizable partners with sqrt(r2) <= rmin * 1.5, r2 the UNWRAPPED ((dx dx) + dy dy) + dz dz
//                 (pair->r, not rimg: :1022).  Whole rows, so nothing is added atomically; the predicate is evaluated as written
//                 (wherever the squares leave it open).
//   order         update_ranking is a bubble sort: the stable descending order of rank_metric.  Every atom finds its own place in it --
//                 the atoms with a larger key, plus those with the same key in front of it -- by the same whole-row walk as the count:
//                 integer compares, no atomics, no scan, correct for any keys.  order[p] = the atom swept p-th.
//   view          positions, parameters, E0 and the dipoles gathered into sweep order (gather), the results put back (scatter).
// Padded slots keep their places at the end.
#include <limits.h>

#include "kernels.h"

namespace mpmc {

constexpr int kRankWaves = 16;

__device__ __forceinline__ bool gr_polarizable(const AtomsDev &at, int i) { return i < at.n && at.alpha[i] != 0.0 && !(at.mf[i].y & AF_PAD); }

// one wave per tile pair (I <= J): lane = an atom of tile I, the 64 atoms of tile J from LDS
template <bool ORTHO>
__global__ __launch_bounds__(64) void k_gr_rmin(AtomsDev at, Box bx, const int2 *__restrict__ tile_pairs, unsigned long long *__restrict__ min_r2_bits) {
	__shared__ double4 s_pos[kTile];
	__shared__ int s_pol[kTile];
	const int lane = threadIdx.x;
	const int2 tp = tile_pairs[blockIdx.x];
	const int i = tp.x * kTile + lane, jl = tp.y * kTile + lane;
	s_pos[lane] = at.xyzq[jl];
	s_pol[lane] = gr_polarizable(at, jl) ? 1 : 0;
	const double4 pi = at.xyzq[i];
	const bool pol_i = gr_polarizable(at, i);
	__syncthreads();
	double m = HUGE_VAL;
	if (pol_i)
		for (int c = 0; c < kTile; ++c) {
			if (!s_pol[c] || (tp.x == tp.y && c == lane)) continue;
			const double4 pj = s_pos[c];
			double ox, oy, oz;
			const double r2 = min_image_sq<ORTHO>(bx, pi.x - pj.x, pi.y - pj.y, pi.z - pj.z, ox, oy, oz);
			if (r2 < m) m = r2;
		}
	for (int off = 32; off > 0; off >>= 1) {
		const double o = __shfl_xor(m, off);
		if (o < m) m = o;
	}
	// one atomic per wave, and only where it can still lower the minimum (the value read may be stale, never too small: it only decreases)
	const unsigned long long bits = (unsigned long long)__double_as_longlong(m);
	if (lane == 0 && m < HUGE_VAL && bits < __hip_atomic_load(min_r2_bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(min_r2_bits, bits);
}

// whole-row counts: one workgroup per row tile, lane = row atom.  The columns come through LDS, kRankWaves tiles at a time (thread t stages
// column atom t of the group, coalesced; a column read from global memory per step, even wave-uniformly, costs its latency every step:
// 283 us against the distance arithmetic's few); wave w then walks tile w of the group.  MODE 0: rank_metric from the distances,
// MODE 1: the place of every atom in the stable descending order of `key`
template <int MODE>
__global__ __launch_bounds__(64 * kRankWaves) void k_gr_rows(AtomsDev at, const unsigned long long *__restrict__ min_r2_bits, double *__restrict__ rmin_out,
                                                            const int *__restrict__ key, int *__restrict__ out, int *__restrict__ tally /*{ max_rank, n_moved }*/) {
	__shared__ int s_cnt[kRankWaves][kTile];
	__shared__ double4 s_pos[MODE == 0 ? kRankWaves * kTile : 1];
	__shared__ int s_val[MODE == 1 ? kRankWaves * kTile : 1]; // MODE 1: the column atom's key, INT_MIN behind the last atom
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	const int nt = at.n_pad / kTile;
	const int i = blockIdx.x * kTile + lane;
	int cnt = 0;
	double thr = 0.0, t2_in = 0.0, t2_out = 0.0;
	double4 pi = make_double4(0.0, 0.0, 0.0, 0.0);
	bool pol_i = false;
	int ki = 0;
	if (MODE == 0) {
		const unsigned long long bits = *min_r2_bits;
		// (no polarizable pair: the reference's rmin stays MAXVALUE, :1003)
		const double rmin = (bits == ~0ull) ? kMaxValue : sqrt(__longlong_as_double((long long)bits));
		if (blockIdx.x == 0 && threadIdx.x == 0) *rmin_out = rmin;
		thr = rmin * 1.5;
		// the predicate is sqrt(r2) <= thr as written; the root is taken only where the squares do not already decide it: one part in a
		// million away from thr^2 no rounding of the square or of the root can change the answer
		const double t2 = thr * thr;
		t2_in = t2 * 0.999999, t2_out = t2 * 1.000001;
		pi = at.xyzq[i];
		pol_i = gr_polarizable(at, i);
	} else {
		ki = (i < at.n) ? key[i] : 0;
	}
	for (int J0 = 0; J0 < nt; J0 += kRankWaves) { // (the same trips for every wave: the barriers below are reached by all)
		const int js = J0 * kTile + (int)threadIdx.x;
		if (MODE == 0) { // (a column that is not polarizable stands at infinity: r2 = inf is within nothing, and the walk needs no branch)
			const bool pol = js < at.n_pad && gr_polarizable(at, js);
			s_pos[threadIdx.x] = pol ? at.xyzq[js] : make_double4(HUGE_VAL, 0.0, 0.0, 0.0);
		} else {
			s_val[threadIdx.x] = (js < at.n) ? key[js] : INT_MIN;
		}
		__syncthreads();
		if (J0 + w < nt) {
			const int base = w * kTile, j0 = (J0 + w) * kTile;
			if (MODE == 0) {
#pragma unroll 8
				for (int c = 0; c < kTile; ++c) {
					const double4 pj = s_pos[base + c];
					const double dx = pi.x - pj.x, dy = pi.y - pj.y, dz = pi.z - pj.z;
					const double r2 = ((dx * dx) + dy * dy) + dz * dz;
					const bool within = r2 < t2_in || (r2 <= t2_out && sqrt(r2) <= thr);
					if (pol_i && j0 + c != i && within) ++cnt;
				}
			} else {
#pragma unroll 8
				for (int c = 0; c < kTile; ++c) {
					const int kj = s_val[base + c]; // (INT_MIN behind the last atom is above no key, and no row stands behind those columns)
					if (kj > ki || (kj == ki && j0 + c < i)) ++cnt;
				}
			}
		}
		__syncthreads();
	}
	s_cnt[w][lane] = cnt;
	__syncthreads();
	if (w != 0) return;
	int sum = 0;
	for (int v = 0; v < kRankWaves; ++v) sum += s_cnt[v][lane];
	if (MODE == 0) {
		out[i] = sum; // (0 for atoms that are not polarizable and for padded slots)
		int top = sum;
		for (int off = 32; off > 0; off >>= 1) top = max(top, __shfl_xor(top, off));
		if (lane == 0 && top > __hip_atomic_load(tally, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(tally, top);
	} else {
		const bool real = i < at.n;
		out[real ? sum : i] = i; // the places are a permutation of [0, n): every element of `out` is written once
		const int moved = __popcll(__ballot(real && sum != i));
		if (lane == 0 && moved) atomicAdd(tally + 1, moved);
	}
}

__global__ __launch_bounds__(256) void k_gr_gather(const int *__restrict__ order, AtomsDev src, GsRankView dst, const double *__restrict__ e_static,
                                                   const double *__restrict__ mu) {
	const int p = blockIdx.x * 256 + threadIdx.x;
	if (p >= src.n_pad) return;
	const int s = order[p];
	dst.xyzq[p] = src.xyzq[s];
	dst.lj[p] = src.lj[s];
	dst.mf[p] = src.mf[s];
	dst.alpha[p] = src.alpha[s];
	dst.eps[p] = src.eps[s];
	dst.inv_molmass[p] = src.inv_molmass[s];
	for (int d = 0; d < 3; ++d) {
		dst.e_static[3 * (size_t)p + d] = e_static[3 * (size_t)s + d];
		dst.mu[3 * (size_t)p + d] = mu[3 * (size_t)s + d];
	}
}

// three components per atom from sweep order back to atom order, up to four vectors; then one value per atom (may be null)
__global__ __launch_bounds__(256) void k_gr_scatter(const int *__restrict__ order, int n_pad, GsRankScatter v) {
	const int p = blockIdx.x * 256 + threadIdx.x;
	if (p >= n_pad) return;
	const int s = order[p];
	for (int k = 0; k < 4; ++k) {
		if (!v.src3[k]) continue;
		for (int d = 0; d < 3; ++d) v.dst3[k][3 * (size_t)s + d] = v.src3[k][3 * (size_t)p + d];
	}
	if (v.src1) v.dst1[s] = v.src1[p];
}

void launch_gs_rank(hipStream_t st, const AtomsDev &at, const Box &bx, const int2 *tile_pairs, int n_tile_pairs, GsRankInfoDev *info, int *rank_metric,
                    int *order) {
	const int nt = at.n_pad / kTile;
	(void)hipMemsetAsync(info, 0, sizeof(GsRankInfoDev), st);
	(void)hipMemsetAsync(&info->min_r2_bits, 0xff, sizeof(unsigned long long), st); // above the bits of every distance
	if (bx.ortho) hipLaunchKernelGGL(k_gr_rmin<true>, dim3(n_tile_pairs), dim3(64), 0, st, at, bx, tile_pairs, &info->min_r2_bits);
	else hipLaunchKernelGGL(k_gr_rmin<false>, dim3(n_tile_pairs), dim3(64), 0, st, at, bx, tile_pairs, &info->min_r2_bits);
	hipLaunchKernelGGL(k_gr_rows<0>, dim3(nt), dim3(64 * kRankWaves), 0, st, at, &info->min_r2_bits, &info->rmin, nullptr, rank_metric, &info->max_rank);
	launch_gs_rank_order(st, at, rank_metric, order, &info->max_rank);
}

void launch_gs_rank_order(hipStream_t st, const AtomsDev &at, const int *key, int *order, int *tally2) {
	hipLaunchKernelGGL(k_gr_rows<1>, dim3(at.n_pad / kTile), dim3(64 * kRankWaves), 0, st, at, nullptr, nullptr, key, order, tally2);
}

void launch_gs_rank_gather(hipStream_t st, const int *order, const AtomsDev &src, const GsRankView &dst, const double *e_static, const double *mu) {
	hipLaunchKernelGGL(k_gr_gather, dim3((src.n_pad + 255) / 256), dim3(256), 0, st, order, src, dst, e_static, mu);
}

void launch_gs_rank_scatter(hipStream_t st, const int *order, int n_pad, const GsRankScatter &v) {
	hipLaunchKernelGGL(k_gr_scatter, dim3((n_pad + 255) / 256), dim3(256), 0, st, order, n_pad, v);
}

} // namespace mpmc
