// pair_term_walk.h -- the two walks of the energy terms that are sums over atom pairs (disp-expansion, rd_crystal, the rd model and its pair
// correction, Silvera-Goldman), written once.  Included after kernels.h by kernels_disp.hip, kernels_crystal.hip, kernels_rd_model.hip and kernels_sg.hip; a term's file holds
// its Term and its launchers, nothing of the walks.
//
// k_pair_term_sum: all tile pairs I <= J of the 64-atom tiles, one 64-lane wave per item, items in a fixed stride over the grid.  Lanes own
// the i-atoms, the j-tile waits in LDS and is read at wave-uniform addresses; equal tiles keep i < j.  `jsplit` waves share a tile pair's j
// range (rd_crystal's small tables; 1 for every other term); a tile pair whose class says CLS_BEYOND_CUTOFF is not walked (`cls`, the rd
// model; null for every other term).  A term that never uses an option says so (kJSplit, kClassSkip) and its instantiations hold none of it.  Each lane adds its pairs in the order (item, then jj ascending); wave_sum; one partial per workgroup
// and quantity at part[q kBlocks + blockIdx.x]; k_sum_partials (trial_kernels.h) adds each array in its fixed order.  No atomics.
//
// k_pair_term_delta: the change under a trial move of m atoms (slots mv_slot, new positions mv_new; old positions resident).  One wave per
// (moved atom t, tile J), lanes own j, the moved atom's values wave-uniform; a pair of two moved atoms belongs to the one earlier in the
// move list: O(m N).  launch_mark_moved in front, the map-clearing k_sum_partials behind.
//
// A Term (passed by value, like PairField of k_field_delta) states:
//   kDoubles, load(slot, v)   the per-atom payload, as doubles (0: none); the walks lay it into LDS as s_v[kDoubles][64] and read it back
//   kGeometry                 false: a sum over the parameters alone -- no positions, no molecule ids (the rd model's pair correction)
//   admits(PairFlags)         which pairs count
//   pair<ORTHO>(...)          one pair at the raw displacement pos_a - pos_b with both payloads and flag words; cnt += the terms it kept
//   kSums                     quantities summed: 1 the energy, 2 + the kept terms (counts as doubles: exact), 3 + the skipped tile pairs
//   kBlocks                   the cap of the grid = the stride of the arrays of partials
//   kJSplit, kClassSkip       whether the term ever runs with jsplit > 1 / with classes
//   kPins                     the delta walk pins the wave-uniform values into vector registers (below); rd_crystal says no: its image loop
//                             wants the vector registers more, and parks a few scalar ones in lanes instead, as it always did
//   prepare()                 once per kernel: constants into vector registers (or nothing)
#pragma once

#include "kernels.h"
#include "device_math.h"
#include "trial_kernels.h"

namespace mpmc {

// partials a launch over this many items leaves
inline int pair_term_grid(long long work_items, int blocks) { return (int)std::max<long long>(1, std::min<long long>(work_items, blocks)); }

template <bool ORTHO, class Term>
__global__ __launch_bounds__(64) void k_pair_term_sum(Term term, const double4 *__restrict__ xyzq, const int2 *__restrict__ mf, const int2 *__restrict__ tile_pairs,
                                                      const int *__restrict__ cls, int n, int n_items, int jsplit, Box bx, double *__restrict__ part) {
	constexpr int D = Term::kDoubles, DA = D > 0 ? D : 1; // (a term without payload: arrays of one unused element, which take no register and no LDS)
	constexpr bool G = Term::kGeometry;
	__shared__ double s_pos[3][kTile], s_v[DA][kTile];
	__shared__ int s_mol[kTile], s_fl[kTile]; // (an instantiation without geometry never touches s_pos and s_mol: they take no LDS there)
	const int l = threadIdx.x;
	if (!Term::kJSplit) jsplit = 1;
	const int jw = kTile / jsplit; // j-atoms per item
	term.prepare();
	double acc = 0.0, terms = 0.0, skipped = 0.0;
	for (int w = blockIdx.x; w < n_items; w += gridDim.x) {
		const int p = w / jsplit, q = w - p * jsplit;
		if (Term::kClassSkip && cls && (cls[p] & CLS_BEYOND_CUTOFF)) { // (wave-uniform) the tiles' bounding boxes are further apart than the cutoff: no pair passes
			if (q == 0) skipped += 1.0;
			continue;
		}
		const int2 tp = tile_pairs[p];
		const int I = tp.x, J = tp.y;
		const int i = I * kTile + l, jl = J * kTile + l; // (both < n_pad: every per-atom array is padded to whole tiles)
		const bool i_in = i < n;
		double4 pi = {}, pj = {};
		if (G) pi = xyzq[i], pj = xyzq[jl];
		const int2 mi = mf[i], mj = mf[jl];
		double vi[DA], vj[DA];
		term.load(i, vi);
		term.load(jl, vj);
		const int nj = min(kTile, n - J * kTile);
		__syncthreads(); // (the previous item's readers are done)
		if (G) s_pos[0][l] = pj.x, s_pos[1][l] = pj.y, s_pos[2][l] = pj.z, s_mol[l] = mj.x;
		for (int d = 0; d < D; d++) s_v[d][l] = vj[d];
		s_fl[l] = mj.y;
		__syncthreads();
		int cnt = 0;
		const int j1 = min(nj, (q + 1) * jw);
		for (int jj = q * jw; jj < j1; ++jj) {
			const PairFlags f = pair_flags(mi.x, mi.y, G ? s_mol[jj] : mi.x, s_fl[jj]); // (without geometry only the flag words speak)
			if (i_in && (I != J || jj > l) && Term::admits(f)) {
				double vb[DA];
				for (int d = 0; d < D; d++) vb[d] = s_v[d][jj];
				acc += term.template pair<ORTHO>(bx, G ? pi.x - s_pos[0][jj] : 0.0, G ? pi.y - s_pos[1][jj] : 0.0, G ? pi.z - s_pos[2][jj] : 0.0, vi, vb, mi.y,
				                                 s_fl[jj], f, cnt);
			}
		}
		if (Term::kSums >= 2) terms += (double)wave_sum_i(cnt); // (at most 64 * 64 * 3375 per item: no overflow; the running total is a double, exact below 2^53)
	}
	acc = wave_sum(acc);
	if (l == 0) {
		part[blockIdx.x] = acc;
		if (Term::kSums >= 2) part[Term::kBlocks + blockIdx.x] = terms;
		if (Term::kSums >= 3) part[2 * Term::kBlocks + blockIdx.x] = skipped;
	}
}

// moved_idx[slot] = index of the slot in the moved list, -1 for every other slot (k_mark_moved, trial_kernels.h)
template <bool ORTHO, class Term>
__global__ __launch_bounds__(64) void k_pair_term_delta(Term term, const double4 *__restrict__ xyzq, const int2 *__restrict__ mf, int n, int n_tiles, Box bx,
                                                        const int *__restrict__ mv_slot, const double4 *__restrict__ mv_new, int m,
                                                        const int *__restrict__ moved_idx, double *__restrict__ part) {
	constexpr int D = Term::kDoubles, DA = D > 0 ? D : 1;
	const int l = threadIdx.x;
	term.prepare();
	// a skewed cell's reciprocal basis in vector registers: with the pointers, the parameters and the loop state the 18 doubles of the two
	// bases do not all fit the scalar registers of this loop
	Box b = bx;
	if (Term::kPins && !ORTHO)
		for (int q = 0; q < 9; q++) asm volatile("" : "+v"(b.r[q]));
	double acc = 0.0, terms = 0.0;
	const int items = m * n_tiles;
	for (int w = blockIdx.x; w < items; w += gridDim.x) {
		const int t = w / n_tiles, J = w - t * n_tiles;
		const int sa = mv_slot[t];
		double4 pao = xyzq[sa], pan = mv_new[t];
		const int2 ma = mf[sa];
		double va[DA];
		term.load(sa, va);
		// (the moved atom's values are wave-uniform: kept in vector registers, the box and the pointers fill the scalar ones; an orthorhombic
		// cell leaves room for the new position)
		if (Term::kPins) {
			asm volatile("" : "+v"(pao.x), "+v"(pao.y), "+v"(pao.z));
			if (!ORTHO) asm volatile("" : "+v"(pan.x), "+v"(pan.y), "+v"(pan.z));
			for (int d = 0; d < D; d++) asm volatile("" : "+v"(va[d]));
		}
		const int j = J * kTile + l; // (< n_pad)
		const bool j_in = j < n;
		const int mv_j = j_in ? moved_idx[j] : -1;
		const double4 pjo = xyzq[j];
		const double4 pjn = (mv_j >= 0) ? mv_new[mv_j] : pjo;
		const int2 mj = mf[j];
		double vj[DA];
		term.load(j, vj);
		const PairFlags f = pair_flags(ma.x, ma.y, mj.x, mj.y);
		// partners of the moved atom t: every other atom the term admits, a moved one only when it comes later in the move list
		const bool ok = j_in && (mv_j < 0 || mv_j > t) && Term::admits(f);
		int cnt[2] = {0, 0};
		if (ok) {
			double e[2];
#pragma unroll 1
			for (int g = 0; g < 2; g++) { // old geometry, then new (one copy of the pair code: fewer live values)
				const double4 pa = g ? pan : pao, pj = g ? pjn : pjo;
				int c = 0;
				e[g] = term.template pair<ORTHO>(b, pa.x - pj.x, pa.y - pj.y, pa.z - pj.z, va, vj, ma.y, mj.y, f, c);
				cnt[g] = c;
			}
			acc += e[1] - e[0];
		}
		if (Term::kSums >= 2) terms += (double)wave_sum_i(cnt[1] - cnt[0]);
	}
	acc = wave_sum(acc);
	if (l == 0) {
		part[blockIdx.x] = acc;
		if (Term::kSums >= 2) part[Term::kBlocks + blockIdx.x] = terms;
	}
}

// the sum and the fixed-order sums of its Term::kSums arrays into out[0 ..]; extra1, extra2 (one quantity only): out[1], out[2]
template <class Term>
inline void launch_pair_term_sum(hipStream_t st, const Term &term, const AtomsDev &at, const int2 *tile_pairs, const int *cls, int n_tile_pairs, int jsplit,
                                 const Box &bx, double *part, double *out, int n_extra = 0, double extra1 = 0.0, double extra2 = 0.0) {
	const long long items = (long long)n_tile_pairs * jsplit;
	const int grid = pair_term_grid(items, Term::kBlocks);
	with_flag(bx.ortho || !Term::kGeometry, [&](auto O) {
		hipLaunchKernelGGL((k_pair_term_sum<O.value || !Term::kGeometry, Term>), dim3(grid), dim3(kTile), 0, st, term, at.xyzq, at.mf, tile_pairs, cls, at.n, (int)items,
		                   jsplit, bx, part);
	});
	launch_sum_partials(st, part, Term::kBlocks, grid, Term::kSums, out, 0, 1.0, n_extra, extra1, extra2);
}

// mark -> delta -> sums of the energy and, with kSums >= 2, of the kept terms into out[0], out[1]; the sum launch clears the map
template <class Term>
inline void launch_pair_term_delta(hipStream_t st, const Term &term, const AtomsDev &at, const Box &bx, const int *mv_slot, const double4 *mv_new, int m,
                                   int *moved_idx, double *part, double *out) {
	const int nt = at.n_pad / kTile;
	const int grid = pair_term_grid((long long)m * nt, Term::kBlocks);
	launch_mark_moved(st, moved_idx, mv_slot, m, 1);
	with_flag(bx.ortho, [&](auto O) {
		hipLaunchKernelGGL((k_pair_term_delta<O.value, Term>), dim3(grid), dim3(kTile), 0, st, term, at.xyzq, at.mf, at.n, nt, bx, mv_slot, mv_new, m, moved_idx, part);
	});
	launch_sum_partials(st, part, Term::kBlocks, grid, std::min(Term::kSums, 2), out, 0, 1.0, 0, 0.0, 0.0, moved_idx, mv_slot, m);
}

} // namespace mpmc
