// trial_kernels.h -- the scaffold the trial-move ("delta") terms share: one pair's energy terms (pair_terms: kernels_delta.hip and
// kernels_exchange.hip), the moved-atom map, the real-space delta-field kernel with its
// finish, the launch sequence around them, and the fixed-order sum of per-workgroup partials.  Included after kernels.h by the HIP
// translation units that launch them (kernels_delta.hip, kernels_wolf_field.hip, kernels_three_body.hip, through exchange_kernels.h
// kernels_exchange.hip and kernels_insert_batch.hip, and through pair_term_walk.h
// kernels_disp.hip, kernels_crystal.hip and kernels_rd_model.hip); the kernels are static, one copy per code object.  A new trial-move
// field term brings its pair arithmetic and calls these; a new pair-sum energy term brings a Term for the two walks of pair_term_walk.h.
#pragma once

#include "kernels.h"
#include "device_math.h"

namespace mpmc {

// u(i,j) of lj() and coulombic_real() (erfc part) for one geometry; adds to e_lj/e_re and the in-cutoff counts with sign sg.
// EXT: the adjacent physics of the pair sweep's extended variant -- coulombic_wolf (:1420-1462) instead of the erfc term, Feynman-Hibbs
// corrections of both terms (:1100-1148, :1521-1557) -- with the same per-pair arithmetic (pair_math.h); imu = 1/M_i + 1/M_j.
template <bool ORTHO, bool EXT>
__device__ __forceinline__ void pair_terms(const Box &bx, const FusedParams &fp, int do_es, const double4 &pi, const double4 &pj, double sig,
                                           double eps, const PairFlags &f, double imu, double sg, double &e_lj, double &e_re, int &n_lj, int &n_es) {
	double ox, oy, oz;
	const double ri2 = min_image_sq<ORTHO>(bx, pi.x - pj.x, pi.y - pj.y, pi.z - pj.z, ox, oy, oz);
	const double ir = fast_rsqrt(ri2);
	if ((ri2 <= bx.t_lj) && !f.rd_excluded) {
		const double sr = sig * ir;
		double s6 = sr * sr * sr;
		s6 *= s6;
		const double t12 = f.attractive_only ? 0.0 : s6 * s6;
		e_lj = fma(sg * 4.0 * eps, t12 - s6, e_lj);
		n_lj += (sg > 0) ? 1 : -1;
		if (EXT && fp.fh_order) e_lj = fma(sg, fh_lj_corr(fp.fh_order, fp.fh_c2, fp.fh_c4, imu, eps, t12, s6, ir), e_lj);
	}
	if (!do_es || f.es_excluded) return;
	if (EXT && fp.wolf) {
		if (ri2 <= bx.t_wolf) { // r < R
			e_re = fma(sg * (pi.w * pj.w), ir - fp.wolf_erfa_over_r - fp.wolf_inv_r2 * (bx.cutoff - ri2 * ir), e_re);
			n_es += (sg > 0) ? 1 : -1;
		}
		return;
	}
	if (ri2 <= bx.t_es) {
		double g;
		const double r = ri2 * ir;
		const double ec = erfc_and_gauss(fp.ewald_alpha * r, g);
		e_re = fma(sg * (pi.w * pj.w) * ec, ir, e_re);
		n_es += (sg > 0) ? 1 : -1;
		if (EXT && fp.fh_order) e_re = fma(sg, fh_es_corr(fp.fh_order, fp.fh_c2, fp.fh_c4, imu, fp.ewald_alpha, ec, g, ri2, r, ir), e_re);
	}
}

// the reduction that ends a trial, one block of 256 threads: the nb block partials { lj, es_real } and their counts, and (do_es) the sum
// over k of w_k |S_k|^2 of the trial structure factors (the caller scales it by 4 pi / V).  k_delta_finish (kernels_delta.hip) and the
// per-candidate finish of kernels_insert_batch.hip both end here, so both add in the same order.  sh: 4 doubles, shc: 256 int64 of LDS.
__device__ __forceinline__ void delta_finish_sums(const double *__restrict__ block_part, const int *__restrict__ block_cnt, int nb, const RecipDev &rc,
                                                  const double4 *__restrict__ sf_trial, int do_es, double *sh, long long *shc, double &s0, double &s1, double &e,
                                                  long long &c0, long long &c1) {
	s0 = 0, s1 = 0, e = 0;
	c0 = 0, c1 = 0;
	for (int b = threadIdx.x; b < nb; b += 256) {
		s0 += block_part[2 * (size_t)b];
		s1 += block_part[2 * (size_t)b + 1];
		c0 += block_cnt[2 * (size_t)b];
		c1 += block_cnt[2 * (size_t)b + 1];
	}
	if (do_es)
		for (int k = threadIdx.x; k < rc.K; k += 256) {
			const double4 sf = sf_trial[k];
			e += rc.w_en[k] * (sf.x * sf.x + sf.y * sf.y);
		}
	s0 = block_sum_256(s0, sh);
	s1 = block_sum_256(s1, sh);
	e = block_sum_256(e, sh);
	c0 = block_count_256(c0, shc);
	c1 = block_count_256(c1, shc);
}

// moved_idx[slot] = index of the slot in the move list (set) or -1 as for every other slot (clear)
static __global__ void k_mark_moved(int *__restrict__ moved_idx, const int *__restrict__ mv_slot, int m, int set) {
	const int k = blockIdx.x * blockDim.x + threadIdx.x;
	if (k < m) moved_idx[mv_slot[k]] = set ? k : -1;
}
inline void launch_mark_moved(hipStream_t st, int *moved_idx, const int *mv_slot, int m, int set) {
	hipLaunchKernelGGL(k_mark_moved, dim3((m + 63) / 64), dim3(64), 0, st, moved_idx, mv_slot, m, set);
}

// ---- polarizable boxes: change of a REAL-SPACE static field that is a pair sum --------------------------------------------------------
// A trial move of m atoms changes, for every atom j, only the terms with a moved partner.  Thread = atom j, loop over the moved atoms k,
// each pair in its new and in its old geometry:
//   E_j += q_k [F(r_j - r_k')  - F(r_j - r_k)],      E_k += q_j [F(r_k' - r_j) - F(r_k - r_j)]   (F odd: the pair is evaluated once)
// PairField (by value, with its parameters) adds sg times one pair's contribution to both atoms: pf.add<ORTHO>(bx, pi, pj, flags, sg, ei, ej).
// The moved atoms' own changes are reduced per wave and land in dk_part[tile][k][3]; k_field_delta_finish adds them up over the tiles.
// moved_idx: the slot -> list-index map, or null: the (short) list is scanned instead.
template <bool ORTHO, class PairField>
__global__ __launch_bounds__(64) void k_field_delta(AtomsDev at, Box bx, PairField pf, const int *__restrict__ mv_slot, const double4 *__restrict__ mv_new,
                                                    int m, const int *__restrict__ moved_idx, const double *__restrict__ e_real,
                                                    double *__restrict__ e_real_trial, double *__restrict__ dk_part /*[n_tiles][m][3]*/) {
	const int j = blockIdx.x * kTile + threadIdx.x; // (j < n_pad: the grid is n_pad / 64 workgroups)
	const double4 pj_old = at.xyzq[j];
	const int2 mj = at.mf[j];
	int kj = -1;
	if (moved_idx) kj = moved_idx[j];
	else
		for (int k = 0; k < m; ++k)
			if (mv_slot[k] == j) kj = k;
	const double4 pj_new = (kj >= 0) ? mv_new[kj] : pj_old;
	const bool j_real = !(mj.y & AF_PAD);
	double ej[3] = {0, 0, 0};
	for (int k = 0; k < m; ++k) {
		double ek[3] = {0, 0, 0};
		if (j_real && !(kj >= 0 && kj <= k)) { // moved-moved pairs once (from the higher list index), never an atom with itself
			const int si = mv_slot[k];
			const int2 mi = at.mf[si];
			const PairFlags f = pair_flags(mi.x, mi.y, mj.x, mj.y);
			if (!f.frozen) {
				pf.template add<ORTHO>(bx, mv_new[k], pj_new, f, 1.0, ek, ej);
				pf.template add<ORTHO>(bx, at.xyzq[si], pj_old, f, -1.0, ek, ej);
			}
		}
		for (int d = 0; d < 3; ++d) ek[d] = wave_sum(ek[d]);
		if (threadIdx.x == 0) {
			double *o = dk_part + ((size_t)blockIdx.x * m + k) * 3;
			o[0] = ek[0];
			o[1] = ek[1];
			o[2] = ek[2];
		}
	}
	for (int d = 0; d < 3; ++d) e_real_trial[3 * (size_t)j + d] = e_real[3 * (size_t)j + d] + ej[d];
}
// the moved atoms' own share: e_real_trial[slot_k] += sum over tiles of dk_part[tile][k]  (one thread per moved atom, tiles in order)
static __global__ __launch_bounds__(64) void k_field_delta_finish(const int *__restrict__ mv_slot, int m, int n_tiles, const double *__restrict__ dk_part,
                                                                  double *__restrict__ e_real_trial) {
	const int k = blockIdx.x * 64 + threadIdx.x;
	if (k >= m) return;
	double s[3] = {0, 0, 0};
	for (int t = 0; t < n_tiles; ++t) {
		const double *q = dk_part + ((size_t)t * m + k) * 3;
		s[0] += q[0];
		s[1] += q[1];
		s[2] += q[2];
	}
	double *o = e_real_trial + 3 * (size_t)mv_slot[k];
	o[0] += s[0];
	o[1] += s[1];
	o[2] += s[2];
}
// mark -> field delta -> finish -> clear; without use_map (short lists) the two map launches drop out and the kernel scans the list
template <bool ORTHO, class PairField>
inline void launch_field_delta(hipStream_t st, const AtomsDev &at, const Box &bx, const PairField &pf, bool use_map, const int *mv_slot,
                               const double4 *mv_new, int m, int *moved_idx, const double *e_real, double *e_real_trial, double *dk_part) {
	const int nt = at.n_pad / kTile;
	if (use_map) launch_mark_moved(st, moved_idx, mv_slot, m, 1);
	hipLaunchKernelGGL((k_field_delta<ORTHO, PairField>), dim3(nt), dim3(kTile), 0, st, at, bx, pf, mv_slot, mv_new, m, use_map ? moved_idx : nullptr, e_real,
	                   e_real_trial, dk_part);
	hipLaunchKernelGGL(k_field_delta_finish, dim3((m + 63) / 64), dim3(64), 0, st, mv_slot, m, nt, dk_part, e_real_trial);
	if (use_map) launch_mark_moved(st, moved_idx, mv_slot, m, 0);
}

// ---- out[a] = the per-workgroup partials of array a (part + a stride) summed in a fixed order (times `scale` when `scaled`; an unscaled
// sum is not multiplied at all), one block per array; n_extra (one array only): out[1], out[2] = extra1, extra2 (values the host keeps and
// the result block carries); mv_slot non-null: block 0 clears the moved-atom map behind a delta launch -----------------------------------
static __global__ __launch_bounds__(256) void k_sum_partials(const double *__restrict__ part, int stride, int nparts, double *__restrict__ out, int scaled,
                                                             double scale, int n_extra, double extra1, double extra2, int *__restrict__ moved_idx,
                                                             const int *__restrict__ mv_slot, int m) {
	__shared__ double sh[4];
	const double *p = part + (size_t)blockIdx.x * stride;
	double s = 0.0;
	for (int b = threadIdx.x; b < nparts; b += 256) s += p[b];
	s = block_sum_256(s, sh);
	if (threadIdx.x == 0) {
		out[blockIdx.x] = scaled ? s * scale : s;
		if (n_extra) out[1] = extra1, out[2] = extra2;
	}
	if (mv_slot && blockIdx.x == 0)
		for (int k = threadIdx.x; k < m; k += 256) moved_idx[mv_slot[k]] = -1;
}
inline void launch_sum_partials(hipStream_t st, const double *part, int stride, int nparts, int n_arrays, double *out, int scaled, double scale, int n_extra = 0,
                                double extra1 = 0.0, double extra2 = 0.0, int *moved_idx = nullptr, const int *mv_slot = nullptr, int m = 0) {
	hipLaunchKernelGGL(k_sum_partials, dim3(n_arrays), dim3(256), 0, st, part, stride, nparts, out, scaled, scale, n_extra, extra1, extra2, moved_idx, mv_slot, m);
}

} // namespace mpmc
