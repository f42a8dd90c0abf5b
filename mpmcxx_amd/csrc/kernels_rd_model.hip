// kernels_rd_model.hip -- the rd model (mpmc_set_rd_model): the pair sum inside the cutoff with another mixing rule (Waldman-Hagler, Halgren,
// C6; reference System::pair_exclusions, src/System.cpp:1069-1177) and another function of r / sigma (System::lj :897-1032,
// lj_buffered_14_7 :1212-1248, dreiding :2098-2215), in place of the LJ sums of the pair kernels.
//
//   E = sum over every pair that is neither rd_excluded nor frozen and passes the form's distance test of rd_pair_energy (pair_math.h)
// at the minimum-image distance (min_image_sq, pair_math.h: the reference's bits in any cell).  The tests are the squared-distance
// thresholds of Box: t_lj (rimg - 1e-12 < cutoff) for the LJ form, t_es (!(rimg > cutoff)) for 14-7 and DREIDING.  The per-atom values
// sp[slot] = (sigma, sigma^2, sigma^3, sigma^6) follow the spatial order (context.cpp: rd_model_ready); sqrt(epsilon) and epsilon are
// AtomsDev::lj's and AtomsDev::eps.
//
// k_rd_model: the tile pairs I <= J of the 64-atom tiles, one wave per tile pair, lanes own the i-atoms, the j-tile in LDS read at
// wave-uniform addresses; equal tiles keep i < j.  A tile pair whose class says CLS_BEYOND_CUTOFF is not walked.  The classes are this
// evaluation's (k_classify, kernels_sym.hip), and their margin is far wider than the 1e-12 A of the LJ test: the class is set for a lower
// bound of the distance of the bounding boxes, itself shortened by 1e-12 of the cell edge, above max(t_lj, t_es) (1 + 1e-9), i.e. about
// 5e-10 cutoff beyond both tests (launch_tile_classes).  Workgroups take tile pairs in a fixed stride and leave three fp64 partials each
// (energy, kept terms, skipped tile pairs; counts as doubles: exact); k_sum_partials (trial_kernels.h) adds each in a fixed order, so a repeated evaluation is
// bit-identical.  No atomics anywhere.
//
// k_rd_model_lrc: the LJ form's pair correction with the mixed parameters over EVERY pair that is not frozen and has eps_ij != 0 and
// sigma_ij != 0 (lj_lrc_corr :1036-1069; intramolecular and excluded pairs count).  It does not factorise over the atoms, so it is a pair
// sum of its own; it depends on the parameters, the flags, the cutoff and the volume only, and the host caches it (context.cpp).
//
// k_rd_model_delta: the change under a trial move of m atoms (slots mv_slot, new positions mv_new; old positions resident).  One wave per
// (moved atom t, tile J), lanes own j; a pair of two moved atoms belongs to the one earlier in the move list: O(m N).
#include "kernels.h"
#include "device_math.h"
#include "trial_kernels.h"

namespace mpmc {

static_assert(S_RDM_SKIPPED < S_COUNT, "the scalar block holds the rd-model slots");

struct ExpFast {
	__device__ __forceinline__ double operator()(double x) const { return exp_fast(x); }
};

__device__ __forceinline__ RdAtom rd_atom(const double4 &sp, double sqe, double e) { return RdAtom{sp.x, sp.y, sp.z, sp.w, sqe, e}; }

// one pair at the raw displacement d = pos_i - pos_j: its energy, 0 outside the form's distance test; cnt += 1 inside it
template <bool ORTHO, int FORM, int MIX>
__device__ __forceinline__ double rdm_pair(const Box &bx, const RdModelParams &rp, double dx, double dy, double dz, const RdAtom &a, const RdAtom &b, double imu,
                                           int &cnt) {
	double ox, oy, oz;
	const double ri2 = min_image_sq<ORTHO>(bx, dx, dy, dz, ox, oy, oz);
	if (!(ri2 <= rp.t_in)) return 0.0;
	cnt += 1;
	const RdMixed m = rd_mix<MIX>(a, b);
	return rd_pair_energy<FORM>(m, ri2, FORM == RD_FORM_LJ ? rp.fh_order : 0, rp.fh_c2, rp.fh_c4, imu, ExpFast{});
}

template <bool ORTHO, int FORM, int MIX>
__global__ __launch_bounds__(64) void k_rd_model(const double4 *__restrict__ xyzq, const double2 *__restrict__ lj, const double *__restrict__ epsv,
                                                 const int2 *__restrict__ mf, const double *__restrict__ inv_molmass, const double4 *__restrict__ sp, const int2 *__restrict__ tile_pairs,
                                                 const int *__restrict__ cls, int n, int n_tile_pairs, Box bx, RdModelParams rp, double *__restrict__ part) {
	__shared__ double s_x[kTile], s_y[kTile], s_z[kTile], s_imm[kTile];
	__shared__ double s_s[kTile], s_s2[kTile], s_s3[kTile], s_s6[kTile], s_sqe[kTile], s_e[kTile];
	__shared__ int s_mol[kTile], s_fl[kTile];
	const int l = threadIdx.x;
	const bool fh = (FORM == RD_FORM_LJ) && rp.fh_order != 0;
	double acc = 0.0, terms = 0.0, skipped = 0.0;
	for (int p = blockIdx.x; p < n_tile_pairs; p += gridDim.x) {
		if (cls && (cls[p] & CLS_BEYOND_CUTOFF)) { // (wave-uniform) the tiles' bounding boxes are further apart than the cutoff: no pair passes
			skipped += 1.0;
			continue;
		}
		const int2 tp = tile_pairs[p];
		const int I = tp.x, J = tp.y;
		const int i = I * kTile + l, jl = J * kTile + l; // (both < n_pad: every per-atom array is padded to whole tiles)
		const bool i_in = i < n;
		const double4 pi = xyzq[i];
		const int2 mi = mf[i];
		const RdAtom ai = rd_atom(sp[i], lj[i].y, epsv[i]);
		const double imm_i = fh ? inv_molmass[i] : 0.0;
		const double4 pj = xyzq[jl];
		const int2 mj = mf[jl];
		const double4 spj = sp[jl];
		const double sqe_j = lj[jl].y, e_j = epsv[jl];
		const double imm_j = fh ? inv_molmass[jl] : 0.0;
		const int nj = min(kTile, n - J * kTile);
		__syncthreads(); // (the previous tile pair's readers are done)
		s_x[l] = pj.x, s_y[l] = pj.y, s_z[l] = pj.z, s_imm[l] = imm_j;
		s_s[l] = spj.x, s_s2[l] = spj.y, s_s3[l] = spj.z, s_s6[l] = spj.w, s_sqe[l] = sqe_j, s_e[l] = e_j;
		s_mol[l] = mj.x, s_fl[l] = mj.y;
		__syncthreads();
		int cnt = 0;
		for (int jj = 0; jj < nj; ++jj) {
			const PairFlags f = pair_flags(mi.x, mi.y, s_mol[jj], s_fl[jj]);
			if (i_in && (I != J || jj > l) && !f.rd_excluded && !f.frozen) {
				const RdAtom bj{s_s[jj], s_s2[jj], s_s3[jj], s_s6[jj], s_sqe[jj], s_e[jj]};
				acc += rdm_pair<ORTHO, FORM, MIX>(bx, rp, pi.x - s_x[jj], pi.y - s_y[jj], pi.z - s_z[jj], ai, bj, imm_i + s_imm[jj], cnt);
			}
		}
		terms += (double)wave_sum_i(cnt); // (at most 64 * 64 per tile pair; the running total is a double, exact below 2^53)
	}
	acc = wave_sum(acc);
	if (l == 0) part[blockIdx.x] = acc, part[kRdModelBlocks + blockIdx.x] = terms, part[2 * kRdModelBlocks + blockIdx.x] = skipped;
}

// every pair once, whatever its distance: the LJ form's pair correction with the mixed parameters
template <int MIX>
__global__ __launch_bounds__(64) void k_rd_model_lrc(const double2 *__restrict__ lj, const double *__restrict__ epsv, const int2 *__restrict__ mf, const double4 *__restrict__ sp,
                                                     const int2 *__restrict__ tile_pairs, int n, int n_tile_pairs, double cutoff, double volume,
                                                     double *__restrict__ part) {
	__shared__ double s_s[kTile], s_s2[kTile], s_s3[kTile], s_s6[kTile], s_sqe[kTile], s_e[kTile];
	__shared__ int s_fl[kTile];
	const int l = threadIdx.x;
	double acc = 0.0;
	for (int p = blockIdx.x; p < n_tile_pairs; p += gridDim.x) {
		const int2 tp = tile_pairs[p];
		const int I = tp.x, J = tp.y;
		const int i = I * kTile + l, jl = J * kTile + l;
		const bool i_in = i < n;
		const int fl_i = mf[i].y;
		const RdAtom ai = rd_atom(sp[i], lj[i].y, epsv[i]);
		const double4 spj = sp[jl];
		const double sqe_j = lj[jl].y, e_j = epsv[jl];
		const int fl_j = mf[jl].y;
		const int nj = min(kTile, n - J * kTile);
		__syncthreads();
		s_s[l] = spj.x, s_s2[l] = spj.y, s_s3[l] = spj.z, s_s6[l] = spj.w, s_sqe[l] = sqe_j, s_e[l] = e_j;
		s_fl[l] = fl_j;
		__syncthreads();
		for (int jj = 0; jj < nj; ++jj) {
			const bool frozen = (fl_i & s_fl[jj] & AF_FROZEN) != 0;
			if (i_in && (I != J || jj > l) && !frozen) {
				const RdAtom bj{s_s[jj], s_s2[jj], s_s3[jj], s_s6[jj], s_sqe[jj], s_e[jj]};
				const RdMixed m = rd_mix<MIX>(ai, bj);
				if (m.eps != 0.0 && m.sigma != 0.0) acc += lrc_term(m.sigma, m.eps, cutoff, volume);
			}
		}
	}
	acc = wave_sum(acc);
	if (l == 0) part[blockIdx.x] = acc;
}

// moved_idx[slot] = index of the slot in the moved list, -1 for every other slot (k_mark_moved, trial_kernels.h)
template <bool ORTHO, int FORM, int MIX>
__global__ __launch_bounds__(64) void k_rd_model_delta(const double4 *__restrict__ xyzq, const double2 *__restrict__ lj, const double *__restrict__ epsv,
                                                       const int2 *__restrict__ mf, const double *__restrict__ inv_molmass, const double4 *__restrict__ sp, int n, int n_tiles, Box bx,
                                                       RdModelParams rp, const int *__restrict__ mv_slot, const double4 *__restrict__ mv_new, int m,
                                                       const int *__restrict__ moved_idx, double *__restrict__ part) {
	const int l = threadIdx.x;
	const bool fh = (FORM == RD_FORM_LJ) && rp.fh_order != 0;
	// a skewed cell's two bases in vector registers: with the pointers, the parameters and the loop state their 18 doubles do not all fit
	// the scalar registers of this loop (k_disp_expansion_delta has the same)
	Box b = bx;
	if (!ORTHO)
		for (int q = 0; q < 9; q++) asm volatile("" : "+v"(b.r[q]), "+v"(b.b[q]));
	double acc = 0.0, terms = 0.0;
	const int items = m * n_tiles;
	for (int w = blockIdx.x; w < items; w += gridDim.x) {
		const int t = w / n_tiles, J = w - t * n_tiles;
		const int sa = mv_slot[t];
		double4 pao = xyzq[sa], pan = mv_new[t];
		const int2 ma = mf[sa];
		RdAtom aa = rd_atom(sp[sa], lj[sa].y, epsv[sa]);
		// (the moved atom's values are wave-uniform: kept in vector registers, the box and the pointers fill the scalar ones)
		asm volatile("" : "+v"(pao.x), "+v"(pao.y), "+v"(pao.z), "+v"(pan.x), "+v"(pan.y), "+v"(pan.z));
		asm volatile("" : "+v"(aa.s), "+v"(aa.s2), "+v"(aa.s3), "+v"(aa.s6), "+v"(aa.sqe), "+v"(aa.e));
		const int j = J * kTile + l; // (< n_pad)
		const bool j_in = j < n;
		const int mv_j = j_in ? moved_idx[j] : -1;
		const double4 pjo = xyzq[j];
		const double4 pjn = (mv_j >= 0) ? mv_new[mv_j] : pjo;
		const int2 mj = mf[j];
		const RdAtom bj = rd_atom(sp[j], lj[j].y, epsv[j]);
		const double imu = fh ? inv_molmass[sa] + inv_molmass[j] : 0.0;
		const PairFlags f = pair_flags(ma.x, ma.y, mj.x, mj.y);
		// partners of the moved atom t: every other atom, a moved one only when it comes later in the move list
		const bool ok = j_in && (mv_j < 0 || mv_j > t) && !f.rd_excluded && !f.frozen;
		int cnt[2] = {0, 0};
		if (ok) {
			double e[2];
#pragma unroll 1
			for (int g = 0; g < 2; g++) { // old geometry, then new (one copy of the pair code)
				const double4 pa = g ? pan : pao, pj = g ? pjn : pjo;
				int c = 0;
				e[g] = rdm_pair<ORTHO, FORM, MIX>(b, rp, pa.x - pj.x, pa.y - pj.y, pa.z - pj.z, aa, bj, imu, c);
				cnt[g] = c;
			}
			acc += e[1] - e[0];
		}
		terms += (double)wave_sum_i(cnt[1] - cnt[0]);
	}
	acc = wave_sum(acc);
	if (l == 0) part[blockIdx.x] = acc, part[kRdModelBlocks + blockIdx.x] = terms;
}

// out[a] = the partials of array a (part + a kRdModelBlocks) in the fixed order of k_sum_partials (trial_kernels.h), one launch per array;
// mv_slot non-null: the last launch clears the moved-atom map behind a delta launch
static void launch_rdm_sums(hipStream_t st, const double *part, int nparts, int n_arrays, double *out, int *moved_idx, const int *mv_slot, int m) {
	for (int a = 0; a < n_arrays; a++) {
		const bool last = (a == n_arrays - 1);
		hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(256), 0, st, part + (size_t)a * kRdModelBlocks, nparts, out + a, 0, 1.0, 0, 0.0, 0.0,
		                   last ? moved_idx : nullptr, last ? mv_slot : nullptr, last ? m : 0);
	}
}

// run-time (form, rule) -> template arguments: f receives two std::integral_constant<int, ...>
template <class F>
static inline void with_rd_model(int form, int mix, F &&f) {
	auto by_mix = [&](auto FORM) {
		switch (mix) {
		case RD_MIX_WALDMAN_HAGLER: f(FORM, std::integral_constant<int, RD_MIX_WALDMAN_HAGLER>{}); break;
		case RD_MIX_HALGREN: f(FORM, std::integral_constant<int, RD_MIX_HALGREN>{}); break;
		case RD_MIX_C6: f(FORM, std::integral_constant<int, RD_MIX_C6>{}); break;
		default: f(FORM, std::integral_constant<int, RD_MIX_LB>{}); break;
		}
	};
	switch (form) {
	case RD_FORM_BUFFERED_14_7: by_mix(std::integral_constant<int, RD_FORM_BUFFERED_14_7>{}); break;
	case RD_FORM_DREIDING: by_mix(std::integral_constant<int, RD_FORM_DREIDING>{}); break;
	default: by_mix(std::integral_constant<int, RD_FORM_LJ>{}); break;
	}
}

int rd_model_grid(long long work_items) { return (int)std::max<long long>(1, std::min<long long>(work_items, kRdModelBlocks)); }

void launch_rd_model(hipStream_t st, const AtomsDev &at, const double4 *sp, const int2 *tile_pairs, const int *cls, int n_tile_pairs, const Box &bx,
                     const RdModelParams &rp, double *part, double *out3) {
	const int grid = rd_model_grid(n_tile_pairs);
	with_rd_model(rp.form, rp.mix, [&](auto F, auto M) {
		with_flag(bx.ortho, [&](auto O) {
			hipLaunchKernelGGL((k_rd_model<O.value, F.value, M.value>), dim3(grid), dim3(kTile), 0, st, at.xyzq, at.lj, at.eps, at.mf, at.inv_molmass, sp, tile_pairs, cls,
			                   at.n, n_tile_pairs, bx, rp, part);
		});
	});
	launch_rdm_sums(st, part, grid, 3, out3, nullptr, nullptr, 0);
}

void launch_rd_model_lrc(hipStream_t st, const AtomsDev &at, const double4 *sp, const int2 *tile_pairs, int n_tile_pairs, int mix, double cutoff,
                         double volume, double *part, double *out) {
	const int grid = rd_model_grid(n_tile_pairs);
	with_rd_model(RD_FORM_LJ, mix, [&](auto, auto M) {
		hipLaunchKernelGGL((k_rd_model_lrc<M.value>), dim3(grid), dim3(kTile), 0, st, at.lj, at.eps, at.mf, sp, tile_pairs, at.n, n_tile_pairs, cutoff, volume, part);
	});
	launch_rdm_sums(st, part, grid, 1, out, nullptr, nullptr, 0);
}

void launch_rd_model_delta(hipStream_t st, const AtomsDev &at, const double4 *sp, const Box &bx, const RdModelParams &rp, const int *mv_slot,
                           const double4 *mv_new, int m, int *moved_idx, double *part, double *out2) {
	const int nt = at.n_pad / kTile;
	const int grid = rd_model_grid((long long)m * nt);
	launch_mark_moved(st, moved_idx, mv_slot, m, 1);
	with_rd_model(rp.form, rp.mix, [&](auto F, auto M) {
		with_flag(bx.ortho, [&](auto O) {
			hipLaunchKernelGGL((k_rd_model_delta<O.value, F.value, M.value>), dim3(grid), dim3(kTile), 0, st, at.xyzq, at.lj, at.eps, at.mf, at.inv_molmass, sp, at.n, nt,
			                   bx, rp, mv_slot, mv_new, m, moved_idx, part);
		});
	});
	launch_rdm_sums(st, part, grid, 2, out2, moved_idx, mv_slot, m); // (clears the map)
}

} // namespace mpmc
