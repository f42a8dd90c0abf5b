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
// k_crystal: all tile pairs I <= J of the 64-atom tiles, lanes own the i-atoms, the j-tile in LDS read at wave-uniform addresses; equal
// tiles keep i < j.  Small tables give every tile pair to `jsplit` waves that share its j range (crystal_jsplit).  Workgroups take their
// items in a fixed stride and leave one fp64 partial and one count each; k_sum_partials (trial_kernels.h) adds them in a fixed order, so
// a repeated evaluation is bit-identical.
//
// k_crystal_delta: the change under a trial move of m atoms.  One wave per (moved atom t, tile J), lanes own j, old and new geometry; a
// pair of two moved atoms belongs to the one earlier in the move list; same-molecule partners count: O(m N images).
#include "kernels.h"
#include "device_math.h"
#include "trial_kernels.h"

namespace mpmc {

static_assert(S_CRYSTAL_TERMS < S_COUNT, "the scalar block holds the rd_crystal slots");

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

template <bool ORTHO>
__global__ __launch_bounds__(64) void k_crystal(const double4 *__restrict__ xyzq, const double2 *__restrict__ lj, const int2 *__restrict__ mf,
                                                const double *__restrict__ inv_molmass, const double4 *__restrict__ shift,
                                                const int2 *__restrict__ tile_pairs, int n, int n_items, int jsplit, Box bx, CrystalParams cp,
                                                double *__restrict__ part) {
	__shared__ double s_x[kTile], s_y[kTile], s_z[kTile], s_sig[kTile], s_sqe[kTile], s_imm[kTile];
	__shared__ int s_mol[kTile], s_fl[kTile];
	const int l = threadIdx.x;
	const int jw = kTile / jsplit; // j-atoms per item
	double acc = 0.0, terms = 0.0;
	for (int w = blockIdx.x; w < n_items; w += gridDim.x) {
		const int p = w / jsplit, q = w - p * jsplit;
		const int2 tp = tile_pairs[p];
		const int I = tp.x, J = tp.y;
		const int i = I * kTile + l, jl = J * kTile + l;
		const bool i_in = i < n;
		const double4 pi = xyzq[i];
		const double2 li = lj[i];
		const int2 mi = mf[i];
		const double imm_i = cp.fh_order ? inv_molmass[i] : 0.0;
		const double4 pj = xyzq[jl];
		const double2 ljj = lj[jl];
		const int2 mj = mf[jl];
		const double imm_j = cp.fh_order ? inv_molmass[jl] : 0.0;
		const int nj = min(kTile, n - J * kTile);
		__syncthreads(); // (the previous item's readers are done)
		s_x[l] = pj.x, s_y[l] = pj.y, s_z[l] = pj.z;
		s_sig[l] = ljj.x, s_sqe[l] = ljj.y, s_imm[l] = imm_j;
		s_mol[l] = mj.x, s_fl[l] = mj.y;
		__syncthreads();
		int cnt = 0;
		const int j1 = min(nj, (q + 1) * jw);
		for (int jj = q * jw; jj < j1; ++jj) {
			const PairFlags f = pair_flags(mi.x, mi.y, s_mol[jj], s_fl[jj]);
			if (i_in && (I != J || jj > l) && !f.frozen) {
				double sig, eps;
				lj_mix(mi.y, s_fl[jj], li.x, li.y, s_sig[jj], s_sqe[jj], sig, eps);
				acc += crystal_pair<ORTHO>(bx, cp, shift, pi.x - s_x[jj], pi.y - s_y[jj], pi.z - s_z[jj], f, sig, eps, imm_i + s_imm[jj], cnt);
			}
		}
		terms += (double)wave_sum_i(cnt); // (at most 64 * 64 * 3375 per item: no overflow; the running total is a double, exact below 2^53)
	}
	acc = wave_sum(acc);
	if (l == 0) part[blockIdx.x] = acc, part[kCrystalBlocks + blockIdx.x] = terms;
}

// moved_idx[slot] = index of the slot in the moved list, -1 for every other slot (k_mark_moved, trial_kernels.h)
template <bool ORTHO>
__global__ __launch_bounds__(64) void k_crystal_delta(const double4 *__restrict__ xyzq, const double2 *__restrict__ lj, const int2 *__restrict__ mf,
                                                      const double *__restrict__ inv_molmass, const double4 *__restrict__ shift, int n, int n_tiles,
                                                      Box bx, CrystalParams cp, const int *__restrict__ mv_slot, const double4 *__restrict__ mv_new,
                                                      int m, const int *__restrict__ moved_idx, double *__restrict__ part) {
	const int l = threadIdx.x;
	double acc = 0.0, terms = 0.0;
	const int items = m * n_tiles;
	for (int w = blockIdx.x; w < items; w += gridDim.x) {
		const int t = w / n_tiles, J = w - t * n_tiles;
		const int sa = mv_slot[t];
		const double4 pao = xyzq[sa], pan = mv_new[t];
		const double2 la = lj[sa];
		const int2 ma = mf[sa];
		const int j = J * kTile + l;
		const bool j_in = j < n;
		const int mv_j = j_in ? moved_idx[j] : -1;
		const double4 pjo = xyzq[j];
		const double4 pjn = (mv_j >= 0) ? mv_new[mv_j] : pjo;
		const double2 ljj = lj[j];
		const int2 mj = mf[j];
		const double imu = cp.fh_order ? inv_molmass[sa] + inv_molmass[j] : 0.0;
		const PairFlags f = pair_flags(ma.x, ma.y, mj.x, mj.y);
		// partners of the moved atom t: every other atom (its own molecule's too), a moved one only when it comes later in the move list
		const bool ok = j_in && (mv_j < 0 || mv_j > t) && !f.frozen;
		int cnt[2] = {0, 0};
		if (ok) {
			double sig, eps;
			lj_mix(ma.y, mj.y, la.x, la.y, ljj.x, ljj.y, sig, eps);
			double e[2];
#pragma unroll 1
			for (int g = 0; g < 2; g++) { // old geometry, then new (one copy of the pair code)
				const double4 pa = g ? pan : pao, pj = g ? pjn : pjo;
				int c = 0;
				e[g] = crystal_pair<ORTHO>(bx, cp, shift, pa.x - pj.x, pa.y - pj.y, pa.z - pj.z, f, sig, eps, imu, c);
				cnt[g] = c;
			}
			acc += e[1] - e[0];
		}
		terms += (double)wave_sum_i(cnt[1] - cnt[0]);
	}
	acc = wave_sum(acc);
	if (l == 0) part[blockIdx.x] = acc, part[kCrystalBlocks + blockIdx.x] = terms;
}

int crystal_jsplit(int n_tile_pairs) {
	int s = 1;
	while (s < 16 && (long long)n_tile_pairs * s < kCrystalMinItems) s *= 2;
	return s;
}

void launch_crystal(hipStream_t st, const AtomsDev &at, const Box &bx, const CrystalParams &cp, const double4 *shift, const int2 *tile_pairs,
                    int n_tile_pairs, double *part, double *out_e, double *out_terms) {
	const int jsplit = crystal_jsplit(n_tile_pairs);
	const long long items = (long long)n_tile_pairs * jsplit;
	const int grid = (int)std::min<long long>(items, kCrystalBlocks);
	with_flag(bx.ortho, [&](auto O) {
		hipLaunchKernelGGL((k_crystal<O.value>), dim3(grid), dim3(kTile), 0, st, at.xyzq, at.lj, at.mf, at.inv_molmass, shift, tile_pairs, at.n, (int)items, jsplit,
		                   bx, cp, part);
	});
	hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(256), 0, st, part, grid, out_e, 0, 1.0, 0, 0.0, 0.0, nullptr, nullptr, 0);
	hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(256), 0, st, part + kCrystalBlocks, grid, out_terms, 0, 1.0, 0, 0.0, 0.0, nullptr, nullptr, 0);
}

void launch_crystal_delta(hipStream_t st, const AtomsDev &at, const Box &bx, const CrystalParams &cp, const double4 *shift, const int *mv_slot,
                          const double4 *mv_new, int m, int *moved_idx, double *part, double *out2) {
	const int nt = at.n_pad / kTile;
	const int grid = (int)std::min<long long>((long long)m * nt, kCrystalBlocks);
	launch_mark_moved(st, moved_idx, mv_slot, m, 1);
	with_flag(bx.ortho, [&](auto O) {
		hipLaunchKernelGGL((k_crystal_delta<O.value>), dim3(grid), dim3(kTile), 0, st, at.xyzq, at.lj, at.mf, at.inv_molmass, shift, at.n, nt, bx, cp, mv_slot,
		                   mv_new, m, moved_idx, part);
	});
	hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(256), 0, st, part, grid, out2, 0, 1.0, 0, 0.0, 0.0, nullptr, nullptr, 0);
	hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(256), 0, st, part + kCrystalBlocks, grid, out2 + 1, 0, 1.0, 0, 0.0, 0.0, moved_idx, mv_slot, m); // (clears the map)
}

} // namespace mpmc
