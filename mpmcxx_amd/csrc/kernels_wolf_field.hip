// kernels_wolf_field.hip -- `polar_wolf on`: the static field of the dipole solve as a damped, shifted Wolf sum, reference
// System::thole_field_wolf (src/System.Energy.cpp:3337-3396), and the reduce of the Palmo-Krimm correction (`polar_palmo on`,
// palmo_contraction :3602-3627 and the tail of polar() :2610-2618).
//
// The pairs are those of thole_field_nopbc: different molecules, not both frozen, r - 1e-12 < R (Box::t_lj), r != 0.  Such a pair adds
// q_j f(r) d / r to atom i and -q_i f(r) d / r to atom j, d = r_i - r_j at the minimum image (min_image_sq, pair_math.h), with
//   a > 0:  f(r) = erfc(a r) / r^2 + 2 a / sqrt(pi) exp(-a^2 r^2) / r - [the same at r = R]
//   a = 0:  f(r) = 1 / r^2 - 1 / R^2
// erfc and the Gaussian come from erfc_and_gauss (device_math.h): one polynomial for every a r >= 0, so a r = 43 (a = 1 at the cutoff of
// the 10 000-atom box) is as good as a r = 0.1; beyond a r = 27 both underflow to exact zeros, which is what they are in fp64.  The
// bracket is position independent: the host evaluates it once per launch (WolfFieldParams).
//
// k_wolf_field: one wave per tile pair I <= J of the 64-atom tiles, lanes own the i-atoms, the j-tile staged in LDS.  At step s lane l
// meets j = (l + s) & 63 and carries that j-atom's sum with it: the three sums move one lane per step (rot_from_next), so both sides are
// accumulated in registers without atomics and in a fixed order -- a repeated evaluation gives the same bits.  The sums land in the
// real-space field slots [source tile][atom][3] that k_field_finalize adds up; tile pairs wholly beyond the cutoff publish zeros.
//
// k_wolf_field_delta: the change of that field under a trial move of m atoms, O(m N): thread = atom j, loop over the moved atoms, each
// pair in its new and in its old geometry (the layout of k_delta_field, kernels_delta.hip).
//
// k_palmo_reduce: ef_induced_change = F - E_ind per polarizable atom, with F = -sum A_ij mu_j from one more contraction of the final
// dipoles and E_ind the induced field the last sweep used; the correction -1/2 sum mu . ef_induced_change goes on top of S_POLAR.
#include "kernels.h"
#include "device_math.h"

namespace mpmc {

WolfFieldParams wolf_field_params(double a, double cutoff) {
	WolfFieldParams wp;
	const double rR = 1.0 / cutoff;
	wp.a = a;
	wp.c_gauss = 2.0 * a * kOneOverSqrtPi;
	wp.cutoff_term = (a != 0.0) ? (std::erfc(a * cutoff) * rR * rR + 2.0 * a * kOneOverSqrtPi * std::exp(-a * a * cutoff * cutoff) * rR) : rR * rR; // :3350, :3380
	return wp;
}

// f(r) / r of a pair at squared distance ri2 > 0
template <bool DAMPED>
__device__ __forceinline__ double wolf_fac(const WolfFieldParams &wp, double ri2) {
	const double ir = fast_rsqrt(ri2);
	if (DAMPED) {
		const double r = ri2 * ir;
		double ga;
		const double ec = erfc_and_gauss(wp.a * r, ga);
		const double big = fma(ec, ir, wp.c_gauss * ga) * ir; // :3375
		return (big - wp.cutoff_term) * ir;
	}
	return (ir * ir - wp.cutoff_term) * ir; // :3380
}

template <bool ORTHO, bool DAMPED>
__global__ __launch_bounds__(64) void k_wolf_field(AtomsDev at, Box bx, WolfFieldParams wp, const int2 *__restrict__ tile_pairs, const int *__restrict__ cls,
                                                   double *__restrict__ fpart /*[nt][n_pad][3]*/) {
	__shared__ double s_x[kTile], s_y[kTile], s_z[kTile], s_q[kTile];
	__shared__ int s_mol[kTile], s_fl[kTile];
	const int lane = threadIdx.x;
	const int tp = blockIdx.x;
	const int2 IJ = tile_pairs[tp];
	const bool diag = (IJ.x == IJ.y);
	const int i = IJ.x * kTile + lane, j0 = IJ.y * kTile;
	const size_t nt_pad3 = (size_t)at.n_pad * 3;
	double *oi = fpart + (size_t)IJ.y * nt_pad3 + 3 * (size_t)i;            // i-atoms, contribution of tile J
	double *oj = fpart + (size_t)IJ.x * nt_pad3 + 3 * (size_t)(j0 + lane); // j-atoms, contribution of tile I
	if (cls[tp] & CLS_BEYOND_CUTOFF) { // (wave-uniform; never a diagonal tile pair) zeros keep the fixed-shape sum of the slots valid
		oi[0] = oi[1] = oi[2] = 0.0;
		oj[0] = oj[1] = oj[2] = 0.0;
		return;
	}
	const double4 pi = at.xyzq[i];
	const int2 mi = at.mf[i];
	{
		const double4 pj = at.xyzq[j0 + lane];
		const int2 mj = at.mf[j0 + lane];
		s_x[lane] = pj.x, s_y[lane] = pj.y, s_z[lane] = pj.z, s_q[lane] = pj.w;
		s_mol[lane] = mj.x, s_fl[lane] = mj.y;
	}
	__syncthreads();
	const bool i_in = i < at.n;
	double ex = 0, ey = 0, ez = 0, gx = 0, gy = 0, gz = 0;
	for (int s = 0; s < kTile; ++s) {
		const int jj = (lane + s) & (kTile - 1);
		const PairFlags f = pair_flags(mi.x, mi.y, s_mol[jj], s_fl[jj]);
		double ox, oy, oz;
		const double ri2 = min_image_sq<ORTHO>(bx, pi.x - s_x[jj], pi.y - s_y[jj], pi.z - s_z[jj], ox, oy, oz);
		// (a diagonal tile pair meets every ordered pair of its 64 atoms and keeps the i side only)
		const bool ok = i_in && (j0 + jj < at.n) && !f.intra && !f.frozen && (ri2 <= bx.t_lj) && (ri2 != 0.0) && !(diag && s == 0);
		const double fv = wolf_fac<DAMPED>(wp, ok ? ri2 : 1.0); // (no branch: a masked pair is evaluated at r = 1 and dropped)
		const double fac = ok ? fv : 0.0;
		const double fj = fac * s_q[jj], fi = fac * pi.w;
		ex = fma(fj, ox, ex);
		ey = fma(fj, oy, ey);
		ez = fma(fj, oz, ez);
		gx = fma(-fi, ox, gx);
		gy = fma(-fi, oy, gy);
		gz = fma(-fi, oz, gz);
		gx = rot_from_next(gx); // the sums of j travel with j: after this step lane l holds those of (l + s + 1) & 63
		gy = rot_from_next(gy);
		gz = rot_from_next(gz);
	}
	oi[0] = ex;
	oi[1] = ey;
	oi[2] = ez;
	if (!diag) { // (64 rotations: lane l holds the sums of j = l again)
		oj[0] = gx;
		oj[1] = gy;
		oj[2] = gz;
	}
}

void launch_wolf_field(hipStream_t st, const AtomsDev &at, const Box &bx, const WolfFieldParams &wp, const int2 *tile_pairs, const int *cls,
                       int n_tile_pairs, double *fpart) {
	if (n_tile_pairs <= 0) return;
#define MPMC_WF(O, D) hipLaunchKernelGGL((k_wolf_field<O, D>), dim3(n_tile_pairs), dim3(kTile), 0, st, at, bx, wp, tile_pairs, cls, fpart)
	if (bx.ortho) {
		if (wp.a != 0.0) MPMC_WF(true, true);
		else MPMC_WF(true, false);
	} else {
		if (wp.a != 0.0) MPMC_WF(false, true);
		else MPMC_WF(false, false);
	}
#undef MPMC_WF
}

// ---- trial moves -------------------------------------------------------------------------------------------------------------------
template <bool ORTHO, bool DAMPED>
__device__ __forceinline__ void wolf_field_pair(const Box &bx, const WolfFieldParams &wp, const double4 &pi, const double4 &pj, const PairFlags &f, double sg,
                                                double (&ei)[3], double (&ej)[3]) {
	double ox, oy, oz;
	const double ri2 = min_image_sq<ORTHO>(bx, pi.x - pj.x, pi.y - pj.y, pi.z - pj.z, ox, oy, oz);
	if (ri2 == 0.0 || f.intra || !(ri2 <= bx.t_lj)) return; // :3361-3368
	const double fac = wolf_fac<DAMPED>(wp, ri2);
	const double fj = sg * fac * pj.w, fi = sg * fac * pi.w;
	ei[0] = fma(fj, ox, ei[0]);
	ei[1] = fma(fj, oy, ei[1]);
	ei[2] = fma(fj, oz, ei[2]);
	ej[0] = fma(-fi, ox, ej[0]);
	ej[1] = fma(-fi, oy, ej[1]);
	ej[2] = fma(-fi, oz, ej[2]);
}

// moved_idx[slot] = index of the slot in the move list, -1 for every other slot (k_wolf_mark sets and clears it)
template <bool ORTHO, bool DAMPED>
__global__ __launch_bounds__(64) void k_wolf_field_delta(AtomsDev at, Box bx, WolfFieldParams wp, const int *__restrict__ mv_slot,
                                                         const double4 *__restrict__ mv_new, int m, const int *__restrict__ moved_idx,
                                                         const double *__restrict__ e_real, double *__restrict__ e_real_trial,
                                                         double *__restrict__ dk_part /*[n_tiles][m][3]*/) {
	const int j = blockIdx.x * kTile + threadIdx.x; // (j < n_pad: the grid is n_pad / 64 workgroups)
	const double4 pj_old = at.xyzq[j];
	const int2 mj = at.mf[j];
	const int kj = moved_idx[j];
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
				wolf_field_pair<ORTHO, DAMPED>(bx, wp, mv_new[k], pj_new, f, 1.0, ek, ej);
				wolf_field_pair<ORTHO, DAMPED>(bx, wp, at.xyzq[si], pj_old, f, -1.0, ek, ej);
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
__global__ void k_wolf_mark(int *__restrict__ moved_idx, const int *__restrict__ mv_slot, int m, int set) {
	const int k = blockIdx.x * blockDim.x + threadIdx.x;
	if (k < m) moved_idx[mv_slot[k]] = set ? k : -1;
}
// the moved atoms' own share: e_real_trial[slot_k] += sum over the tiles of dk_part[tile][k], tiles in order
__global__ __launch_bounds__(64) void k_wolf_field_delta_finish(const int *__restrict__ mv_slot, int m, int n_tiles, const double *__restrict__ dk_part,
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

void launch_wolf_field_delta(hipStream_t st, const AtomsDev &at, const Box &bx, const WolfFieldParams &wp, const int *mv_slot, const double4 *mv_new, int m,
                             int *moved_idx, const double *e_real, double *e_real_trial, double *dk_part) {
	const int nt = at.n_pad / kTile;
	const dim3 mg((m + 63) / 64), mb(64);
	hipLaunchKernelGGL(k_wolf_mark, mg, mb, 0, st, moved_idx, mv_slot, m, 1);
#define MPMC_WD(O, D) hipLaunchKernelGGL((k_wolf_field_delta<O, D>), dim3(nt), dim3(kTile), 0, st, at, bx, wp, mv_slot, mv_new, m, moved_idx, e_real, e_real_trial, dk_part)
	if (bx.ortho) {
		if (wp.a != 0.0) MPMC_WD(true, true);
		else MPMC_WD(true, false);
	} else {
		if (wp.a != 0.0) MPMC_WD(false, true);
		else MPMC_WD(false, false);
	}
#undef MPMC_WD
	hipLaunchKernelGGL(k_wolf_field_delta_finish, mg, mb, 0, st, mv_slot, m, nt, dk_part, e_real_trial);
	hipLaunchKernelGGL(k_wolf_mark, mg, mb, 0, st, moved_idx, mv_slot, m, 0);
}

// ---- Palmo-Krimm ---------------------------------------------------------------------------------------------------------------------
// one workgroup, fixed-order sums (the shape of k_polar_energy, which runs in front of it and has written S_POLAR)
__global__ __launch_bounds__(256) void k_palmo_reduce(AtomsDev at, const double *__restrict__ mu, const double *__restrict__ f_new,
                                                      const double *__restrict__ e_induced, double *__restrict__ change, double *__restrict__ scal) {
	__shared__ double sh[4];
	double u = 0;
	for (int i = threadIdx.x; i < at.n_pad; i += 256) {
		const size_t b = 3 * (size_t)i;
		const bool live = (i < at.n) && (at.alpha[i] != 0.0);
		double c[3];
		for (int p = 0; p < 3; ++p) {
			c[p] = live ? f_new[b + p] - e_induced[b + p] : 0.0; // :3616-3622
			change[b + p] = c[p];
		}
		if (live) u += ((mu[b] * c[0]) + mu[b + 1] * c[1]) + mu[b + 2] * c[2]; // :2615
	}
	u = wave_sum(u);
	if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = u;
	__syncthreads();
	if (threadIdx.x == 0) {
		const double corr = -0.5 * (((sh[0] + sh[1]) + sh[2]) + sh[3]);
		scal[S_PALMO] = corr;
		scal[S_POLAR] += corr;
	}
}
void launch_palmo_reduce(hipStream_t st, const AtomsDev &at, const double *mu, const double *f_new, const double *e_induced, double *change, double *scal) {
	hipLaunchKernelGGL(k_palmo_reduce, dim3(1), dim3(256), 0, st, at, mu, f_new, e_induced, change, scal);
}

} // namespace mpmc
