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
// Trial moves: the change of that field under a move of m atoms, O(m N), is k_field_delta (trial_kernels.h: thread = atom j, loop over
// the moved atoms, each pair in its new and in its old geometry) with the pair arithmetic WolfField below.
//
// k_palmo_reduce: ef_induced_change = F - E_ind per polarizable atom, with F = -sum A_ij mu_j from one more contraction of the final
// dipoles and E_ind the induced field the last sweep used; the correction -1/2 sum mu . ef_induced_change goes on top of S_POLAR.
#include "kernels.h"
#include "device_math.h"
#include "trial_kernels.h"

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
	with_flags(bx.ortho, wp.a != 0.0, [&](auto O, auto D) {
		hipLaunchKernelGGL((k_wolf_field<O.value, D.value>), dim3(n_tile_pairs), dim3(kTile), 0, st, at, bx, wp, tile_pairs, cls, fpart);
	});
}

// ---- trial moves -------------------------------------------------------------------------------------------------------------------
template <bool DAMPED>
struct WolfField {
	WolfFieldParams wp;
	template <bool ORTHO>
	__device__ __forceinline__ void add(const Box &bx, const double4 &pi, const double4 &pj, const PairFlags &f, double sg, double (&ei)[3],
	                                    double (&ej)[3]) const {
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
};

void launch_wolf_field_delta(hipStream_t st, const AtomsDev &at, const Box &bx, const WolfFieldParams &wp, const int *mv_slot, const double4 *mv_new, int m,
                             int *moved_idx, const double *e_real, double *e_real_trial, double *dk_part) {
	with_flags(bx.ortho, wp.a != 0.0, [&](auto O, auto D) { // (always through the map, whatever the length of the list)
		launch_field_delta<O.value>(st, at, bx, WolfField<D.value>{wp}, true, mv_slot, mv_new, m, moved_idx, e_real, e_real_trial, dk_part);
	});
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
	u = block_sum_256(u, sh);
	if (threadIdx.x == 0) {
		const double corr = -0.5 * u;
		scal[S_PALMO] = corr;
		scal[S_POLAR] += corr;
	}
}
void launch_palmo_reduce(hipStream_t st, const AtomsDev &at, const double *mu, const double *f_new, const double *e_induced, double *change, double *scal) {
	hipLaunchKernelGGL(k_palmo_reduce, dim3(1), dim3(256), 0, st, at, mu, f_new, e_induced, change, scal);
}

} // namespace mpmc
