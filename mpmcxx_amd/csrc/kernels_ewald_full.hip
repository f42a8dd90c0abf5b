// kernels_ewald_full.hip -- `polar_ewald_full on`: the induced field of the dipole solve as an Ewald sum, reference System::ewald_full
// (src/System.Energy.cpp:2785-2830) with induced_real_term (:3046-3104), induced_recip_term (:2975-3042) and induced_corr_term
// (:3120-3143).  The static field is the one of `polar_ewald on` (recip_term + real_term: the existing field kernels); what is here runs
// behind it.
//
// Once per evaluation:
//   k_pef_fill    one wave per tile pair I <= J of the 64-atom tiles.  Lane l owns i = 64 I + l and meets j = 64 J + ((l + s) & 63) at step
//                 s; the pair's factors (-s1 / r^3, 3 s2 / r^5) go to store[tp][64 s + l], 16 bytes per pair, zeros for a pair outside the
//                 predicate (alpha_i != 0, alpha_j != 0, !(rimg > R): Box::t_es on the squared minimum-image distance of min_image_sq, the
//                 reference's association order).  cnt[tp] = pairs inside the predicate, each unordered pair once; a tile pair without
//                 any writes nothing and is never read, and one whose tiles' bounding boxes lie beyond R (CLS_BEYOND_CUTOFF of this
//                 evaluation's classes) is not walked at all.  erfc and exp are the library's (ocml): the store is filled once, and
//                 s1, s2 are differences of numbers near 1 at short range.
//   k_pef_phases  (cos, sin)(k . r_i) for every k of the hemisphere and every atom, raw positions: [K][n_pad] double2.  The phases do not
//                 change between the passes.  (Without the table -- phases == null, the measurement switch "pef_phase_table" = 0 -- the
//                 two kernels below form the same sincos per (k, atom) and pass: the same bits, profiles/ewald_full.txt has the A/B.)
// Once per pass:
//   k_pef_contract  streams the store in the order it was written: T = b d d^T + a I with d recomputed from the positions (the store
//                 holds the two scalars of a pair, as the Thole tensor store does).  The i side is accumulated per lane, the j side
//                 travels with j from lane to lane (rot_from_next), so both land without atomics and in a fixed order in the slots
//                 part[source tile][atom][3]; a tile pair without a pair inside the predicate publishes zeros.
//   k_pef_sf      one workgroup per k: Pc = sum_j (k . mu_j) cos(k . r_j), Ps likewise with sin, by a fixed-order block sum; one more
//                 workgroup sums the dipoles (the correction term's total).
//   k_pef_finish  one workgroup per tile, eight waves that share the slots and the k vectors of its 64 atoms and are added in wave order
//                 (one thread per atom, walking 709 k vectors and 157 slots alone, took 0.24 ms per pass at 10 000 atoms): the slots,
//                 the reciprocal field with w_p = (8 pi / V) kw_z (the reference's scalar weight) or (8 pi / V) kw_p
//                 (MPMC_PEF_VECTOR_KWEIGHT), the correction, E_ind, mu = alpha (E0 + E_ind), and whether any component moved by more
//                 than the allowed amount (are_we_done_yet :3215-3239).
#include "kernels.h"
#include "device_math.h"

namespace mpmc {

template <bool ORTHO>
__global__ __launch_bounds__(64) void k_pef_fill(AtomsDev at, Box bx, double a, double l, const int2 *__restrict__ tile_pairs,
                                                 const int *__restrict__ cls, double2 *__restrict__ store, int *__restrict__ cnt) {
	__shared__ double s_x[kTile], s_y[kTile], s_z[kTile], s_al[kTile];
	const int lane = threadIdx.x;
	const int tp = blockIdx.x;
	const int2 IJ = tile_pairs[tp];
	const bool diag = (IJ.x == IJ.y);
	const int i = IJ.x * kTile + lane, j0 = IJ.y * kTile;
	if (cls && (cls[tp] & CLS_BEYOND_CUTOFF)) { // (wave-uniform) the tiles' bounding boxes are further apart than R: no pair passes
		if (lane == 0) cnt[tp] = 0;
		return;
	}
	const double4 pi = at.xyzq[i];
	const bool i_ok = (i < at.n) && (at.alpha[i] != 0.0);
	{
		const double4 pj = at.xyzq[j0 + lane];
		s_x[lane] = pj.x, s_y[lane] = pj.y, s_z[lane] = pj.z;
		s_al[lane] = (j0 + lane < at.n) ? at.alpha[j0 + lane] : 0.0;
	}
	__syncthreads();
	// first walk: the predicate alone (a tile pair wholly outside it leaves the store untouched)
	int mine = 0;
	for (int s = 0; s < kTile; ++s) {
		const int jj = (lane + s) & (kTile - 1);
		double ox, oy, oz;
		const double ri2 = min_image_sq<ORTHO>(bx, pi.x - s_x[jj], pi.y - s_y[jj], pi.z - s_z[jj], ox, oy, oz);
		const bool ok = i_ok && (s_al[jj] != 0.0) && (ri2 <= bx.t_es) && !(diag && s == 0);
		mine += (ok && (!diag || lane < jj)) ? 1 : 0; // (a diagonal tile pair meets every unordered pair twice)
	}
	const int total = __shfl(wave_sum_i(mine), 0, 64);
	if (lane == 0) cnt[tp] = total;
	if (total == 0) return;
	double2 *out = store + (size_t)tp * (kTile * kTile);
	const double c = kOneOverSqrtPi;
	for (int s = 0; s < kTile; ++s) {
		const int jj = (lane + s) & (kTile - 1);
		double ox, oy, oz;
		const double ri2 = min_image_sq<ORTHO>(bx, pi.x - s_x[jj], pi.y - s_y[jj], pi.z - s_z[jj], ox, oy, oz);
		const bool ok = i_ok && (s_al[jj] != 0.0) && (ri2 <= bx.t_es) && !(diag && s == 0);
		double2 v = make_double2(0.0, 0.0);
		if (ok) { // :3070-3087
			const double r = sqrt(ri2);
			const double ir = 1.0 / r, ir3 = ir * ir * ir, ir5 = ir * ir * ir3;
			const double e = erfc(a * r), g = exp(-a * a * r * r);
			const double t = l * r, et = exp(-t);
			const double d2 = 1.0 + t + 0.5 * t * t;
			const double d3 = d2 + t * t * t / 6.0;
			const double common = e + 2.0 * a * r * c * g;
			const double s1 = common - d2 * et;
			const double s2 = common + 4.0 * a * a * a * r * r * r / 3.0 * c * g - d3 * et;
			v = make_double2(-s1 * ir3, 3.0 * s2 * ir5);
		}
		out[s * kTile + lane] = v;
	}
}

__global__ __launch_bounds__(256) void k_pef_count(const int *__restrict__ cnt, int n_tile_pairs, long long *__restrict__ out) {
	__shared__ long long shc[256];
	long long v = 0;
	for (int t = threadIdx.x; t < n_tile_pairs; t += 256) v += cnt[t];
	v = block_count_256(v, shc);
	if (threadIdx.x == 0) out[0] = v;
}

// (cos, sin)(k . r): the one expression of the phase table and of the kernels that recompute it (phases == null: the A/B of the table)
__device__ __forceinline__ double2 pef_phase(const double4 &kv, const double4 &p) {
	const double ph = ((kv.x * p.x) + kv.y * p.y) + kv.z * p.z;
	double sn, cs;
	sincos(ph, &sn, &cs);
	return make_double2(cs, sn);
}

__global__ __launch_bounds__(256) void k_pef_phases(AtomsDev at, const double4 *__restrict__ kvec, double2 *__restrict__ phases) {
	const int i = blockIdx.x * 256 + threadIdx.x;
	const int k = blockIdx.y;
	if (i >= at.n_pad) return;
	phases[(size_t)k * at.n_pad + i] = (i < at.n) ? pef_phase(kvec[k], at.xyzq[i]) : make_double2(0.0, 0.0);
}

template <bool ORTHO>
__global__ __launch_bounds__(64) void k_pef_contract(AtomsDev at, Box bx, const double *__restrict__ mu, const int2 *__restrict__ tile_pairs,
                                                     const int *__restrict__ cnt, const double2 *__restrict__ store, double *__restrict__ part /*[nt][n_pad][3]*/) {
	__shared__ double s_x[kTile], s_y[kTile], s_z[kTile], s_mx[kTile], s_my[kTile], s_mz[kTile];
	const int lane = threadIdx.x;
	const int tp = blockIdx.x;
	const int2 IJ = tile_pairs[tp];
	const bool diag = (IJ.x == IJ.y);
	const int i = IJ.x * kTile + lane, j0 = IJ.y * kTile;
	const size_t nt_pad3 = (size_t)at.n_pad * 3;
	double *oi = part + (size_t)IJ.y * nt_pad3 + 3 * (size_t)i;            // i-atoms, contribution of tile J
	double *oj = part + (size_t)IJ.x * nt_pad3 + 3 * (size_t)(j0 + lane); // j-atoms, contribution of tile I
	if (cnt[tp] == 0) { // (wave-uniform) zeros keep the fixed-shape sum of the slots valid
		oi[0] = oi[1] = oi[2] = 0.0;
		if (!diag) oj[0] = oj[1] = oj[2] = 0.0;
		return;
	}
	const double4 pi = at.xyzq[i];
	const double mix = mu[3 * (size_t)i], miy = mu[3 * (size_t)i + 1], miz = mu[3 * (size_t)i + 2];
	{
		const double4 pj = at.xyzq[j0 + lane];
		const size_t b = 3 * (size_t)(j0 + lane);
		s_x[lane] = pj.x, s_y[lane] = pj.y, s_z[lane] = pj.z;
		s_mx[lane] = mu[b], s_my[lane] = mu[b + 1], s_mz[lane] = mu[b + 2];
	}
	__syncthreads();
	const double2 *in = store + (size_t)tp * (kTile * kTile);
	double ex = 0, ey = 0, ez = 0, gx = 0, gy = 0, gz = 0;
	for (int s = 0; s < kTile; ++s) {
		const int jj = (lane + s) & (kTile - 1);
		const double2 ab = ld_stream<true>(in + s * kTile + lane); // (zeros for a pair outside the predicate)
		double ox, oy, oz;
		(void)min_image_sq<ORTHO>(bx, pi.x - s_x[jj], pi.y - s_y[jj], pi.z - s_z[jj], ox, oy, oz);
		const double mjx = s_mx[jj], mjy = s_my[jj], mjz = s_mz[jj];
		const double dj = ab.y * (((ox * mjx) + oy * mjy) + oz * mjz); // b (d . mu_j)
		const double di = ab.y * (((ox * mix) + oy * miy) + oz * miz); // b (d . mu_i)
		ex += dj * ox + ab.x * mjx;
		ey += dj * oy + ab.x * mjy;
		ez += dj * oz + ab.x * mjz;
		gx += di * ox + ab.x * mix;
		gy += di * oy + ab.x * miy;
		gz += di * oz + ab.x * miz;
		gx = rot_from_next(gx); // the sums of j travel with j: after this step lane l holds those of (l + s + 1) & 63
		gy = rot_from_next(gy);
		gz = rot_from_next(gz);
	}
	oi[0] = ex;
	oi[1] = ey;
	oi[2] = ez;
	if (!diag) { // (a diagonal tile pair meets every ordered pair of its 64 atoms and keeps the i side only)
		oj[0] = gx;
		oj[1] = gy;
		oj[2] = gz;
	}
}

// psum[2 k] = Pc, psum[2 k + 1] = Ps for k < K; psum[2 K .. 2 K + 2] = sum_j mu_j
template <bool CACHED>
__global__ __launch_bounds__(256) void k_pef_sf(AtomsDev at, const double4 *__restrict__ kvec, int K, const double2 *__restrict__ phases,
                                                const double *__restrict__ mu, double *__restrict__ psum) {
	__shared__ double sh[4];
	const int k = blockIdx.x;
	if (k == K) {
		double tx = 0, ty = 0, tz = 0;
		for (int j = threadIdx.x; j < at.n; j += 256) {
			tx += mu[3 * (size_t)j];
			ty += mu[3 * (size_t)j + 1];
			tz += mu[3 * (size_t)j + 2];
		}
		tx = block_sum_256(tx, sh);
		ty = block_sum_256(ty, sh);
		tz = block_sum_256(tz, sh);
		if (threadIdx.x == 0) psum[2 * K] = tx, psum[2 * K + 1] = ty, psum[2 * K + 2] = tz;
		return;
	}
	const double4 kv = kvec[k];
	const double2 *ph = phases + (size_t)k * at.n_pad;
	double pc = 0, ps = 0;
	for (int j = threadIdx.x; j < at.n; j += 256) {
		const size_t b = 3 * (size_t)j;
		const double km = ((kv.x * mu[b]) + kv.y * mu[b + 1]) + kv.z * mu[b + 2];
		const double2 cs = CACHED ? ph[j] : pef_phase(kv, at.xyzq[j]);
		pc += km * cs.x;
		ps += km * cs.y;
	}
	pc = block_sum_256(pc, sh);
	ps = block_sum_256(ps, sh);
	if (threadIdx.x == 0) psum[2 * k] = pc, psum[2 * k + 1] = ps;
}

constexpr int kPefGroups = 8; // waves of a finish workgroup: each takes every eighth k vector and every eighth slot of its tile's 64 atoms
// RELAX (`polar_sor` / `polar_esor`, new_dipoles :3196-3204): new_mu itself becomes w_new new_mu + w_old old_mu, so the verdict compares the
// blend with the old dipoles.  The plain instantiation never looks at the weights.
template <bool CACHED, bool RELAX>
__device__ __forceinline__ void pef_finish_block(const AtomsDev &at, const EwaldFullParams &ep, const double *__restrict__ e_static, const double *__restrict__ part,
                                                 int n_tiles, const double2 *__restrict__ phases, const double4 *__restrict__ kvec,
                                                 const double4 *__restrict__ kw, int K, const double *__restrict__ psum,
                                                 const double *__restrict__ mu_old, double *__restrict__ mu_new, double *__restrict__ e_induced,
                                                 int *__restrict__ not_done, double w_new = 1.0, double w_old = 0.0) {
	__shared__ double sh[kPefGroups][6][kTile];
	const int a = threadIdx.x & (kTile - 1), g = threadIdx.x >> 6;
	const int i = blockIdx.x * kTile + a; // (< n_pad: one workgroup per tile)
	const size_t b = 3 * (size_t)i;
	double e[3] = {0.0, 0.0, 0.0}, r[3] = {0.0, 0.0, 0.0};
	if (i < at.n) {
		const size_t nt_pad3 = (size_t)at.n_pad * 3;
		for (int t = g; t < n_tiles; t += kPefGroups) // the real-space slots
			for (int p = 0; p < 3; ++p) e[p] += part[(size_t)t * nt_pad3 + b + p];
		const double4 pos = at.xyzq[i];
		for (int k = g; k < K; k += kPefGroups) {
			const double2 cs = CACHED ? phases[(size_t)k * at.n_pad + i] : pef_phase(kvec[k], pos);
			const double4 w = kw[k];
			const double f = -cs.y * psum[2 * k + 1] - cs.x * psum[2 * k]; // :3033
			r[0] += (ep.vector_weight ? w.x : w.z) * f;
			r[1] += (ep.vector_weight ? w.y : w.z) * f;
			r[2] += w.z * f;
		}
	}
	for (int p = 0; p < 3; ++p) sh[g][p][a] = e[p], sh[g][3 + p][a] = r[p];
	__syncthreads();
	if (g != 0) return;
	if (i >= at.n) {
		for (int p = 0; p < 3; ++p) mu_new[b + p] = 0.0, e_induced[b + p] = 0.0;
		return;
	}
	bool broke = false;
	for (int p = 0; p < 3; ++p) {
		double ep_real = sh[0][p][a], ep_recip = sh[0][3 + p][a];
		for (int q = 1; q < kPefGroups; ++q) ep_real += sh[q][p][a], ep_recip += sh[q][3 + p][a]; // the groups in order
		const double m = mu_old[b + p];
		const double ei = (ep_real + ep.recip_scale * ep_recip) + (ep.c_total * psum[2 * K + p] + ep.c_self * m); // :3140
		e_induced[b + p] = ei;
		double nm = at.alpha[i] * (e_static[b + p] + ei); // :3203
		if constexpr (RELAX) nm = relax_blend(w_new, w_old, nm, m);
		mu_new[b + p] = nm;
		const double d = nm - m;
		broke = broke || (d * d > ep.allowed_sqerr);
	}
	if (not_done && broke) *not_done = 1; // (every writer stores the same value)
}
template <bool CACHED>
__global__ __launch_bounds__(kTile * kPefGroups) void k_pef_finish(AtomsDev at, EwaldFullParams ep, const double *__restrict__ e_static, const double *__restrict__ part,
                                                                   int n_tiles, const double2 *__restrict__ phases, const double4 *__restrict__ kvec,
                                                                   const double4 *__restrict__ kw, int K, const double *__restrict__ psum,
                                                                   const double *__restrict__ mu_old, double *__restrict__ mu_new, double *__restrict__ e_induced,
                                                                   int *__restrict__ not_done) {
	pef_finish_block<CACHED, false>(at, ep, e_static, part, n_tiles, phases, kvec, kw, K, psum, mu_old, mu_new, e_induced, not_done);
}
template <bool CACHED>
__global__ __launch_bounds__(kTile * kPefGroups) void k_pef_finish_relax(AtomsDev at, EwaldFullParams ep, const double *__restrict__ e_static,
                                                                         const double *__restrict__ part, int n_tiles, const double2 *__restrict__ phases,
                                                                         const double4 *__restrict__ kvec, const double4 *__restrict__ kw, int K,
                                                                         const double *__restrict__ psum, const double *__restrict__ mu_old,
                                                                         double *__restrict__ mu_new, double *__restrict__ e_induced, int *__restrict__ not_done,
                                                                         RelaxWeights w) {
	pef_finish_block<CACHED, true>(at, ep, e_static, part, n_tiles, phases, kvec, kw, K, psum, mu_old, mu_new, e_induced, not_done, w.w_new, w.w_old);
}

void launch_pef_fill(hipStream_t st, const AtomsDev &at, const Box &bx, double ewald_a, double polar_damp, const int2 *tile_pairs, const int *cls,
                     int n_tile_pairs, double2 *store, int *cnt, long long *n_pairs_out) {
	if (n_tile_pairs <= 0) return;
	with_flag(bx.ortho, [&](auto O) {
		hipLaunchKernelGGL((k_pef_fill<O.value>), dim3(n_tile_pairs), dim3(kTile), 0, st, at, bx, ewald_a, polar_damp, tile_pairs, cls, store, cnt);
	});
	hipLaunchKernelGGL(k_pef_count, dim3(1), dim3(256), 0, st, cnt, n_tile_pairs, n_pairs_out);
}
void launch_pef_phases(hipStream_t st, const AtomsDev &at, const double4 *kvec, int K, double2 *phases) {
	if (K <= 0) return;
	hipLaunchKernelGGL(k_pef_phases, dim3((at.n_pad + 255) / 256, K), dim3(256), 0, st, at, kvec, phases);
}
void launch_pef_contract(hipStream_t st, const AtomsDev &at, const Box &bx, const double *mu, const int2 *tile_pairs, int n_tile_pairs, const int *cnt,
                         const double2 *store, double *part) {
	if (n_tile_pairs <= 0) return;
	with_flag(bx.ortho, [&](auto O) {
		hipLaunchKernelGGL((k_pef_contract<O.value>), dim3(n_tile_pairs), dim3(kTile), 0, st, at, bx, mu, tile_pairs, cnt, store, part);
	});
}
void launch_pef_sf(hipStream_t st, const AtomsDev &at, const double4 *kvec, int K, const double2 *phases, const double *mu, double *psum) {
	with_flag(phases != nullptr, [&](auto C) { hipLaunchKernelGGL((k_pef_sf<C.value>), dim3(K + 1), dim3(256), 0, st, at, kvec, K, phases, mu, psum); });
}
void launch_pef_finish(hipStream_t st, const AtomsDev &at, const EwaldFullParams &ep, const double *e_static, const double *part, int n_tiles,
                       const double2 *phases, const double4 *kvec, const double4 *kw, int K, const double *psum, const double *mu_old, double *mu_new,
                       double *e_induced, int *not_done, const RelaxWeights *relax) {
	with_flag(phases != nullptr, [&](auto C) {
		if (relax)
			hipLaunchKernelGGL((k_pef_finish_relax<C.value>), dim3(at.n_pad / kTile), dim3(kTile * kPefGroups), 0, st, at, ep, e_static, part, n_tiles, phases, kvec, kw, K,
			                   psum, mu_old, mu_new, e_induced, not_done, *relax);
		else
			hipLaunchKernelGGL((k_pef_finish<C.value>), dim3(at.n_pad / kTile), dim3(kTile * kPefGroups), 0, st, at, ep, e_static, part, n_tiles, phases, kvec, kw, K, psum,
			                   mu_old, mu_new, e_induced, not_done);
	});
}

} // namespace mpmc
