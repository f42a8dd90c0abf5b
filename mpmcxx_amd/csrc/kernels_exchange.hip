// kernels_exchange.hip -- exchange moves: the energy change of inserting or removing ONE molecule of m atoms, O(m N) + O(K m).
//
// A uVT insert / remove move and a Gibbs transfer change the composition, not the positions of atoms that stay.  The change is the same
// object as a displacement's (kernels_delta.hip), evaluated once instead of in an old and a new geometry:
//   E_trial = E_accepted + sg [ sum_{k in molecule, j resident, j not in molecule} u(k,j) + sum_{k<l in molecule} u(k,l) ]
//             + (E_recip[S + sg dS] - E_recip[S]) + change of the position-independent terms (host, trial.cpp),    sg = +1 | -1
// with the per-pair arithmetic (pair_terms, trial_kernels.h), the predicates (pair_flags) and the minimum image of the displacement kernel,
// so the in-cutoff counts come out as a full evaluation's.  The molecule is a staged list of XchAtom records (kernels.h) in both
// directions: an inserted molecule has no slots yet, a removed one is recognised among the resident atoms by its molecule id.  The block
// partials, their reduction, the reciprocal energy and the post of the result are launch_delta's (launch_delta_finish).
#include "kernels.h"
#include "device_math.h"
#include "trial_kernels.h"

namespace mpmc {

// thread = resident slot j of tile `tile`; loops over the molecule's atoms
template <bool ORTHO, bool EXT>
__device__ __forceinline__ void exchange_pairs_tile(const AtomsDev &at, const Box &bx, const FusedParams &fp, int do_es, const XchAtom *__restrict__ mol, int m,
                                                    double sg, double *__restrict__ block_part, int *__restrict__ block_cnt, int tile) {
	const int j = tile * kTile + threadIdx.x;
	const double4 pj = at.xyzq[j];
	const double2 lj = at.lj[j];
	const int2 mj = at.mf[j];
	const int gmol = mol[0].mf.x;
	double e_lj = 0, e_re = 0;
	int n_lj = 0, n_es = 0;
	double imm_j = 0.0;
	if (EXT && fp.fh_order) imm_j = at.inv_molmass[j];
	if (!(mj.y & AF_PAD) && mj.x != gmol) { // (a removed molecule's own atoms are not its partners: their pairs are the own block's)
		for (int k = 0; k < m; ++k) {
			const int2 mi = mol[k].mf;
			const PairFlags f = pair_flags(mi.x, mi.y, mj.x, mj.y);
			if (f.frozen) continue;
			const double2 li = mol[k].lj;
			double sig, eps;
			lj_mix(mi.y, mj.y, li.x, li.y, lj.x, lj.y, sig, eps);
			double imu = 0.0;
			if (EXT && fp.fh_order) imu = mol[k].inv_molmass + imm_j;
			pair_terms<ORTHO, EXT>(bx, fp, do_es, mol[k].xyzq, pj, sig, eps, f, imu, sg, e_lj, e_re, n_lj, n_es);
		}
	}
	e_lj = wave_sum(e_lj);
	e_re = wave_sum(e_re);
	n_lj = wave_sum_i(n_lj);
	n_es = wave_sum_i(n_es);
	if (threadIdx.x == 0) {
		block_part[2 * (size_t)tile] = e_lj;
		block_part[2 * (size_t)tile + 1] = e_re;
		block_cnt[2 * (size_t)tile] = n_lj;
		block_cnt[2 * (size_t)tile + 1] = n_es;
	}
}

// the molecule's own pairs, one block: whatever pair_flags admits among its atoms (partial `slot`), and with Ewald electrostatics the
// intramolecular charge-to-screen term of coulombic_real (:1503-1504; raw distance, as delta_intra_block) into out_intra
template <bool ORTHO, bool EXT>
__device__ __forceinline__ void exchange_own_block(const Box &bx, const FusedParams &fp, int do_es, int do_ewald, const XchAtom *__restrict__ mol, int m, double sg,
                                                   double *__restrict__ block_part, int *__restrict__ block_cnt, int slot, double *__restrict__ out_intra) {
	double e_lj = 0, e_re = 0, acc = 0;
	int n_lj = 0, n_es = 0;
	for (int k = threadIdx.x; k < m; k += kTile) {
		const XchAtom a = mol[k];
		for (int l = k + 1; l < m; ++l) {
			const XchAtom b = mol[l];
			const PairFlags f = pair_flags(a.mf.x, a.mf.y, b.mf.x, b.mf.y);
			if (f.frozen) continue;
			double sig, eps;
			lj_mix(a.mf.y, b.mf.y, a.lj.x, a.lj.y, b.lj.x, b.lj.y, sig, eps);
			double imu = 0.0;
			if (EXT && fp.fh_order) imu = a.inv_molmass + b.inv_molmass;
			pair_terms<ORTHO, EXT>(bx, fp, do_es, a.xyzq, b.xyzq, sig, eps, f, imu, sg, e_lj, e_re, n_lj, n_es);
			const double qq = a.xyzq.w * b.xyzq.w;
			if (!do_ewald || qq == 0.0) continue;
			const double dx = a.xyzq.x - b.xyzq.x, dy = a.xyzq.y - b.xyzq.y, dz = a.xyzq.z - b.xyzq.z;
			const double r2 = ((dx * dx) + dy * dy) + dz * dz;
			const double ir = fast_rsqrt(r2);
			double g;
			acc += sg * (qq * (1.0 - erfc_and_gauss(fp.ewald_alpha * (r2 * ir), g)) * ir);
		}
	}
	e_lj = wave_sum(e_lj);
	e_re = wave_sum(e_re);
	acc = wave_sum(acc);
	n_lj = wave_sum_i(n_lj);
	n_es = wave_sum_i(n_es);
	if (threadIdx.x == 0) {
		block_part[2 * (size_t)slot] = e_lj;
		block_part[2 * (size_t)slot + 1] = e_re;
		block_cnt[2 * (size_t)slot] = n_lj;
		block_cnt[2 * (size_t)slot + 1] = n_es;
		out_intra[0] = acc;
	}
}

// trial structure factors: sf_trial[k] = sf[k] + sg sum_molecule q e^{i k.r}; one wave per k-vector, the four components split as in
// k_recip_sf (energy: not frozen, q != 0; field: every atom)
__device__ __forceinline__ void exchange_recip_k(const RecipDev &rc, const XchAtom *__restrict__ mol, int m, double sg, double4 *__restrict__ sf_trial, int kidx) {
	const double4 kv = rc.kvec[kidx];
	double re = 0, im = 0, C = 0, S = 0;
	for (int k = threadIdx.x; k < m; k += kTile) {
		const double4 p = mol[k].xyzq;
		const int fl = mol[k].mf.y;
		double s, c;
		sincos(((kv.x * p.x) + kv.y * p.y) + kv.z * p.z, &s, &c);
		const double qc = p.w * c, qs = p.w * s;
		C += qc;
		S += qs;
		if (!(fl & (AF_FROZEN | AF_ZERO_Q))) {
			re += qc;
			im += qs;
		}
	}
	re = wave_sum(re);
	im = wave_sum(im);
	C = wave_sum(C);
	S = wave_sum(S);
	if (threadIdx.x == 0) {
		const double4 o = rc.sf[kidx];
		sf_trial[kidx] = make_double4(o.x + sg * re, o.y + sg * im, o.z + sg * C, o.w + sg * S);
	}
}

// ONE launch, block-uniform roles as in k_delta_all: blocks [0, nt) one tile each, block nt the molecule's own pairs, blocks
// (nt, nt + 1 + K) one k-vector each (Ewald electrostatics only: otherwise the grid ends at nt + 1)
template <bool ORTHO, bool EXT>
__global__ __launch_bounds__(64) void k_exchange_all(AtomsDev at, Box bx, RecipDev rc, FusedParams fp, int do_es, int do_ewald, const XchAtom *__restrict__ mol,
                                                     int m, double sg, double4 *__restrict__ sf_trial, double *__restrict__ block_part,
                                                     int *__restrict__ block_cnt, double *__restrict__ out_intra) {
	const int nt = at.n_pad / kTile;
	const int b = blockIdx.x;
	if (b < nt) exchange_pairs_tile<ORTHO, EXT>(at, bx, fp, do_es, mol, m, sg, block_part, block_cnt, b);
	else if (b == nt) exchange_own_block<ORTHO, EXT>(bx, fp, do_es, do_ewald, mol, m, sg, block_part, block_cnt, nt, out_intra);
	else if (b - nt - 1 < rc.K) exchange_recip_k(rc, mol, m, sg, sf_trial, b - nt - 1);
}

void launch_exchange(hipStream_t st, const AtomsDev &at, const Box &bx, const RecipDev &rc, const FusedParams &fp, int do_es, const XchAtom *mol, int m,
                     double sg, double4 *sf_trial, double *block_part, int *block_cnt, double *out4, long long *dcnt2, double *host_out, double seq) {
	const int nt = at.n_pad / kTile;
	const bool ext = (do_es && fp.wolf) || fp.fh_order;
	const int do_ewald = (do_es && !fp.wolf) ? 1 : 0; // intramolecular + reciprocal parts exist
	const int grid = nt + 1 + (do_ewald ? rc.K : 0);
	with_flags(bx.ortho != 0, ext, [&](auto O, auto E) {
		hipLaunchKernelGGL((k_exchange_all<O.value, E.value>), dim3(grid), dim3(kTile), 0, st, at, bx, rc, fp, do_es, do_ewald, mol, m, sg, sf_trial, block_part,
		                   block_cnt, out4 + D_ES_INTRA);
	});
	launch_delta_finish(st, block_part, block_cnt, nt + 1, rc, sf_trial, bx, do_ewald, out4, dcnt2, host_out, seq);
}

} // namespace mpmc
