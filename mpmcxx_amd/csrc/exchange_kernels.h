// exchange_kernels.h -- the three block roles of an exchange move as device functions: the molecule against one resident tile, the
// molecule's own block, one k-vector of the trial structure factors.  kernels_exchange.hip runs them for ONE molecule (k_exchange_all),
// kernels_insert_batch.hip for a chunk of insertion candidates against the same resident loads (k_insert_batch_all): the arithmetic of a
// candidate and its order are these functions', so a batched candidate comes out with the bits of the single trial.  Included after
// kernels.h; pair_terms is trial_kernels.h's.
#pragma once

#include "kernels.h"
#include "device_math.h"
#include "trial_kernels.h"

namespace mpmc {

// what a thread of a tile role holds of its resident slot
struct XchResident {
	double4 pj;
	double2 lj;
	int2 mj;
	double imm_j;
};
template <bool EXT>
__device__ __forceinline__ XchResident exchange_load_resident(const AtomsDev &at, const FusedParams &fp, int j) {
	XchResident r;
	r.pj = at.xyzq[j];
	r.lj = at.lj[j];
	r.mj = at.mf[j];
	r.imm_j = 0.0;
	if (EXT && fp.fh_order) r.imm_j = at.inv_molmass[j];
	return r;
}

// the resident slot against the molecule's atoms k = 0 .. m-1 in order, wave sums, lane 0 writes partial `tile`
template <bool ORTHO, bool EXT>
__device__ __forceinline__ void exchange_pairs_resident(const XchResident &rs, const Box &bx, const FusedParams &fp, int do_es, const XchAtom *__restrict__ mol, int m,
                                                        double sg, double *__restrict__ block_part, int *__restrict__ block_cnt, int tile) {
	const double4 pj = rs.pj;
	const double2 lj = rs.lj;
	const int2 mj = rs.mj;
	const int gmol = mol[0].mf.x;
	double e_lj = 0, e_re = 0;
	int n_lj = 0, n_es = 0;
	const double imm_j = rs.imm_j;
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

// thread = resident slot j of tile `tile`; loops over the molecule's atoms
template <bool ORTHO, bool EXT>
__device__ __forceinline__ void exchange_pairs_tile(const AtomsDev &at, const Box &bx, const FusedParams &fp, int do_es, const XchAtom *__restrict__ mol, int m,
                                                    double sg, double *__restrict__ block_part, int *__restrict__ block_cnt, int tile) {
	const XchResident rs = exchange_load_resident<EXT>(at, fp, tile * kTile + threadIdx.x);
	exchange_pairs_resident<ORTHO, EXT>(rs, bx, fp, do_es, mol, m, sg, block_part, block_cnt, tile);
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

} // namespace mpmc
