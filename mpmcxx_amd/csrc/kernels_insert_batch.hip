// kernels_insert_batch.hip -- batched insertion candidates: the exchange-move energy of MANY trial poses of one molecule against the same
// accepted configuration, in one launch chain (mpmc_insert_candidates, trial.cpp).
//
// Widom insertion, orientational-bias / multiple-try insertion and energy-biased site selection all ask "what is the energy with this
// molecule at this pose?" many times before anything is accepted.  One such question is k_exchange_all + k_delta_finish, a few
// microseconds of device work behind ~30 us of host launch-and-poll; a batch of them shares the launches and the wait.
//   k_insert_batch_all     grid (nt + 1 [+ K], candidate chunks): the block-uniform roles of k_exchange_all in x; a block takes
//                          kInsBatchBlockCands candidates in y and runs them ONE AFTER THE OTHER against the resident loads it made once
//                          (tile role).  Each candidate has its own accumulators, wave sums and partials: its summation order is that of
//                          the single trial whatever the chunk and wherever the candidate stands in the batch.
//   k_insert_batch_finish  one block per candidate: delta_finish_sums (trial_kernels.h), the reduction of k_delta_finish, into the
//                          candidate's record of the device result array.
// No atomics: a repeated call gives the same bits.  Nothing resident is written: the accepted structure factors are read, each candidate's
// trial structure factors go to scratch.
#include "kernels.h"
#include "device_math.h"
#include "trial_kernels.h"
#include "exchange_kernels.h"

namespace mpmc {

// mol: [nc][m] staged records; block_part / block_cnt: [nc][nt + 1][2]; sf_trial: [nc][K]; out: [nc]
template <bool ORTHO, bool EXT>
__global__ __launch_bounds__(64) void k_insert_batch_all(AtomsDev at, Box bx, RecipDev rc, FusedParams fp, int do_es, int do_ewald, const XchAtom *__restrict__ mol,
                                                         int m, int nc, double4 *__restrict__ sf_trial, double *__restrict__ block_part,
                                                         int *__restrict__ block_cnt, InsCandOut *__restrict__ out) {
	const int nt = at.n_pad / kTile;
	const int b = blockIdx.x;
	const int c0 = blockIdx.y * kInsBatchBlockCands;
	const int c1 = min(c0 + kInsBatchBlockCands, nc);
	const size_t nb = (size_t)nt + 1;
	if (b < nt) {
		const XchResident rs = exchange_load_resident<EXT>(at, fp, b * kTile + threadIdx.x);
		for (int c = c0; c < c1; ++c)
			exchange_pairs_resident<ORTHO, EXT>(rs, bx, fp, do_es, mol + (size_t)c * m, m, 1.0, block_part + 2 * nb * c, block_cnt + 2 * nb * c, b);
	} else if (b == nt) {
		for (int c = c0; c < c1; ++c)
			exchange_own_block<ORTHO, EXT>(bx, fp, do_es, do_ewald, mol + (size_t)c * m, m, 1.0, block_part + 2 * nb * c, block_cnt + 2 * nb * c, nt, &out[c].es_intra);
	} else if (b - nt - 1 < rc.K) {
		for (int c = c0; c < c1; ++c) exchange_recip_k(rc, mol + (size_t)c * m, m, 1.0, sf_trial + (size_t)c * rc.K, b - nt - 1);
	}
}

__global__ __launch_bounds__(256) void k_insert_batch_finish(const double *__restrict__ block_part, const int *__restrict__ block_cnt, int nb, RecipDev rc,
                                                             const double4 *__restrict__ sf_trial, Box bx, int do_es, InsCandOut *__restrict__ out) {
	__shared__ double sh[4];
	__shared__ long long shc[256];
	const size_t c = blockIdx.x;
	double s0, s1, e;
	long long c0, c1;
	delta_finish_sums(block_part + 2 * (size_t)nb * c, block_cnt + 2 * (size_t)nb * c, nb, rc, sf_trial + c * (size_t)rc.K, do_es, sh, shc, s0, s1, e, c0, c1);
	if (threadIdx.x == 0) {
		InsCandOut &o = out[c];
		o.lj = s0;
		o.es_real = s1;
		if (!do_es) o.es_intra = 0.0; // (the own block wrote it otherwise)
		o.es_recip = e * (4.0 * kPi / bx.volume);
		o.n_lj = c0;
		o.n_es = c1;
	}
}

void launch_insert_batch(hipStream_t st, const AtomsDev &at, const Box &bx, const RecipDev &rc, const FusedParams &fp, int do_es, const XchAtom *mol, int m, int nc,
                         double4 *sf_trial, double *block_part, int *block_cnt, InsCandOut *out) {
	const int nt = at.n_pad / kTile;
	const bool ext = (do_es && fp.wolf) || fp.fh_order;
	const int do_ewald = (do_es && !fp.wolf) ? 1 : 0; // intramolecular + reciprocal parts exist
	const dim3 grid(nt + 1 + (do_ewald ? rc.K : 0), (nc + kInsBatchBlockCands - 1) / kInsBatchBlockCands);
	with_flags(bx.ortho != 0, ext, [&](auto O, auto E) {
		hipLaunchKernelGGL((k_insert_batch_all<O.value, E.value>), grid, dim3(kTile), 0, st, at, bx, rc, fp, do_es, do_ewald, mol, m, nc, sf_trial, block_part, block_cnt,
		                   out);
	});
	hipLaunchKernelGGL(k_insert_batch_finish, dim3(nc), dim3(256), 0, st, block_part, block_cnt, nt + 1, rc, sf_trial, bx, do_ewald, out);
}

} // namespace mpmc
