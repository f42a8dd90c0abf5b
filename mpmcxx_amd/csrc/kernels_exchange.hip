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
#include "exchange_kernels.h" // the three block roles (shared with kernels_insert_batch.hip)

namespace mpmc {

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
