// kernels_contact.hip -- cavity_autoreject (mpmc_set_cavity_autoreject): how many pairs are "in contact".  Two integer pair sums, no energy:
//
//   sigma rule     (System::lj src/System.Energy.cpp:1001-1004, lj_buffered_14_7 :1237-1239, dreiding :2182-2185): a pair the rd function admits
//                  -- neither rd_excluded nor frozen, inside the form's distance test -- with rimg < scale * sigma_ij has its rd_energy replaced
//                  by MAXVALUE.  sigma_ij is the mixed sigma of the context's rd model (rd_mix, pair_math.h; >= 0 there, so the LJ form's fabs
//                  changes nothing), or lj_mix's |sigma_ij| for the plain term.  Under the disp-expansion term: ContactDispTerm below.
//   absolute rule  (System::cavity_absolute_check src/System.Cavity.cpp:211-228): every measured pair of different molecules with
//                  rimg < scale, whatever its exclusions and whatever the cutoff.  System::pairs measures a pair `if (!frozen || polarization)`
//                  (src/System.cpp:985): without polarization a pair of two frozen atoms is not measured and does not count here (the host
//                  counts those pairs from the atom list: they keep rimg = 0 and always trip the test).
//
// rimg is the correctly rounded square root of min_image_sq (pair_math.h: the reference's bits in any cell), the products scale * sigma_ij
// are not fused: both tests are the reference's comparisons of the reference's doubles.
//
// The two walks are pair_term_walk.h's.  ContactTerm sums three quantities: the pairs the sigma rule replaces (in the walk's energy slot: a
// sum of 1.0s, exact), the absolute contacts (the walk's kept terms) and the tile pairs that were not walked.  Both rules share one walk.
// A contact needs rimg < dmax = scale * max(sigma_ij), respectively scale: k_contact_classes marks the tile pairs whose bounding boxes
// (k_tile_bounds of this evaluation, kernels_sym.hip) lie further apart than that, with the bound and the margins of k_classify, and the walk
// skips them (orthorhombic cells).
#include "pair_term_walk.h"

#include <cmath>

namespace mpmc {

static_assert(S_CA_SKIPPED == S_CA_REPLACED + 2 && S_CA_SKIPPED < S_COUNT, "the scalar block holds the three contact slots side by side");
static_assert(D_CA_ABSOLUTE == D_CA_REPLACED + 1, "the delta launcher writes { replaced, absolute } side by side");

// MODEL: sigma_ij by the rd model's rule MIX from sp = (sigma, sigma^2, sigma^3, sigma^6); otherwise by lj_mix from |sigma| and the flag words
template <int RULES, bool MODEL, int MIX>
struct ContactTerm {
	static constexpr bool kSigma = (RULES & CA_RULE_SIGMA) != 0, kAbsolute = (RULES & CA_RULE_ABSOLUTE) != 0;
	static constexpr int kDoubles = (kSigma && MODEL) ? 4 : 1, kSums = 3, kBlocks = kContactBlocks;
	static constexpr bool kGeometry = true, kJSplit = false, kClassSkip = true, kPins = true;
	const double4 *sp;
	const double2 *lj;
	ContactParams cp;
	__device__ __forceinline__ void prepare() {}
	__device__ __forceinline__ void load(int slot, double *v) const {
		if (kSigma && MODEL) {
			const double4 s = sp[slot];
			v[0] = s.x, v[1] = s.y, v[2] = s.z, v[3] = s.w;
		} else v[0] = kSigma ? lj[slot].x : 0.0;
	}
	// (the absolute rule looks at excluded pairs too: the pair function applies each rule's own admission)
	__device__ __forceinline__ static bool admits(const PairFlags &f) { return kAbsolute ? !f.intra : (!f.rd_excluded && !f.frozen); }
	template <bool ORTHO>
	__device__ __forceinline__ double pair(const Box &bx, double dx, double dy, double dz, const double *a, const double *b, int fla, int flb, const PairFlags &f,
	                                       int &cnt) const {
		double ox, oy, oz;
		const double ri2 = min_image_sq<ORTHO>(bx, dx, dy, dz, ox, oy, oz);
		const double rimg = sqrt(ri2);
		double replaced = 0.0;
		if (kSigma && !f.rd_excluded && !f.frozen && ri2 <= cp.t_in) {
			double sigma, eps;
			if (MODEL) sigma = rd_mix<MIX>(RdAtom{a[0], a[1], a[2], a[3], 0.0, 0.0}, RdAtom{b[0], b[1], b[2], b[3], 0.0, 0.0}).sigma;
			else lj_mix(fla, flb, a[0], 0.0, b[0], 0.0, sigma, eps);
			if (rimg < cp.scale * sigma) replaced = 1.0;
		}
		if (kAbsolute && !f.intra && (cp.measure_frozen || !f.frozen) && rimg < cp.scale) cnt += 1;
		return replaced;
	}
};

// The sigma rule under the disp-expansion term (System::disp_expansion :1958, 1983-1989): every pair that is neither rd_excluded nor frozen,
// with no cutoff; sigma_ij = r0_ij = (r0_i + r0_j) / 2 as mixed; and, when cavity_autoreject_repulsion != 0, a second test on the pair's
// repulsion 315.775 exp(-alpha_ij (r - r0_ij)) (0 when alpha_ij or r0_ij is 0, as in disp_expansion_pair) -- a pair that fails either test is
// replaced once.  Payload: (alpha, r0) of DispTerm's table.
template <int RULES>
struct ContactDispTerm {
	static constexpr bool kSigma = (RULES & CA_RULE_SIGMA) != 0, kAbsolute = (RULES & CA_RULE_ABSOLUTE) != 0;
	static constexpr int kDoubles = 2, kSums = 3, kBlocks = kContactBlocks;
	static constexpr bool kGeometry = true, kJSplit = false, kClassSkip = true, kPins = true;
	const double4 *co;
	ContactParams cp;
	__device__ __forceinline__ void prepare() {}
	__device__ __forceinline__ void load(int slot, double *v) const {
		const double4 c = co[slot];
		v[0] = c.x, v[1] = c.y;
	}
	__device__ __forceinline__ static bool admits(const PairFlags &f) { return kAbsolute ? !f.intra : (!f.rd_excluded && !f.frozen); }
	template <bool ORTHO>
	__device__ __forceinline__ double pair(const Box &bx, double dx, double dy, double dz, const double *a, const double *b, int, int, const PairFlags &f,
	                                       int &cnt) const {
		double ox, oy, oz;
		const double rimg = sqrt(min_image_sq<ORTHO>(bx, dx, dy, dz, ox, oy, oz));
		double replaced = 0.0;
		if (kSigma && !f.rd_excluded && !f.frozen) {
			const double r0_ij = 0.5 * (a[1] + b[1]);
			bool hit = rimg < cp.scale * r0_ij;
			if (cp.repulsion != 0.0) {
				const double a_ij = disp_mix_alpha(a[0], b[0], cp.schmidt != 0);
				const double rep = (a_ij != 0.0 && r0_ij != 0.0) ? kDispRepulsion * exp(-a_ij * (rimg - r0_ij)) : 0.0;
				hit = hit || rep > cp.repulsion;
			}
			replaced = hit ? 1.0 : 0.0;
		}
		if (kAbsolute && !f.intra && (cp.measure_frozen || !f.frozen) && rimg < cp.scale) cnt += 1;
		return replaced;
	}
};

// run-time (rules, model, rule of mixing) -> template arguments
template <class F>
static inline void with_contact(const ContactParams &cp, F &&f) {
	auto by_mix = [&](auto R) {
		if (!(cp.rules & CA_RULE_SIGMA) || !cp.model || cp.disp) return f(R, std::false_type{}, std::integral_constant<int, RD_MIX_LB>{});
		switch (cp.mix) {
		case RD_MIX_WALDMAN_HAGLER: return f(R, std::true_type{}, std::integral_constant<int, RD_MIX_WALDMAN_HAGLER>{});
		case RD_MIX_HALGREN: return f(R, std::true_type{}, std::integral_constant<int, RD_MIX_HALGREN>{});
		case RD_MIX_C6: return f(R, std::true_type{}, std::integral_constant<int, RD_MIX_C6>{});
		default: return f(R, std::true_type{}, std::integral_constant<int, RD_MIX_LB>{});
		}
	};
	switch (cp.rules & (CA_RULE_SIGMA | CA_RULE_ABSOLUTE)) {
	case CA_RULE_SIGMA: by_mix(std::integral_constant<int, CA_RULE_SIGMA>{}); break;
	case CA_RULE_ABSOLUTE: by_mix(std::integral_constant<int, CA_RULE_ABSOLUTE>{}); break;
	default: by_mix(std::integral_constant<int, CA_RULE_SIGMA | CA_RULE_ABSOLUTE>{}); break;
	}
}

// cls[t] = CLS_BEYOND_CUTOFF when no pair of tile pair t can be closer than sqrt(thr2): the lower bound of k_classify for orthorhombic
// cells (gaps of the wrapped fractional bounding boxes on the unit circle, each shortened by 1e-12), 0 otherwise and for I == J
__global__ __launch_bounds__(256) void k_contact_classes(const double *__restrict__ tb, const int2 *__restrict__ tile_pairs, int ntp, Box bx, double thr2,
                                                         int *__restrict__ cls) {
	const int t = blockIdx.x * 256 + threadIdx.x;
	if (t >= ntp) return;
	const int2 IJ = tile_pairs[t];
	int c = 0;
	if (IJ.x != IJ.y) {
		double d2 = 0;
		for (int d = 0; d < 3; ++d) {
			const double a0 = tb[12 * (size_t)IJ.x + d], a1 = tb[12 * (size_t)IJ.x + 3 + d];
			const double b0 = tb[12 * (size_t)IJ.y + d], b1 = tb[12 * (size_t)IJ.y + 3 + d];
			double gap = 0.0;
			if (a1 < b0) gap = fmin(b0 - a1, a0 + 1.0 - b1);
			else if (b1 < a0) gap = fmin(a0 - b1, b0 + 1.0 - a1);
			gap = fmax(0.0, gap - 1e-12);
			const double L = fabs(bx.b[4 * d]);
			d2 += (L * gap) * (L * gap);
		}
		if (d2 > thr2) c = CLS_BEYOND_CUTOFF;
	}
	cls[t] = c;
}

void launch_contact(hipStream_t st, const AtomsDev &at, const double4 *sp, const int2 *tile_pairs, int n_tile_pairs, const Box &bx, const ContactParams &cp,
                    const double *tile_bounds, int *cls, double *part, double *out3) {
	const bool skip = tile_bounds && cls && bx.ortho && std::isfinite(cp.dmax);
	if (skip) {
		const double thr2 = (cp.dmax * cp.dmax) * (1.0 + 1e-9);
		hipLaunchKernelGGL(k_contact_classes, dim3((n_tile_pairs + 255) / 256), dim3(256), 0, st, tile_bounds, tile_pairs, n_tile_pairs, bx, thr2, cls);
	}
	with_contact(cp, [&](auto R, auto M, auto X) {
		if constexpr ((decltype(R)::value & CA_RULE_SIGMA) != 0) {
			if (cp.disp) return launch_pair_term_sum(st, ContactDispTerm<R.value>{sp, cp}, at, tile_pairs, skip ? cls : nullptr, n_tile_pairs, 1, bx, part, out3);
		}
		launch_pair_term_sum(st, ContactTerm<R.value, M.value, X.value>{sp, at.lj, cp}, at, tile_pairs, skip ? cls : nullptr, n_tile_pairs, 1, bx, part, out3);
	});
}

// ---- exchange moves (kernels_exchange.hip, kernels_insert_batch.hip): the molecule against one resident tile, per candidate.  A sibling of
// k_exchange_all / k_insert_batch_all in the same launch chain, in front of the finish kernel that posts: thread = resident slot, the
// molecule's atoms in order, candidates of a block one after the other against the resident load it made once.  The molecule's own pairs
// are intramolecular and count under neither rule.  Counts are integers: any order of summation gives the same value.
template <bool ORTHO>
__global__ __launch_bounds__(64) void k_exchange_contact(AtomsDev at, Box bx, ContactParams cp, const XchAtom *__restrict__ mol, int m, int nc, int *__restrict__ part) {
	const int nt = at.n_pad / kTile;
	const int b = blockIdx.x, j = b * kTile + threadIdx.x; // (< n_pad)
	const int c0 = blockIdx.y * kInsBatchBlockCands, c1 = min(c0 + kInsBatchBlockCands, nc);
	const double4 pj = at.xyzq[j];
	const double sj = at.lj[j].x;
	const int2 mj = at.mf[j];
	const bool sigma_rule = (cp.rules & CA_RULE_SIGMA) != 0, absolute_rule = (cp.rules & CA_RULE_ABSOLUTE) != 0;
	for (int c = c0; c < c1; ++c) {
		const XchAtom *__restrict__ g = mol + (size_t)c * m;
		int n_rep = 0, n_abs = 0;
		if (!(mj.y & AF_PAD) && mj.x != g[0].mf.x) { // (a removed molecule's own atoms are not its partners)
			for (int k = 0; k < m; ++k) {
				const int2 mi = g[k].mf;
				const PairFlags f = pair_flags(mi.x, mi.y, mj.x, mj.y);
				const double4 pi = g[k].xyzq;
				double ox, oy, oz;
				const double ri2 = min_image_sq<ORTHO>(bx, pi.x - pj.x, pi.y - pj.y, pi.z - pj.z, ox, oy, oz);
				const double rimg = sqrt(ri2);
				if (sigma_rule && !f.rd_excluded && !f.frozen && ri2 <= cp.t_in) {
					double sigma, eps;
					lj_mix(mi.y, mj.y, g[k].lj.x, 0.0, sj, 0.0, sigma, eps);
					if (rimg < cp.scale * sigma) n_rep += 1;
				}
				if (absolute_rule && !f.intra && (cp.measure_frozen || !f.frozen) && rimg < cp.scale) n_abs += 1;
			}
		}
		n_rep = wave_sum_i(n_rep);
		n_abs = wave_sum_i(n_abs);
		if (threadIdx.x == 0) {
			part[2 * ((size_t)c * nt + b)] = n_rep;
			part[2 * ((size_t)c * nt + b) + 1] = n_abs;
		}
	}
}
// one wave per candidate: its tiles' counts summed
__global__ __launch_bounds__(64) void k_exchange_contact_finish(const int *__restrict__ part, int nt, double sg, double *__restrict__ out2, long long *__restrict__ out_ll) {
	const size_t c = blockIdx.x;
	long long r = 0, a = 0;
	for (int b = threadIdx.x; b < nt; b += 64) {
		r += part[2 * (c * nt + b)];
		a += part[2 * (c * nt + b) + 1];
	}
	for (int off = 32; off > 0; off >>= 1) {
		r += __shfl_down(r, off, 64);
		a += __shfl_down(a, off, 64);
	}
	if (threadIdx.x == 0) {
		if (out2 && c == 0) out2[0] = sg * (double)r, out2[1] = sg * (double)a;
		if (out_ll) out_ll[2 * c] = r, out_ll[2 * c + 1] = a;
	}
}

void launch_exchange_contact(hipStream_t st, const AtomsDev &at, const Box &bx, const ContactParams &cp, const XchAtom *mol, int m, int nc, double sg, int *part,
                             double *out2, long long *out_ll) {
	const int nt = at.n_pad / kTile;
	const dim3 grid(nt, (nc + kInsBatchBlockCands - 1) / kInsBatchBlockCands);
	with_flag(bx.ortho != 0, [&](auto O) { hipLaunchKernelGGL((k_exchange_contact<O.value>), grid, dim3(kTile), 0, st, at, bx, cp, mol, m, nc, part); });
	hipLaunchKernelGGL(k_exchange_contact_finish, dim3(nc), dim3(64), 0, st, part, nt, sg, out2, out_ll);
}

void launch_contact_delta(hipStream_t st, const AtomsDev &at, const double4 *sp, const Box &bx, const ContactParams &cp, const int *mv_slot,
                          const double4 *mv_new, int m, int *moved_idx, double *part, double *out2) {
	with_contact(cp, [&](auto R, auto M, auto X) {
		if constexpr ((decltype(R)::value & CA_RULE_SIGMA) != 0) {
			if (cp.disp) return launch_pair_term_delta(st, ContactDispTerm<R.value>{sp, cp}, at, bx, mv_slot, mv_new, m, moved_idx, part, out2);
		}
		launch_pair_term_delta(st, ContactTerm<R.value, M.value, X.value>{sp, at.lj, cp}, at, bx, mv_slot, mv_new, m, moved_idx, part, out2);
	});
}

} // namespace mpmc
