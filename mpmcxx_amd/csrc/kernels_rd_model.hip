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
// The two walks are pair_term_walk.h's.  RdModelTerm states the payload (sp, sqrt(epsilon), epsilon, 1 / molecule mass), the admission
// (neither rd_excluded nor frozen) and the pair function, and sums three quantities (energy, kept terms, skipped tile pairs; counts as
// doubles: exact).  A tile pair whose class says CLS_BEYOND_CUTOFF is not walked.  The classes are this evaluation's (k_classify,
// kernels_sym.hip), and their margin is far wider than the 1e-12 A of the LJ test: the class is set for a lower bound of the distance of the
// bounding boxes, itself shortened by 1e-12 of the cell edge, above max(t_lj, t_es) (1 + 1e-9), i.e. about 5e-10 cutoff beyond both tests
// (launch_tile_classes).
//
// RdModelLrcTerm: the LJ form's pair correction with the mixed parameters over EVERY pair that is not frozen and has eps_ij != 0 and
// sigma_ij != 0 (lj_lrc_corr :1036-1069; intramolecular and excluded pairs count).  It does not factorise over the atoms, so it is a pair
// sum of its own, the same walk without positions; it depends on the parameters, the flags, the cutoff and the volume only, and the host
// caches it (context.cpp).
#include "pair_term_walk.h"

namespace mpmc {

static_assert(S_RDM_SKIPPED < S_COUNT, "the scalar block holds the rd-model slots");

struct ExpFast {
	__device__ __forceinline__ double operator()(double x) const { return exp_fast(x); }
};

// the first six doubles of both payloads: (sigma, sigma^2, sigma^3, sigma^6, sqrt(epsilon), epsilon)
__device__ __forceinline__ void rd_atom_load(const double4 *sp, const double2 *lj, const double *epsv, int slot, double *v) {
	const double4 s = sp[slot];
	v[0] = s.x, v[1] = s.y, v[2] = s.z, v[3] = s.w, v[4] = lj[slot].y, v[5] = epsv[slot];
}
__device__ __forceinline__ RdAtom rd_atom(const double *v) { return RdAtom{v[0], v[1], v[2], v[3], v[4], v[5]}; }

// one pair at the raw displacement d = pos_i - pos_j: its energy, 0 outside the form's distance test; cnt += 1 inside it
template <bool ORTHO, int FORM, int MIX>
__device__ __forceinline__ double rdm_pair(const Box &bx, const RdModelParams &rp, double dx, double dy, double dz, const RdAtom &a, const RdAtom &b, double imu,
                                           int &cnt) {
	double ox, oy, oz;
	const double ri2 = min_image_sq<ORTHO>(bx, dx, dy, dz, ox, oy, oz);
	if (!(ri2 <= rp.t_in)) return 0.0;
	cnt += 1;
	const RdMixed m = rd_mix<MIX, FORM>(a, b);
	return rd_pair_energy<FORM>(m, ri2, FORM == RD_FORM_LJ ? rp.fh_order : 0, rp.fh_c2, rp.fh_c4, imu, ExpFast{});
}

template <int FORM, int MIX>
struct RdModelTerm {
	static constexpr int kDoubles = 7, kSums = 3, kBlocks = kRdModelBlocks; // (RdAtom, 1 / molecule mass)
	static constexpr bool kGeometry = true, kJSplit = false, kClassSkip = true, kPins = true;
	const double4 *sp;
	const double2 *lj;
	const double *epsv, *inv_molmass;
	RdModelParams rp;
	__device__ __forceinline__ void prepare() {}
	__device__ __forceinline__ void load(int slot, double *v) const {
		rd_atom_load(sp, lj, epsv, slot, v);
		v[6] = ((FORM == RD_FORM_LJ) && rp.fh_order != 0) ? inv_molmass[slot] : 0.0;
	}
	__device__ __forceinline__ static bool admits(const PairFlags &f) { return !f.rd_excluded && !f.frozen; }
	template <bool ORTHO>
	__device__ __forceinline__ double pair(const Box &bx, double dx, double dy, double dz, const double *a, const double *b, int, int, const PairFlags &,
	                                       int &cnt) const {
		return rdm_pair<ORTHO, FORM, MIX>(bx, rp, dx, dy, dz, rd_atom(a), rd_atom(b), a[6] + b[6], cnt);
	}
};

// every pair once, whatever its distance: the LJ form's pair correction with the mixed parameters
template <int MIX>
struct RdModelLrcTerm {
	static constexpr int kDoubles = 6, kSums = 1, kBlocks = kRdModelBlocks;
	static constexpr bool kGeometry = false, kJSplit = false, kClassSkip = false, kPins = false;
	const double4 *sp;
	const double2 *lj;
	const double *epsv;
	double cutoff, volume;
	__device__ __forceinline__ void prepare() {}
	__device__ __forceinline__ void load(int slot, double *v) const { rd_atom_load(sp, lj, epsv, slot, v); }
	__device__ __forceinline__ static bool admits(const PairFlags &f) { return !f.frozen; }
	template <bool ORTHO>
	__device__ __forceinline__ double pair(const Box &, double, double, double, const double *a, const double *b, int, int, const PairFlags &, int &) const {
		const RdMixed m = rd_mix<MIX>(rd_atom(a), rd_atom(b));
		return (m.eps != 0.0 && m.sigma != 0.0) ? lrc_term(m.sigma, m.eps, cutoff, volume) : 0.0;
	}
};

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

void launch_rd_model(hipStream_t st, const AtomsDev &at, const double4 *sp, const int2 *tile_pairs, const int *cls, int n_tile_pairs, const Box &bx,
                     const RdModelParams &rp, double *part, double *out3) {
	with_rd_model(rp.form, rp.mix, [&](auto F, auto M) {
		launch_pair_term_sum(st, RdModelTerm<F.value, M.value>{sp, at.lj, at.eps, at.inv_molmass, rp}, at, tile_pairs, cls, n_tile_pairs, 1, bx, part, out3);
	});
}

void launch_rd_model_lrc(hipStream_t st, const AtomsDev &at, const double4 *sp, const int2 *tile_pairs, int n_tile_pairs, int mix, double cutoff,
                         double volume, double *part, double *out) {
	with_rd_model(RD_FORM_LJ, mix, [&](auto, auto M) {
		launch_pair_term_sum(st, RdModelLrcTerm<M.value>{sp, at.lj, at.eps, cutoff, volume}, at, tile_pairs, nullptr, n_tile_pairs, 1, Box{}, part, out); // (no cell: no geometry)
	});
}

void launch_rd_model_delta(hipStream_t st, const AtomsDev &at, const double4 *sp, const Box &bx, const RdModelParams &rp, const int *mv_slot,
                           const double4 *mv_new, int m, int *moved_idx, double *part, double *out2) {
	with_rd_model(rp.form, rp.mix, [&](auto F, auto M) {
		launch_pair_term_delta(st, RdModelTerm<F.value, M.value>{sp, at.lj, at.eps, at.inv_molmass, rp}, at, bx, mv_slot, mv_new, m, moved_idx, part, out2);
	});
}

} // namespace mpmc
