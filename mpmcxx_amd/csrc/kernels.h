// kernels.h -- launch wrappers of the gfx950 kernels (implemented in the kernels*.hip files named section by section), the slots of the
// result blocks, and the constants the host shares with them; used by context.cpp, evaluate.cpp and trial.cpp.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "pair_math.h"
#include "polar_relax.h"

namespace mpmc {

// run-time flags -> template arguments: f receives std::true_type / std::false_type per flag, e.g.
//   with_flags(bx.ortho, damped, [&](auto O, auto D) { hipLaunchKernelGGL((k<O.value, D.value>), ...); });
template <class F>
inline void with_flag(bool a, F &&f) {
	if (a) f(std::true_type{});
	else f(std::false_type{});
}
template <class F>
inline void with_flags(bool a, bool b, F &&f) {
	with_flag(a, [&](auto A) { with_flag(b, [&](auto B) { f(A, B); }); });
}

constexpr int kTile = 64; // one wavefront owns 64 i-atoms; j-atoms are staged in LDS 64 at a time
constexpr int kKSplit = 8; // k-vector range split of the reciprocal field kernel: at least this many slices, ...
constexpr int kKSplitMax = 64, kKSplitWaves = 1024;
// ... and more when there are few tiles: one wave walks its slice of the k-vectors serially (26 us for the whole range over 8 slices,
// whatever the number of atoms), so a small system cuts the range until about kKSplitWaves waves share it.  A function of n_pad alone:
// the launcher of the field kernel and the kernel that adds the slices up both call it.
inline int recip_ksplit(int n_pad) {
	const int nt = n_pad / kTile;
	int ks = kKSplit;
	while (ks < kKSplitMax && nt * ks < kKSplitWaves) ks *= 2;
	return ks;
}
// doubles in the slice buffer [recip_ksplit(n_pad)][n_pad][3] for any n_pad <= max_pad
inline size_t recip_slices_capacity(size_t max_pad) { return std::max((size_t)kKSplit * 3 * max_pad, (size_t)2 * kKSplitWaves * kTile * 3); }

// device view of one System's atoms (struct-of-arrays, padded to a multiple of kTile)
struct AtomsDev {
	const double4 *xyzq; // x, y, z, charge
	const double2 *lj;   // |sigma|, sqrt(epsilon)
	const int2 *mf;      // molecule id, AF_* flags
	const double *alpha; // polarizability
	const double *eps;   // epsilon (atom self-LRC term)
	const double *inv_molmass; // 1 / (mass of the owning molecule, amu): Feynman-Hibbs reduced masses (may be null)
	int n, n_pad;
};

// slots of the scalar result vector on the device
enum : int {
	S_LJ = 0, S_LRC_PAIR, S_ES_REAL, S_ES_INTRA, // pair kernel
	S_ES_RECIP, S_ES_SELF, S_LRC_SELF,           // recip / atom kernel
	S_POLAR, S_RRMS,                             // polarization
	S_THREE_BODY,                                // Axilrod-Teller (kernels_three_body.hip)
	S_DISP, S_DISP_LRC_PAIR, S_DISP_LRC_SELF,    // disp-expansion pair sum and its two long-range corrections (kernels_disp.hip)
	S_PALMO,                                     // Palmo-Krimm correction, already part of S_POLAR (kernels_wolf_field.hip)
	S_CRYSTAL, S_CRYSTAL_TERMS,                  // rd_crystal pair sum and its image-term count (a double: exact) (kernels_crystal.hip)
	S_RDM, S_RDM_TERMS, S_RDM_SKIPPED,           // rd-model pair sum, its kept terms and the tile pairs it skipped (doubles: exact) (kernels_rd_model.hip)
	S_CA_REPLACED, S_CA_ABSOLUTE, S_CA_SKIPPED,  // cavity_autoreject: pairs replaced by MAXVALUE, absolute contacts, tile pairs not walked (doubles: exact) (kernels_contact.hip)
	S_SG, S_SG_TERMS,                            // Silvera-Goldman pair sum and its kept terms (a double: exact) (kernels_sg.hip)
	S_COUNT = 24
};
enum : int { C_LJ_IN = 0, C_ES_IN, C_INTRA, C_RDX, C_ESX, C_FROZEN, C_COUNT = 8 };
// slots of a trial move's result block on the device (d_delta_out): what launch_delta leaves, then one change per further term
enum : int {
	D_LJ = 0, D_ES_REAL, D_ES_INTRA, D_ES_RECIP, D_SPARE, // the five pair values (kernels_delta.hip; the spare one is written 0)
	D_CNT_LJ, D_CNT_ES,                                   // the two int64 counts
	D_THREE_BODY,                                         // Axilrod-Teller (kernels_three_body.hip)
	D_DISP,                                               // disp-expansion (kernels_disp.hip)
	D_RD, D_RD_TERMS,                                     // rd_crystal's lattice sum and image terms, OR the rd model's OR Silvera-Goldman's sum and kept terms
	D_CA_REPLACED, D_CA_ABSOLUTE,                         // cavity_autoreject: change of the replaced pairs and of the absolute contacts (kernels_contact.hip)
	D_COUNT
};
// rd_crystal and the rd model share D_RD and D_RD_TERMS.  They never meet: a context with a model is not `rd_crystal on` (crystal_on is false
// for it, context.h) and rd_model_ready refuses the combination, so at most one of launch_crystal_delta and launch_rd_model_delta runs
// per move; each writes both slots.  The Silvera-Goldman term shares them too: it is refused together with a model and ignores rd_crystal.
static_assert(D_RD_TERMS == D_RD + 1, "the delta launchers of the rd terms write { sum, terms } side by side");
// the pinned host mirror (h_delta_out) holds the same slots with the launch number of k_delta_finish, which the host polls, in between:
// that slot stays where it was before the later terms came
constexpr int kDeltaHostSeq = D_THREE_BODY + 1;
constexpr int kDeltaHostCount = D_COUNT + 1;
constexpr int delta_host_index(int d) { return d < kDeltaHostSeq ? d : d + 1; }
// tile-pair classes written by k_classify (any cell: DESIGN section 3 has the bound used for skewed cells): lower bound of the
// minimum-image distance between the two tiles' bounding boxes
enum : int {
	CLS_BEYOND_CUTOFF = 1, // > cutoff: no pair of the tile pair passes any cutoff predicate
	CLS_THOLE_FAR = 2,     // lambda*r > kTholeFarX for every pair: T is the bare dipole tensor (see below for what that drops)
	CLS_UNIFORM_X = 4,     // per dimension (x, y, z = 4, 8, 16): one periodic image index serves all 4096 pairs of the tile pair in
	CLS_UNIFORM_Y = 8,     // that dimension (wrapped coordinates); tp_shift holds the lattice vector component B img
	CLS_UNIFORM_Z = 16
};
// Beyond lambda r = kTholeFarX a tile pair's tensors are the bare dipole tensors (nothing stored, recomputed from the positions).  The
// Thole factors differ from 1 by exp(-x)(x^3/6 + x^2/2 + x + 1) = 4.7e-10 at x = 30 -- a RELATIVE error of tensors that are themselves
// < 1/(14 A)^3 = 3.6e-4 of the self term 1/alpha, and only for the few pairs that sit right at the boundary (the class is decided by the
// tiles' bounding boxes, so almost every pair of a far tile pair is much further out).  Measured on the 10 000-atom box: the polarization
// energy moves by 6e-15 relative between x = 40 and x = 30 (1.4e-12 at x = 26), dipoles by < 1e-13 of the largest one.  The store shrinks from 5299 to
// 2576 of 12 403 tile pairs (347 -> 169 MB read per Jacobi iteration), which is worth 6-8 % of the whole-job rate: with 32 beads in
// flight the aggregate HBM traffic (3.7 TB/s at x = 40) is a co-bottleneck.  A compile-time constant: it is the knob of an approximation
// (rounds 1-2 read it from the environment).
constexpr double kTholeFarX = 30.0;

// reciprocal space: structure factors for every k, then energy + O(N) atom terms
struct RecipDev {
	const double4 *kvec; // kx, ky, kz, k^2            [K]
	const double *w_en;  // exp(-k^2/4a^2)/k^2         [K]
	const double4 *kw;   // k_p/k^2 exp(-k^2/4ap^2), _ [K]
	const int4 *lvec;    // integer l of k = 2 pi R l       [K] (null: one sincos per (k, atom))
	double4 *sf;         // SF_re, SF_im (energy: non-frozen, q != 0), C_k, S_k (field: all atoms)  [K]
	int K;
};
constexpr int kRecipTabMaxK = 15; // phase tables of 3 x 64 x (kmax+1) complex numbers must fit 64 KiB of LDS
// sf_part: [n_tiles][K] scratch of the factorised form (may be null: direct sincos form)
void launch_recip_sf(hipStream_t st, const AtomsDev &at, const Box &bx, const RecipDev &rc, int kmax, double4 *sf_part);
// reciprocal energy + O(N) atom terms: coulombic_self, lj_lrc_self, and the PAIR long-range correction summed in O(N)
// through moments of (sqrt(eps), |sigma|) (Lorentz-Berthelot makes the pair term a polynomial in sigma_i + sigma_j)
// position-independent terms (pair LRC, self LRC, Ewald self) into their three slots of the scalar block; part_scratch: kAtomTermScratch doubles
constexpr size_t kAtomTermScratch = 64 * 34;
void launch_atom_terms(hipStream_t st, const AtomsDev &at, const Box &bx, double ewald_alpha, int rd_lrc, int do_es, double *part_scratch,
                       double *scal);

// static field
void launch_field_recip(hipStream_t st, const AtomsDev &at, const Box &bx, const RecipDev &rc, int kmax, double *e_recip /*[recip_ksplit(n_pad)][n_pad][3]*/);
// E0 = recip*(8 pi/V) + sum_s part ; mu0 = gamma * alpha * E0
void launch_field_finalize(hipStream_t st, const AtomsDev &at, const Box &bx, int polar_ewald, const double *e_recip,
                           const double *part, int n_split, double gamma, double *e_static, double *mu,
                           double *e_real_out = nullptr /*the real-space part alone (sum of the slots): what a trial move updates incrementally*/,
                           double *mu_copy = nullptr /*a second copy of mu0: slot 0 of the ring of dipole differences*/);

// new_mu = alpha (E0 + F) ; optionally rrms per atom.  Precision-terminated solves pass ctl = { broke, converged-at, ticket } (device
// ints, zeroed at the start of the solve) and the iteration number: are_we_done_yet runs on the device, the kernels of iterations
// enqueued after convergence return at once (see iteration_verdict in kernels.hip)
void launch_dipole_update(hipStream_t st, const AtomsDev &at, const double *e_static, const double *part, int n_split,
                          const double *mu_old, double *mu_new, double *e_induced, int want_rrms, double *rrms_atom,
                          double allowed_sqerr, int *ctl, int *host_flag /*pinned {closed iteration, converged-at}, may be null*/, int it,
                          double *dk = nullptr /*new_mu - mu_old per component: this iteration's slot of the ring of dipole differences*/,
                          const RelaxWeights *relax = nullptr /*`polar_sor` / `polar_esor`: the relaxed instantiation stores w_new new_mu + w_old mu_old*/);
// iterator failure: mu = alpha * E0
void launch_dipole_reset(hipStream_t st, const AtomsDev &at, const double *e_static, double *mu);
// end of an evaluation: the scalar block [S_COUNT doubles][C_COUNT int64] goes to pinned host memory, the launch number behind it (a host
// that polls that slot finds the results complete), and the device block is left zeroed for the next evaluation
void launch_post_results(hipStream_t st, double *scal, double *out_host, double seq);
void launch_polar_energy(hipStream_t st, const AtomsDev &at, const double *mu, const double *e_static, const double *rrms_atom,
                         double *scal);
// The same energy of a Jacobi solve of n iterations from mu_0 = alpha E0, without mu_n: -1/2 sum_{k=0..n} m_k with
// m_2a = <d_a, d_a>_{1/alpha} and m_2a+1 = <d_a, d_a+1>_{1/alpha} over the ring dk[ceil(n/2) + 1][3 n_pad] (d_0 = mu_0, d_k = mu_k -
// mu_k-1); for a = 0, d_0 / alpha is E0 itself.  One block, fixed order; S_RRMS = 0 (such a solve reports none).
constexpr int kMomentsMaxIter = 64;                         // longer fixed-count solves keep -1/2 E0 . mu_n (the ring would outgrow its use)
constexpr int kMomentsMaxHalf = (kMomentsMaxIter + 1) / 2;
void launch_polar_moments(hipStream_t st, const AtomsDev &at, const double *dk, const double *e_static, int n_iter, double *scal);
void launch_polar_moments_and_pairs(hipStream_t st, const AtomsDev &at, const double *dk, const double *e_static, int n_iter,
                                    const double *block_part, const int *block_cnt, int nb, double *scal, long long *cnt);

// dense thole_amatrix rows (parity / DENSE solver)
// rows and columns are ORIGINAL atom indices; slot_of maps them to the device order
void launch_amatrix_rows(hipStream_t st, const AtomsDev &at, const int *slot_of, const Box &bx, double polar_damp, int row0, int nrows,
                         double *a /*[nrows][3n]*/);

// ---- symmetric production kernels (kernels_sym.hip) -------------------------------------------------------
struct FusedParams {
	double ewald_alpha, polar_ewald_alpha, polar_damp;
	int rd_lrc;
	int do_es;    // electrostatics on
	int do_field; // 0 none, 1 Ewald real_term, 2 thole_field_nopbc
	int do_thole; // write the (a,b) tensor store
	// adjacent physics (extended kernel variant only)
	int wolf;             // coulombic_wolf instead of the erfc term
	int fh_order;         // 0 off, 2 or 4: Feynman-Hibbs corrections
	double fh_c2, fh_c4;  // M2A2 hbar^2 / (24 kB T amu2kg),  M2A4 hbar^4 / (1152 kB^2 T^2 amu2kg^2)
	double wolf_erfa_over_r, wolf_inv_r2; // erf(alpha R)/R, 1/R^2
	double thole_far_x; // lambda r beyond which the exponential damping is dropped (the value the tile classes were made with)
	int store_only;     // nothing but the Thole tensor store (trial moves of polarizable boxes: energies and field come from the delta kernels)
	int touch_n;        // store-only passes: >= 0 restricts the pass to the tile pairs that contain one of touch[0 .. touch_n) (the tiles of
	int touch[8];       // the moved atoms: every other tile pair keeps the tensors it has); < 0: all tile pairs
	int pair_waves;     // waves per tile pair of the sweep: 4 for small tables (n_tile_pairs <= kPairSplitMax), else 1
};
// Tables up to this many tile pairs run everything on ONE stream: forking the side stream (reciprocal space, panel table) and joining it
// costs two cross-stream waits, more than the 20-odd us of work they overlap.  Measured (profiles/r02_one_stream.txt), one evaluation at
// a time: -11 % at 216 atoms, -7 % at 1000, -5 % at 2000, -2 % at 3000 (1128 tile pairs), level at 4000 (2016), +3 % at 5000, +2 % at
// 10 000; with 32 beads in flight: +7 % evaluations/s at 3000 atoms on one stream, level at 5000 and 7000, -2.6 % at 10 000.
constexpr int kOneStreamMaxPairs = 1536;
// Tables up to this many tile pairs run the pair sweep with four waves per tile pair.  Measured (profiles/r02_pair_waves.txt): one
// evaluation at a time four waves win at every size (-12 % at 216 atoms, -11 % at 3000, -7 % at 5000, -3 % at 7000, -1 % at 10 000);
// with 32 beads in flight they are level at 3000 atoms, +3..7 % at 5000, +1.4 % at 7000 (6105 tile pairs) and level (-0.3 %) at
// 10 000 (12 403) -- so the switch sits between the last size with a gain in both regimes and the first without one.
constexpr int kPairSplitMax = 8192;
// every unordered pair once: energies + counts (block partials), static-field partials fpart[nt][n_pad][3],
// Thole store ab[n_tile_pairs][64*64] (double2 = 16 B per pair)
// tp_list (may be null): the launch covers the tile pairs tp_list[0 .. n_tile_pairs) only -- what the fast sweep below leaves to it
void launch_pair_fused(hipStream_t st, const AtomsDev &at, const Box &bx, const FusedParams &fp, const int2 *tile_pairs,
                       const int *cls, int n_tile_pairs, double *block_part /*[ntp][2]*/, int *block_cnt /*[ntp][2]*/, double *fpart, double2 *ab,
                       const int *tp_list = nullptr);
// ---- the fast pair sweep (kernels_pair.hip): any cell, Ewald electrostatics with alpha r_c inside the erfc table; every tile pair
// except those with an atom that changes lj_mix (kAtomFlagsMixing: sigma < 0, dispersion coefficients) ----
struct PairSweepParams {
	double alpha_scaled_half, polar_damp_half, thole_far_x; // half of: the Ewald alpha over the erfc table's piece width, the Thole damping parameter (the sweep works with 2 r)
	int store;      // write the Thole tensor store
	int nt;         // tiles
	int have_shift; // tp_shift / CLS_UNIFORM_* are valid
	int split;      // 0 | 1 | 2: two waves per tile pair (half the steps each), two tile pairs per workgroup -- never / every entry / the entries behind n_main
	int n_main;     // workgroups [0, n_main) take whole entries of the table, the ones behind them half entries
	int fast;       // fused geometry with the tile pair's band around the cutoff thresholds (tp_shift.w); 0: the reference's form everywhere
};
// Tables with more tile pairs than this take the sweep by default.  Measured (profiles/r03_sweep_sizes.txt), k_pair_fused (four waves per
// tile pair up to kPairSplitMax) against the sweep: one evaluation at a time +2 % at 3000 atoms (1128 tile pairs), -3 % at 5000 (3160),
// -5 % at 7000, -9 % at 10 000; 32 beads in flight the sweep wins from 3000 atoms on (+4 % evaluations/s, +4.5 % at 5000, +9 % at 7000).
constexpr int kSweepMinPairs = 2048;
// two waves per tile pair (half the steps each; kernels_pair.hip): for the last kSweepSplitTailPermille / 1000 of the work table (round 5; round 4
// measured "all" against "none": faster alone, 0.7 % slower with 32 evaluations in flight)
constexpr int kSweepSplitTailPermille = 250;
// host: the device layout of the erfc table, 3 * 512 double2 = (c0,c1)[512], (c2,c3)[512], (c4,c5)[512]  (erfc_table.cpp)
constexpr int kErfTableDouble2 = 3 * 512;
void erfc_table_device_layout(double2 *out /*[kErfTableDouble2]*/);
// work table of the sweep: one workgroup per entry { J, I0 }, its four waves take the tile pairs (I0 .. I0+3, J); returns the
// number of entries (out may be null: count only)
int pair_sweep_blocks(int n_tiles, int2 *out);
// whether the sweep can serve this evaluation (switches, alpha r_c inside the erfc table).  Frozen, chargeless, sigma- or epsilon-less
// atoms are masked by the sweep itself (its MODE 2); only tile pairs with a kAtomFlagsMixing atom are skipped by it and must go
// through launch_pair_fused with their list (context.cpp builds it with the same constant)
bool pair_sweep_covers(const Box &bx, const FusedParams &fp, double ewald_alpha);
void launch_pair_sweep(hipStream_t st, const AtomsDev &at, const Box &bx, const FusedParams &fp, bool intra /*some molecule has more than one atom*/,
                       const int2 *blocks, int n_blocks, const int *cls, const double4 *tp_shift /*null: no uniform images*/,
                       const double2 *erf_tab, double *block_part, int *block_cnt, double *fpart, double2 *ab, int split_mode = 0 /*0 | 1 | 2: see PairSweepParams*/,
                       int n_split_tail = 0 /*mode 2: how many entries at the end of the table are halved*/, bool fast_geometry = false, int lds_pad_bytes = 0 /*unused dynamic LDS per workgroup: fewer workgroups per CU*/,
                       int replicas = 1 /*measurement only: the grid repeated in y (mpmc_debug_time_pair with panel_replicas)*/);
void launch_reduce_pairs(hipStream_t st, const double *block_part, const int *block_cnt, int nb, double *scal, long long *cnt);
// polarizable evaluations: launch_polar_energy and launch_reduce_pairs as the two blocks of one launch (the tail of the evaluation)
void launch_polar_energy_and_pairs(hipStream_t st, const AtomsDev &at, const double *mu, const double *e_static, const double *rrms_atom,
                                   const double *block_part, const int *block_cnt, int nb, double *scal, long long *cnt);
// LJ (+ counts) of a small system in ONE launch: no tile classes, the last-arriving block folds the partials and writes the scalar
// vector [S_COUNT doubles][C_COUNT int64][seq] into pinned host memory (seq last: a host polling that slot finds the results
// complete); `counter` is a zeroed int the kernel leaves zeroed
void launch_pair_lj_single(hipStream_t st, const AtomsDev &at, const Box &bx, const FusedParams &fp, const int2 *tile_pairs, int n_tile_pairs,
                           double *block_part, int *block_cnt, int *counter, double *out_host, double seq);
// S_ES_RECIP = (4 pi / V) sum_k w_k |S_k|^2 from the structure factors of this configuration
void launch_recip_energy(hipStream_t st, const RecipDev &rc, const Box &bx, double *scal);
// position-independent pair-flag counts (n_intra, n_rd_excluded, n_es_excluded, n_frozen): once per atom upload
void launch_static_counts(hipStream_t st, const AtomsDev &at, const int2 *tile_pairs, int n_tile_pairs, int *block_cnt /*[ntp][4]*/,
                          long long *cnt4);
// sum over intramolecular non-frozen pairs of q_i q_j erf(alpha r)/r with the plain (non-image) distance (:1503-1504)
void launch_intra_terms(hipStream_t st, const AtomsDev &at, const int *slot_of, double ewald_alpha, double *scal);
// per-tile bounding boxes (wrapped fractional coordinates) and tile-pair classes (CLS_*)
void launch_tile_classes(hipStream_t st, const AtomsDev &at, const Box &bx, const int2 *tile_pairs, int n_tile_pairs, double polar_damp,
                         double *tile_bounds /*[nt][12]*/, int *cls, double4 *tp_shift /*[ntp], may be null*/,
                         const double origin_f[3] /*fractional origin of the spatial sort: where the periodic wrap is cut*/,
                         double thole_far_x = kTholeFarX /*lambda r beyond which a tile pair is CLS_THOLE_FAR*/);
// one Jacobi contraction over all tile pairs (class read per block): part[nt][n_pad][3].  The matrix-free solver (and panels = 0);
// evaluations with a tensor store take the panel form below, in any cell
void launch_dipole_iter_hybrid(hipStream_t st, const AtomsDev &at, const Box &bx, const double *mu, const int2 *tile_pairs,
                               const int *cls, const double4 *tp_shift /*null: no uniform-image fast path*/, int n_tile_pairs,
                               const double2 *ab /*null: matrix-free, tensors inside the damping range rebuilt from the positions*/,
                               double *part, double polar_damp, const int *converged = nullptr);
// ---- panel form of the contraction (kernels_panel.hip; any cell): two tile pairs that share their j-tile per workgroup ----
int panel_segment_entries(int J); // entries the work table reserves for j-tile J; seg[J] = their running sum
// the work table of the panel kernel: per j-tile its diagonal tile pair, panels of two tile pairs of equal class, odd singles
void launch_build_panels(hipStream_t st, const int *cls, int n_tiles, const int *seg /*[n_tiles + 1]*/, int4 *panels);
// i-side partial sums -> part[J][I atoms] (the usual slots, upper triangle + diagonal only; [3][64] inside a slot); j-side -> gpart[entry][3][64]
void launch_dipole_iter_panel(hipStream_t st, const AtomsDev &at, const Box &bx, const double *mu, const int2 *tile_pairs,
                              const double4 *tp_shift, const int4 *panels, int n_entries, const double2 *ab, double *part, double *gpart,
                              const int *converged = nullptr, long long *trace = nullptr /*measurement only (trace_panel)*/,
                              int replicas = 1 /*measurement only: the grid repeated in y (mpmc_debug_time_panel)*/);
// new_mu = alpha (E0 + F) from the panel kernel's slots, one workgroup per tile (the launch that follows every panel contraction)
void launch_dipole_update_panel(hipStream_t st, const AtomsDev &at, const double *e_static, const double *part, const double *gpart, const int *seg,
                                const double *mu_old, double *mu_new, double *e_induced, int want_rrms, double *rrms_atom, double allowed_sqerr,
                                int *ctl, int *host_flag, int it, double *dk = nullptr /*as launch_dipole_update*/, const RelaxWeights *relax = nullptr /*likewise*/);
// lane-rotation primitive self-test: out[l] = lane whose value lane l received (must be (l+1)&63)
void launch_rot_selftest(hipStream_t st, int *out);

// ---- dense solver (kernels_dense.hip): the reference's 3N x 3N layout, contraction on the fp64 matrix cores ------------------------
// a: (3 n_pad)^2 doubles, slot order, diagonal 3x3 blocks and padded slots zero
void launch_dense_build(hipStream_t st, const AtomsDev &at, const Box &bx, double polar_damp, double *a, bool upper_only = false);
// the symmetric form (default): tile pairs I <= J only, both products per 16 x 16 block; part[source tile][n_pad][3] like the other solvers
void launch_dense_symv(hipStream_t st, const double *a, int n_pad, const double *x, const int2 *tile_pairs, int n_tile_pairs, double *part);
// part[chunk][n_pad][3] = - (rows of the chunk of A) . x  (A symmetric); k_dipole_update sums the chunks
void launch_dense_matvec(hipStream_t st, const double *a, int n_pad, const double *x, int n_chunks, double *part);

// ---- direct dipole solve (kernels_chol.hip): `polar_iterative off`, A mu = E0 by a blocked Cholesky factorisation -------------------
constexpr int kCholNB = 64;     // block width: the diagonal block one workgroup factors in LDS, the tile of the trailing update
constexpr int kCholPanel = 192; // panel width (three blocks = the rows of one atom tile): rank of the trailing update behind a panel
// unknowns 3 n_pol rounded up to whole panels (the matrix is np x np doubles, lower triangle used)
inline int chol_padded(int n_pol) { return (3 * n_pol + kCholPanel - 1) / kCholPanel * kCholPanel; }
// pol_list[n_pol]: slots of the atoms with alpha != 0 (written here); m: the lower triangle of thole_amatrix restricted to them
void launch_chol_build(hipStream_t st, const AtomsDev &at, const Box &bx, double polar_damp, int *pol_list, int n_pol, int np, double *m);
// b[np] = E0 of the unknowns; clears status[0]
void launch_chol_rhs(hipStream_t st, const int *pol_list, int n_pol, int np, const double *e_static, double *b, int *status);
// m = L (in place); status[0] = 1-based index of the first non-positive pivot, else 0 (every later kernel then returns at once)
void launch_chol_factor(hipStream_t st, double *m, int np, int *status);
// v0 = right-hand side in, solution out; v1 = scratch (both np long)
void launch_chol_solve(hipStream_t st, const double *m, int np, double *v0, double *v1, const int *status);
void launch_chol_scatter(hipStream_t st, const int *pol_list, int n_pol, const double *x, double *mu /*zeroed by the caller*/, const int *status);
// info[3] = { status, max |E0 + e_induced - mu / alpha|, max |E0| }; e_induced in: -(A_off mu) of one contraction, out: mu / alpha - E0
void launch_chol_finish(hipStream_t st, const AtomsDev &at, const double *mu, const double *e_static, double *e_induced, const int *status,
                        double *info);

// ---- Gauss-Seidel sweeps (kernels_gs.hip): `polar_gs on`, identity atom order, matrix-free ---------------------------
// one sweep over all tiles in atom order: mu is updated in place, e_induced receives each atom's induced field.  part: the slots of the
// symmetric kernel [nt][n_pad][3]; U, L: [n_pad][3] (tiles above / below); tile_pairs, cls, tp_shift: this evaluation's tile-pair tables
size_t gs_block_store_elements(int n_tiles); // double2 elements of the in-tile block store of the Gauss-Seidel sweeps
void launch_gs_blocks(hipStream_t st, const AtomsDev &at, const Box &bx, double polar_damp, double2 *blocks);
void launch_gs_sweep(hipStream_t st, const AtomsDev &at, const Box &bx, double polar_damp, const double *e_static, double *mu, double *e_induced,
                     double *part, const int2 *tile_pairs, const int *cls, const double4 *tp_shift, int n_tile_pairs, double *U, double *L,
                     const double2 *blocks);
void launch_gs_finish(hipStream_t st, const AtomsDev &at, const double *mu_old, const double *mu_new, int want_rrms, double *rrms_atom,
                      double allowed_sqerr, int *not_done_flag);
// `polar_sor` / `polar_esor` behind a sweep (:3526-3536): out = w_new mu_swept + w_old mu_old for every slot; out may be mu_old itself
void launch_gs_blend(hipStream_t st, const AtomsDev &at, const double *mu_swept, const double *mu_old, double *out, const RelaxWeights &w);

// ---- `polar_gs_ranked` (kernels_gs_rank.hip): the rank pass, the sweep order and the ranked view of the sweeps above -----------------
struct GsRankInfoDev { // what the rank pass leaves on the device (copied to pinned memory in front of the post)
	unsigned long long min_r2_bits; // bits of the smallest squared image distance between polarizable atoms (all ones: no such pair)
	double rmin;                    // its root, or MAXVALUE
	int max_rank, n_moved;          // largest rank_metric; places of the order that differ from the identity
	int pad[2];
};
struct GsRankView { // the per-atom arrays of the view, each n_pad (x 3) long, in sweep order
	double4 *xyzq;
	double2 *lj;
	int2 *mf;
	double *alpha, *eps, *inv_molmass, *e_static, *mu;
};
struct GsRankScatter { // up to four [n_pad][3] vectors (null: skipped) and one [n_pad] array (may be null) from sweep order to atom order
	const double *src3[4];
	double *dst3[4];
	const double *src1;
	double *dst1;
};
// rmin, rank_metric[n_pad] and order[n_pad] (order[p] = the atom swept p-th; padded slots keep their places) of the resident positions
void launch_gs_rank(hipStream_t st, const AtomsDev &at, const Box &bx, const int2 *tile_pairs, int n_tile_pairs, GsRankInfoDev *info, int *rank_metric,
                    int *order);
// the order alone, of any keys: order[p] = the atom at place p of the stable descending order of key[0 .. n); tally2[1] += places that moved
void launch_gs_rank_order(hipStream_t st, const AtomsDev &at, const int *key, int *order, int *tally2);
void launch_gs_rank_gather(hipStream_t st, const int *order, const AtomsDev &src, const GsRankView &dst, const double *e_static, const double *mu);
void launch_gs_rank_scatter(hipStream_t st, const int *order, int n_pad, const GsRankScatter &v);

// ---- trial moves (kernels_delta.hip) ----------------------------------------------------------------------
// out4 = { d lj_pairs, d es_real(erfc part), d intramolecular term, E_recip of the trial structure factors }, dcnt2 = { d n_lj, d n_es }
// a trial move short enough to travel in the kernel arguments (no staging copy): trial positions + charge, slot and original index
constexpr int kMvInline = 8;
struct MvInline {
	double nw[kMvInline][4];
	int slot[kMvInline], orig[kMvInline];
};
void launch_commit_positions_inline(hipStream_t st, double4 *xyzq, const MvInline &inl, int m);
void launch_delta(hipStream_t st, const AtomsDev &at, const int *slot_of, const Box &bx, const RecipDev &rc,
                  const FusedParams &fp /*ewald_alpha and the Wolf / Feynman-Hibbs fields*/, int do_es,
                  const int *mv_slot, const int *orig_of_mv, const double4 *mv_new, int m, int *moved_idx, double4 *sf_trial,
                  double *block_part, int *block_cnt, double *out4, long long *dcnt2,
                  double *host_out /*pinned [kDeltaHostCount]: the D_* slots at delta_host_index, the launch number `seq` stored last*/, double seq,
                  const MvInline *inl = nullptr /*non-null: the move is in here (m <= kMvInline), the device lists are not read*/);
void launch_commit_positions(hipStream_t st, double4 *xyzq, const int *mv_slot, const double4 *mv_new, int m);
// polarizable boxes: e_real_trial = e_real + (real-space static field of the pairs with a moved atom, new minus old geometry);
// dk_part: scratch [n_tiles][m][3]
void launch_delta_field(hipStream_t st, const AtomsDev &at, const Box &bx, double polar_ewald_alpha, int polar_ewald, const int *mv_slot,
                        const double4 *mv_new, int m, int *moved_idx, const double *e_real, double *e_real_trial, double *dk_part);
// resident positions of the moved atoms <-> mv_new (call again to undo)
void launch_swap_positions(hipStream_t st, double4 *xyzq, const int *mv_slot, double4 *mv_new, int m);
// the reduction and post of launch_delta alone: nb block partials, the energy of sf_trial (do_ewald), the result into out4 / dcnt2 / host_out
void launch_delta_finish(hipStream_t st, const double *block_part, const int *block_cnt, int nb, const RecipDev &rc, const double4 *sf_trial, const Box &bx,
                         int do_ewald, double *out4, long long *dcnt2, double *host_out, double seq);

// ---- exchange moves (kernels_exchange.hip): trial insertion / removal of ONE molecule -------------------------------------------------------
// The molecule travels as a staged list of these records, whether its atoms are resident (removal) or not (insertion): what the slot arrays
// hold for an atom.  mf.x is the molecule's id: a resident atom with that id is one of the molecule's own (removal) and is never a partner;
// for an insertion it is an id no resident atom has.
struct XchAtom {
	double4 xyzq;  // position, charge
	double2 lj;    // |sigma|, sqrt(epsilon)
	int2 mf;       // molecule id, AF_* flags
	double inv_molmass;
};
static_assert(sizeof(XchAtom) == 64, "one staged exchange atom is 64 bytes");
// sg (+1 insertion, -1 removal) times [ pairs of the molecule's atoms with every other resident atom + the molecule's own pairs and
// intramolecular term ], sf_trial = sf + sg * (the molecule's phases); block partials [nt + 1][2] (the last one: the molecule's own block),
// then launch_delta_finish: the result block is that of launch_delta, signed changes of the accepted totals
void launch_exchange(hipStream_t st, const AtomsDev &at, const Box &bx, const RecipDev &rc, const FusedParams &fp, int do_es, const XchAtom *mol, int m,
                     double sg, double4 *sf_trial, double *block_part /*[nt + 1][2]*/, int *block_cnt /*[nt + 1][2]*/, double *out4, long long *dcnt2,
                     double *host_out, double seq);

// ---- batched insertion candidates (kernels_insert_batch.hip): nc trial poses of one molecule against the same accepted configuration ------
// What launch_exchange + launch_delta_finish leave for ONE insertion, per candidate: the signed changes and counts of the D_* block.
struct InsCandOut {
	double lj, es_real, es_intra, es_recip;
	long long n_lj, n_es;
};
constexpr int kInsBatchBlockCands = 8; // candidates a block runs against the resident loads it made once (no result depends on it)
constexpr int kInsBatchChunk = 256;    // candidates per launch chain: the scratch is [kInsBatchChunk] x { (nt + 1) partials, K structure factors }
// mol: [nc][m] staged records (sg = +1); sf_trial: [nc][K]; block_part / block_cnt: [nc][nt + 1][2]; out: [nc], every field written
void launch_insert_batch(hipStream_t st, const AtomsDev &at, const Box &bx, const RecipDev &rc, const FusedParams &fp, int do_es, const XchAtom *mol, int m, int nc,
                         double4 *sf_trial, double *block_part, int *block_cnt, InsCandOut *out);

// ---- Axilrod-Teller three-body dispersion (kernels_three_body.hip) --------------------------------------------------------------
// au[slot] = (a, u) per atom (context.cpp: three_body_coefficients; padding a = 0, u = 1).  Both launches leave kThreeBodyBlocks (or fewer)
// partials in `part` and write scale * their fixed-order sum to out[0].
constexpr int kThreeBodyBlocks = 8192;
long long three_body_tile_triples(int n_tiles);
int three_body_grid(long long work_items); // partials a launch over this many tile triples / tile pairs leaves
// the full sum over unordered triples
void launch_three_body(hipStream_t st, const AtomsDev &at, const double2 *au, const Box &bx, double scale, double *part, double *out);
// the change under a trial move: old positions resident, the moved atoms' new ones in mv_new; moved_idx: the all -1 slot map of the delta
// kernels (marked and cleared again inside)
void launch_three_body_delta(hipStream_t st, const AtomsDev &at, const double2 *au, const Box &bx, double scale, const int *mv_slot, const double4 *mv_new,
                             int m, int *moved_idx, double *part, double *out);

// ---- the pair-sum energy terms: disp-expansion, rd_crystal, the rd model.  One tile-pair walk and one moved-atom walk serve them all
// (pair_term_walk.h); each term's file states its payload, its admission rule and its pair function.  Every sum launch leaves kXBlocks (or
// fewer) partials per quantity in `part` (arrays kXBlocks apart) and writes their fixed-order sums side by side; every delta launch takes the
// old positions as resident and the moved atoms' new ones in mv_new, marks and clears again the all -1 slot map moved_idx, and writes the
// change of each quantity side by side.
//
// ---- dispersion-expansion repulsion/dispersion (kernels_disp.hip) ---------------------------------------------------------------
// co[slot] = (alpha, r0, s6, s8), t10[slot] = s10 with c_n,ij = s_n,i s_n,j (unit factors included; context.cpp: disp_coefficients;
// padding zeros).  out[0] = the pair sum; the full sum also writes lrc_pair and lrc_self to out[1] and out[2].
constexpr int kDispBlocks = 16384; // (12 403 tile pairs at 10 000 atoms: one per workgroup, no tail of doubled waves)
struct DispParams {
	int damp, schmidt; // damp_dispersion, schmidt_ff
};
void launch_disp_expansion(hipStream_t st, const AtomsDev &at, const double4 *co, const double *t10, const int2 *tile_pairs, int n_tile_pairs,
                           const Box &bx, const DispParams &dp, double lrc_pair, double lrc_self, double *part, double *out);
void launch_disp_expansion_delta(hipStream_t st, const AtomsDev &at, const double4 *co, const double *t10, const Box &bx, const DispParams &dp,
                                 const int *mv_slot, const double4 *mv_new, int m, int *moved_idx, double *part, double *out);

// ---- `rd_crystal`: the lattice-summed Lennard-Jones of System::lj (kernels_crystal.hip) --------------------------------------------
// shift[n] = the lattice vector S(n) = ((B[0] n0 + B[1] n1) + B[2] n2) of image n, n in [-(order-1), order-1]^3 in the reference's loop
// order (context.cpp: crystal_ready builds it on the host with the cutoff and the two thresholds below, after every change of the cell).
// out2 = { pair sum, image terms kept (a double: exact) }, or their changes; part: [2 kCrystalBlocks].
constexpr int kCrystalBlocks = 16384;
constexpr int kCrystalMinItems = 2048; // small tables split every tile pair's j range until about this many waves share the sum
struct CrystalParams {
	int n_img, centre;    // images in the table; index of n = (0, 0, 0), which rd_excluded pairs skip
	double t_pair;        // ri2 <= t_pair  <=>  sqrt(ri2) - 1e-12 < cut   (the pair contributes, :934)
	double t_img;         // r2 <= t_img    <=>  !(sqrt(r2) > cut)         (the image term is kept, :957)
	int fh_order;         // Feynman-Hibbs: 0 off, 2 or 4, with the constants of FusedParams
	double fh_c2, fh_c4;
};
int crystal_jsplit(int n_tile_pairs); // waves per tile pair of the sum (a function of the table alone: repeated evaluations agree to the bit)
void launch_crystal(hipStream_t st, const AtomsDev &at, const Box &bx, const CrystalParams &cp, const double4 *shift, const int2 *tile_pairs,
                    int n_tile_pairs, double *part, double *out2);
void launch_crystal_delta(hipStream_t st, const AtomsDev &at, const Box &bx, const CrystalParams &cp, const double4 *shift, const int *mv_slot,
                          const double4 *mv_new, int m, int *moved_idx, double *part, double *out2);

// ---- the rd model: another mixing rule and another pair function for the sum inside the cutoff (kernels_rd_model.hip) --------------
// sp[slot] = (sigma, sigma^2, sigma^3, sigma^6) per atom, sigma >= 0 (context.cpp: rd_model_ready; padding zeros); sqrt(epsilon) is
// AtomsDev::lj's.  part: [3 kRdModelBlocks].
constexpr int kRdModelBlocks = 16384;
struct RdModelParams {
	int form, mix;       // RD_FORM_*, RD_MIX_* (pair_math.h)
	double t_in;         // ri2 <= t_in: the form's distance test (Box::t_lj for the LJ form, Box::t_es for 14-7 and DREIDING)
	int fh_order;        // Feynman-Hibbs (LJ form only): 0 off, 2 or 4, with the constants of FusedParams
	double fh_c2, fh_c4;
};
// out3 = { pair sum, kept terms, tile pairs skipped }; cls: this evaluation's tile-pair classes (CLS_BEYOND_CUTOFF tile pairs are not
// walked), or null: every tile pair is walked
void launch_rd_model(hipStream_t st, const AtomsDev &at, const double4 *sp, const int2 *tile_pairs, const int *cls, int n_tile_pairs, const Box &bx,
                     const RdModelParams &rp, double *part, double *out3);
// out[0] = the LJ form's pair correction with the mixed parameters over every pair that is not frozen (the host caches it)
void launch_rd_model_lrc(hipStream_t st, const AtomsDev &at, const double4 *sp, const int2 *tile_pairs, int n_tile_pairs, int mix, double cutoff,
                         double volume, double *part, double *out);
// out2 = { change of the pair sum, change of the kept terms }
void launch_rd_model_delta(hipStream_t st, const AtomsDev &at, const double4 *sp, const Box &bx, const RdModelParams &rp, const int *mv_slot,
                           const double4 *mv_new, int m, int *moved_idx, double *part, double *out2);

// ---- the Silvera-Goldman H2 potential: a pair function of the distance alone over EVERY pair inside the cutoff (kernels_sg.hip) -----
// perm[slot] = the atom's index in the caller's list (Feynman-Hibbs: the molecule mass of the pair's FIRST atom there).  part: [2 kSgBlocks].
constexpr int kSgBlocks = 4096;
struct SgParams {
	int fh;      // feynman_hibbs: the second-order term of System::sg :1829-1847 (feynman_hibbs_order plays no part)
	double fh_c; // M2A^2 hBar^2 / (24 kB T amu): times 1 / (molecule mass, amu)
};
// out2 = { pair sum, kept terms }
void launch_sg(hipStream_t st, const AtomsDev &at, const int *perm, const int2 *tile_pairs, int n_tile_pairs, const Box &bx, const SgParams &sp, double *part,
               double *out2);
// out2 = { change of the pair sum, change of the kept terms }
void launch_sg_delta(hipStream_t st, const AtomsDev &at, const int *perm, const Box &bx, const SgParams &sp, const int *mv_slot, const double4 *mv_new, int m,
                     int *moved_idx, double *part, double *out2);

// ---- cavity_autoreject: the contact counts of mpmc_set_cavity_autoreject (kernels_contact.hip) -------------------------------------------
// Integer pair sums carried as doubles (exact).  sp: the rd model's per-atom table when `model` is set, the disp-expansion term's
// coefficient table co when `disp` is set (else unused, may be null).
constexpr int kContactBlocks = 16384;
enum : int { CA_RULE_SIGMA = 1, CA_RULE_ABSOLUTE = 2 }; // (mirror MPMC_AUTOREJECT_* of the public header: context.cpp asserts it)
struct ContactParams {
	int rules;          // CA_RULE_*
	int model, mix;     // sigma rule: sigma_ij by the rd model's rule RD_MIX_* from sp (model != 0), or by lj_mix (model == 0)
	int measure_frozen; // absolute rule: pairs of two frozen atoms are measured (polarization on, System.cpp:985)
	int disp, schmidt;  // sigma rule under the disp-expansion term: sigma_ij = r0_ij and alpha_ij from co = (alpha, r0, ..) in place of sp, no cutoff
	double repulsion;   // ... and its second test (cavity_autoreject_repulsion != 0): 315.775 exp(-alpha_ij (r - r0_ij)) > repulsion
	double scale;       // cavity_autoreject_scale
	double t_in;        // sigma rule: ri2 <= t_in, the rd function's own distance test (Box::t_lj for LJ, Box::t_es for 14-7 and DREIDING)
	double dmax;        // no contact at or beyond this distance: scale * (largest sigma, with a margin), respectively scale; infinite
	                    // under the repulsion test, which has no such bound here: every tile pair is walked
};
// out3 = { pairs replaced, absolute contacts, tile pairs skipped }.  tile_bounds (this evaluation's k_tile_bounds) and cls (scratch
// [n_tile_pairs]) non-null in an orthorhombic cell: tile pairs further apart than dmax are not walked; otherwise every tile pair is walked
void launch_contact(hipStream_t st, const AtomsDev &at, const double4 *sp, const int2 *tile_pairs, int n_tile_pairs, const Box &bx, const ContactParams &cp,
                    const double *tile_bounds, int *cls, double *part /*[3 kContactBlocks]*/, double *out3);
// out2 = { change of the pairs replaced, change of the absolute contacts } under a trial move
void launch_contact_delta(hipStream_t st, const AtomsDev &at, const double4 *sp, const Box &bx, const ContactParams &cp, const int *mv_slot,
                          const double4 *mv_new, int m, int *moved_idx, double *part, double *out2);

// exchange moves: the contacts of a staged molecule (XchAtom records, as launch_exchange's) with the residents, per candidate.  The plain
// term only (the exchange delta path has no rd model, rd_crystal or disp-expansion).  part: scratch [nc][nt][2] ints.  out2 (may be null; nc = 1):
// { sg * replaced, sg * absolute } as doubles, side by side; out_ll (may be null): [nc][2] the counts themselves.
void launch_exchange_contact(hipStream_t st, const AtomsDev &at, const Box &bx, const ContactParams &cp, const XchAtom *mol, int m, int nc, double sg, int *part,
                             double *out2, long long *out_ll);

// ---- `polar_wolf`: the Wolf static field, and the reduce of `polar_palmo` (kernels_wolf_field.hip)--------------------------------------
struct WolfFieldParams {
	double a;           // polar_wolf_alpha
	double c_gauss;     // 2 a / sqrt(pi)
	double cutoff_term; // a > 0: erfc(a R) / R^2 + 2 a / sqrt(pi) exp(-a^2 R^2) / R;  a = 0: 1 / R^2
};
WolfFieldParams wolf_field_params(double polar_wolf_alpha, double cutoff); // (host; follows every change of the cutoff: made per launch)
// the whole field into the real-space slots fpart[nt][n_pad][3] that launch_field_finalize adds up (polar_ewald = 0); cls: this
// evaluation's tile-pair classes
void launch_wolf_field(hipStream_t st, const AtomsDev &at, const Box &bx, const WolfFieldParams &wp, const int2 *tile_pairs, const int *cls,
                       int n_tile_pairs, double *fpart);
// trial moves: e_real_trial = e_real + (field of the pairs with a moved atom, new minus old geometry); dk_part: scratch [n_tiles][m][3];
// moved_idx: the all -1 slot map of the delta kernels (marked and cleared again inside)
void launch_wolf_field_delta(hipStream_t st, const AtomsDev &at, const Box &bx, const WolfFieldParams &wp, const int *mv_slot, const double4 *mv_new, int m,
                             int *moved_idx, const double *e_real, double *e_real_trial, double *dk_part);
// change = f_new - e_induced for polarizable atoms, 0 for the others; scal[S_PALMO] = -1/2 sum mu . change, added to scal[S_POLAR]
void launch_palmo_reduce(hipStream_t st, const AtomsDev &at, const double *mu, const double *f_new, const double *e_induced, double *change, double *scal);

// ---- `polar_ewald_full`: the induced field as an Ewald sum (kernels_ewald_full.hip) ----------------------------------------------------
struct EwaldFullParams {
	int vector_weight;    // MPMC_PEF_VECTOR_KWEIGHT: w_p = (8 pi / V) kw_p; 0: the reference's (8 pi / V) kw_z for every p
	double recip_scale;   // 8 pi / V
	double c_total;       // -4 pi / (3 V), on sum_j mu_j
	double c_self;        // 4 a^3 / (3 sqrt(pi)), on mu_i
	double allowed_sqerr; // (polar_precision DEBYE2SKA)^2
};
// once per evaluation: store[n_tile_pairs][64 * 64] = (-s1 / r^3, 3 s2 / r^5) per pair in the order the contraction walks it, zeros outside
// the predicate; cnt[tp] = pairs inside it (a tile pair with none is not written); n_pairs_out[0] = their sum
void launch_pef_fill(hipStream_t st, const AtomsDev &at, const Box &bx, double ewald_a, double polar_damp, const int2 *tile_pairs,
                     const int *cls /*this evaluation's tile-pair classes (CLS_BEYOND_CUTOFF tile pairs are skipped), or null*/, int n_tile_pairs, double2 *store,
                     int *cnt, long long *n_pairs_out);
// phases[K][n_pad] = (cos, sin)(k . r_i), raw positions (launch_pef_sf and launch_pef_finish take null for it: the phases are then recomputed)
void launch_pef_phases(hipStream_t st, const AtomsDev &at, const double4 *kvec, int K, double2 *phases);
// once per pass: part[source tile][n_pad][3] = the real-space induced field of `mu`, every slot written
void launch_pef_contract(hipStream_t st, const AtomsDev &at, const Box &bx, const double *mu, const int2 *tile_pairs, int n_tile_pairs, const int *cnt,
                         const double2 *store, double *part);
// psum[2 k], psum[2 k + 1] = Pc, Ps of k < K; psum[2 K .. 2 K + 2] = sum_j mu_j (fixed-order block sums)
void launch_pef_sf(hipStream_t st, const AtomsDev &at, const double4 *kvec, int K, const double2 *phases, const double *mu, double *psum);
// e_induced = slots + reciprocal + correction; mu_new = alpha (E0 + e_induced); not_done (may be null): set to 1 when a component moved by
// more than the allowed amount
void launch_pef_finish(hipStream_t st, const AtomsDev &at, const EwaldFullParams &ep, const double *e_static, const double *part, int n_tiles,
                       const double2 *phases, const double4 *kvec, const double4 *kw, int K, const double *psum, const double *mu_old, double *mu_new,
                       double *e_induced, int *not_done, const RelaxWeights *relax = nullptr /*new_dipoles :3196-3204: new_mu itself is the blend, the verdict sees it*/);

// ---- the cavity-bias grid (kernels_cavity.hip; System::cavity_update_grid, src/System.Cavity.cpp:15-188) --------------------------------
// Distances are r = ((dx dx) + dy dy) + dz dz, unfused, d = grid - atom / dart - grid; inside means r < t2 (the exact-threshold form of
// sqrt(r) < radius, mpmc_cavity_r2_threshold).  No minimum image.  Every result is an integer: nothing depends on an order of summation.
constexpr int kCavityChunk = 256;       // atoms / empty points staged in LDS at a time
constexpr int kCavityTargetWaves = 2048; // work items a launch aims for (256 CUs x 4 SIMDs x 2)
// how many slices of the atom range (n atoms) a grid of `points` sphere centres is binned in: a function of (points, n) alone
inline int cavity_atom_slices(long long points, int n) {
	const long long blocks = (points + 63) / 64;
	const long long want = (kCavityTargetWaves + blocks - 1) / blocks, most = ((long long)n + 63) / 64;
	return (int)(want < 1 ? 1 : (want > most ? (most < 1 ? 1 : most) : want));
}
// ... and how many slices of the open list a launch over n_darts darts walks: a function of (points, n_darts) alone
inline int cavity_dart_slices(long long points, int n_darts) {
	const long long blocks = ((long long)n_darts + 63) / 64;
	if (blocks < 1) return 1;
	const long long want = (kCavityTargetWaves + blocks - 1) / blocks, most = (points + kCavityChunk - 1) / kCavityChunk;
	return (int)(want < 1 ? 1 : (want > most ? (most < 1 ? 1 : most) : want));
}
// part[s][p] = atoms of slice s inside the sphere of point p; grid [points][3], atoms [n][3]; part is [slices][points rounded up to 64]
void launch_cavity_occupancy(hipStream_t st, const double *grid, int points, const double *atoms, int n, int slices, double t2, int *part);
// occ[p] = sum_s part[s][p]; open[] = the flat indices of the points with occ == 0, ascending; res[0] = their number.  wave_cnt: scratch, one
// int per 64 points.
void launch_cavity_compact(hipStream_t st, const int *part, int slices, int points, int *occ, int *wave_cnt, int *open, long long *res);
// res[1] = darts inside at least one empty sphere; darts are basis^T applied to dart_frac [n_darts][3] (the reference's loop order).  mask:
// scratch, [slices][dart waves].  n_darts == 0: res[1] = 0, no dart kernel runs.
void launch_cavity_darts(hipStream_t st, const double *grid, const int *open, const double *dart_frac, int n_darts, int slices, const double basis[9], double t2,
                         unsigned long long *mask, long long *res);

// ---- volume-change trial moves (kernels_volume.hip; System::volume_change, src/System.MonteCarlo.cpp:1235-1340) --------------------------
// out[slot] = the atom of that slot shifted by its molecule's com * s - com (charge copied; the padding slots copied): mass [n] and
// mol_first [n_mol + 1] in ORIGINAL atom order, every molecule's sums sequential in that order
void launch_volume_scale(hipStream_t st, const double4 *xyzq, const int *slot_of, const double *mass, const int *mol_first, int n_mol, int n, int n_pad, double s,
                         double4 *out);

// device-resident positions [n][3] in original atom order -> xyzq[slot].xyz (perm[slot] = original index)
void launch_set_positions(hipStream_t st, const double *pos_dev, const int *perm, double4 *xyzq, int n);

} // namespace mpmc
