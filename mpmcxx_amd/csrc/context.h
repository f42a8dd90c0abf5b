// context.h -- INTERNAL to libmpmc_energy.so: the device-resident state behind an mpmc_ctx handle and the helpers its translation units
// share (context.cpp: lifetime, box, options, atoms; evaluate.cpp: one energy evaluation and its pieces; trial.cpp: per-move delta
// energies; pi.cpp: the path-integral bead loop).  Not installed, not part of the C ABI (include/mpmc_energy.h).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <mutex>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/mpmc_energy.h"
#include "kernels.h"

using namespace mpmc;

namespace mpmc {
extern thread_local std::string g_create_error; // last create-time error of this thread (context.cpp)
}

struct EvPair {
	hipEvent_t a, b;
	int cls;
};

// Pinned host memory comes from the HIP runtime's own pool: an address freed by one context is handed to the next.  The runtime is not
// instrumented, so the sanitizer build (tools/host_tsan.sh) is told here what the pool's lock orders: every release happens before every
// later allocation -- otherwise the old owner's writes and the new owner's count as a race between two threads that never shared anything.
#if defined(__SANITIZE_THREAD__)
extern "C" void AnnotateHappensBefore(const char *file, int line, const volatile void *tag);
extern "C" void AnnotateHappensAfter(const char *file, int line, const volatile void *tag);
inline char g_pinned_pool_tag;
#endif
template <class T>
inline hipError_t pinned_alloc(T **p, size_t bytes) {
	hipError_t e = hipHostMalloc((void **)p, bytes);
#if defined(__SANITIZE_THREAD__)
	AnnotateHappensAfter(__FILE__, __LINE__, &g_pinned_pool_tag);
#endif
	return e;
}
inline hipError_t pinned_free(void *p) {
#if defined(__SANITIZE_THREAD__)
	AnnotateHappensBefore(__FILE__, __LINE__, &g_pinned_pool_tag);
#endif
	return hipHostFree(p);
}

// A grow-only buffer that owns its memory: device memory that starts from zeros and is counted in the context's bytes_total (DevBuf), or
// pinned host memory, neither filled nor counted (PinnedBuf).  Move-only.  The destructor frees without a context: a buffer dies with
// the context that owns it, and there is nothing left to account to.
struct mpmc_ctx;
template <class T, bool kPinned = false>
struct DevBuf {
	T *p = nullptr;
	size_t cap = 0; // elements (what bytes_total counts for p; the allocation itself is never shorter than one element)
	DevBuf() = default;
	DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
	DevBuf &operator=(DevBuf &&o) noexcept {
		std::swap(p, o.p), std::swap(cap, o.cap);
		return *this;
	}
	~DevBuf() { release(nullptr); } // (members of a context: it dies with them; a local buffer calls release(c) itself before it goes)
	operator T *() const { return p; }
	void release(mpmc_ctx *c); // frees; given a context, takes the bytes out of its count
	// Room for `need` elements: nothing to do when need <= cap; otherwise the old buffer goes (with its contents) and a fresh one of
	// max(need, grow_to) elements takes its place.  MPMC_OK, or the error code with c->err set and the buffer left empty.
	int reserve(mpmc_ctx *c, size_t need, size_t grow_to = 0);
};
template <class T>
using PinnedBuf = DevBuf<T, true>;

// Measurement / A-B switches (mpmc_debug_configure; the library reads no environment variable for any of them).  The defaults are the
// production path; none of them changes a result beyond the last bits (tests/test_gpu_round3_fixes.py holds every one to the reference).
struct mpmc_tuning {
	int stream_mode = -1;   // "side_stream": -1 by table size (kOneStreamMaxPairs), 0 never fork the side stream, 1 always
	int pair_kernel = 0;    // "pair_kernel": 0 the fast sweep (kernels_pair.hip) where it applies and the table is large, 1 never, 2 wherever it applies
	int pair_waves = 0;     // "pair_waves": waves per tile pair of k_pair_fused, 0 by table size (kPairSplitMax), 1 | 4
	int sort_grid = -1;           // "sort_grid": -1 the aligned-grid spatial order where the table is large enough (round 4), 0 the nested count-based bisection of rounds 1-3
	int sort_nx = 0, sort_ny = 0; // "sort_nx" / "sort_ny": > 0: the aligned grid with exactly this many x slabs / y strips (measurement)
	bool side_after_sweep = true; // "side_after_sweep": two streams: the side stream's kernels are enqueued behind the pair sweep's launch (0: in front, rounds 1-3)
	bool lazy_side_stream = true; // "lazy_side_stream": the side stream is created when an evaluation first forks, not with the context -- the runtime deals
	                              // hardware queues to streams in turn, and an ensemble that never forks then has its main streams on all four (+0.6 %)
	bool poll_retire = true;      // "poll_retire": a polled-for evaluation queries its streams afterwards so that the runtime retires the finished commands
	bool poll_long = true;        // "poll_long": evaluations of large tables are polled for before the wait synchronises the stream (0: rounds 1-3)
	bool dense_symmetric = true; // "dense_symmetric": the dense solver reads the upper block triangle of A only (0: rounds 1-3, the whole matrix)
	bool fast_geometry = true; // "fast_geometry": fused minimum image in the pair sweep, the reference's form only inside a 1e-9 band around the cutoff (0: everywhere)
	int pair_split = -1;    // "pair_split": two waves per tile pair in the fast sweep (half-length workgroups): -1 the last part of the table (round 5), 0 never | 1 everywhere
	int pair_split_tail = -1; // "pair_split_tail": per mille of the sweep's work table that is halved under pair_split = -1 (default kSweepSplitTailPermille)
	int sweep_order = 1; // "sweep_order": the pair sweep's work table by descending j-tile (1, round 5: the short rows with their partial entries end the launch; -2 to -4 % per lone
	                     // launch without field and store, level with them) | 0 ascending (rounds 3-4)
	int sweep_lds_pad = 2048; // "sweep_lds_pad": bytes of unused dynamic LDS on the pair sweep's launch when the side stream runs beside it: four
	                          // workgroups per CU instead of five (no loss: 133 -> 131 us) leave 30 KB of LDS for the reciprocal-space kernels, which otherwise
	                          // wait for sweep workgroups to retire (k_recip_sf_tab 68 -> 53 us beside the sweep; profiles/r05_one_evaluation_timeline.txt)
	bool use_panels = true; // "panels": panel form of the Jacobi contraction (orthorhombic cells, stored tensors); 0: one tile pair per workgroup
	bool no_uniform = false;   // "uniform_images" = 0: no tile-pair-wide periodic images
	bool no_classes = false;   // "tile_classes" = 0: every tile pair is "near" (nothing skipped, every tensor stored)
	bool single_launch = true; // "single_launch": small LJ-only boxes in one launch
	bool no_recip_tab = false; // "recip_table" = 0: one sincos per (k, atom) instead of the factorised phases
	bool no_sort = false;      // "spatial_sort" = 0: atoms stay in the caller's order
	bool no_order_carry = false; // "order_carry" = 0: every upload of the atom list sorts
	bool no_polar_delta = false; // "polar_delta" = 0: trial moves of polarizable boxes run a full evaluation
	bool no_inline_move = false; // "inline_move" = 0: trial moves always travel through the staging block
	bool no_contact_skip = false; // "contact_skip" = 0: the contact walk of cavity_autoreject walks every tile pair
	int virtual_device = -1;     // "virtual_device" = v >= 0 (test hook): mpmc_pi_allreduce treats this context as living on a device of its own (csrc/comm.cpp group_beads)
	int fail_next_wait = 0;      // "fail_next_wait" = 1: the next wait of this context fails as if the runtime had refused it (test of the recovery path)
	bool trace_panel = false;    // "trace_panel" = 1: per-workgroup time stamps of the panel kernel (tools/panel_trace.py)
	bool dipoles_on_demand = true; // "dipoles_on_demand" = 0: every evaluation runs all its Jacobi iterations at once (A/B against the on-demand path-integral loop)
	bool pef_phase_table = true;   // "pef_phase_table" = 0: `polar_ewald_full` recomputes (cos, sin)(k . r) in every pass instead of reading its table (A/B: profiles/ewald_full.txt)
	long long tensor_budget_mb = 4096; // "tensor_budget_mb": AUTO solver: largest tensor store it will allocate
	long long direct_budget_mb = -1;   // "direct_budget_mb": direct dipole solve: largest factor it will allocate (-1: what the device has free)
};

// What a context keeps across mpmc_set_atoms AND across a growth of its capacity (grow_capacity hands `kept` to the fresh context in one
// assignment).  Everything else of mpmc_ctx is rebuilt by the fresh context: the spatial order, the per-atom coefficients, every buffer.
struct mpmc_kept {
	mpmc_tuning tune;
	bool prof = false; // profiling (mpmc_set_profiling) and what it has measured so far
	mpmc_timings tim{};
	// how the host waits ended (mpmc_debug_wait_counters): polls that saw the device's post, polls that ran out of their budget (the
	// wait then fell back to a stream synchronisation), plain stream synchronisations, and yields taken inside long polls
	long long n_poll_hits = 0, n_poll_timeouts = 0, n_stream_syncs = 0, n_poll_yields = 0;
	long long n_uploads_carried = 0, n_uploads_sorted = 0; // (diagnostics: mpmc_debug_upload_counts)
	long long n_xch_delta = 0, n_xch_full = 0, n_xch_resums = 0; // (diagnostics: mpmc_debug_exchange_counts)
	long long n_ins_calls = 0, n_ins_cands = 0;                  // (diagnostics: mpmc_debug_insert_batch_counts)
	long long n_vol[4] = {0, 0, 0, 0}; // (diagnostics: mpmc_debug_volume_trial_counts) evaluated, accepted, rejected, evaluations made by a reject
	bool tb_enabled = false, tb_mk = false; // Axilrod-Teller term switched on; Midzuno-Kihara c9 (mpmc_set_axilrod_teller)
	bool de_enabled = false;                // disp-expansion term switched on (mpmc_set_disp_expansion); the atoms' dispersion flag is AF_DISP_RD then
	int de_flags = 0;                       // MPMC_DISP_*
	bool pw_enabled = false;                // `polar_wolf` (mpmc_set_polar_wolf), kept across mpmc_set_box and mpmc_set_options too
	double pw_alpha = 0.0;
	bool palmo_enabled = false;             // `polar_palmo` (mpmc_set_polar_palmo), likewise
	bool rc_enabled = false;                // `rd_crystal` (mpmc_set_rd_crystal), kept across mpmc_set_box and mpmc_set_options too
	int rc_order = 0;                       // rd_crystal_order
	int rdm_form = 0, rdm_mix = 0;          // the rd model (mpmc_set_rd_model), likewise: MPMC_RD_FORM_*, MPMC_RD_MIX_*; (0, 0) = the plain term
	bool sg_enabled = false;                // the Silvera-Goldman potential (mpmc_set_silvera_goldman), likewise
	bool pef_enabled = false;               // `polar_ewald_full` (mpmc_set_polar_ewald_full), likewise
	int pef_flags = 0;                      // MPMC_PEF_*
	int relax_scheme = 0;                   // `polar_sor` / `polar_esor` (mpmc_set_polar_relax), likewise: MPMC_POLAR_RELAX_*
	bool zodid = false;                     // `polar_zodid`, likewise
	bool gs_ranked = false;                 // `polar_gs_ranked` (mpmc_set_polar_gs_ranked), likewise
	bool on_demand = false;                 // mpmc_set_dipoles_on_demand: mpmc_energy / mpmc_energy_async stop at the iterations the energy needs
	int cav_grid = 0;                       // `cavity_bias` (mpmc_set_cavity_grid), likewise: cavity_grid_size, 0 = off
	double cav_radius = 0.0;                // cavity_radius
	int ca_rules = 0;                       // cavity_autoreject (mpmc_set_cavity_autoreject), likewise: MPMC_AUTOREJECT_*, 0 = off
	double ca_scale = 0.0, ca_repulsion = 0.0; // cavity_autoreject_scale, cavity_autoreject_repulsion
};

// A contiguous run of atoms with every per-atom array of mpmc_set_atoms: the molecule of an exchange trial, or a whole atom list
struct AtomRun {
	std::vector<double> pos, q, alpha, eps, sigma, mass; // (mass empty: none given)
	std::vector<int32_t> mol, frozen, disp;
	int size() const { return (int)q.size(); }
	void clear() { pos.clear(), q.clear(), alpha.clear(), eps.clear(), sigma.clear(), mass.clear(), mol.clear(), frozen.clear(), disp.clear(); }
};
// The sums of k_atom_terms_part (kernels.hip) over an atom list, on the host, and the atoms per flag class
constexpr int kXchSums = 34, kXchClasses = 16, kXchResum = 1024;
struct XchSums {
	double s[kXchSums] = {0};
	long long cls[kXchClasses] = {0}; // atoms by (AF_FROZEN, AF_NULL_RD, dispersion coefficients, AF_ZERO_Q): all pair_flags reads of an atom of another molecule
	int32_t mol_max = 0;              // largest molecule id of the list
};

struct ContactCounts { // cavity_autoreject (kernels_contact.hip): pairs replaced by MAXVALUE, absolute contacts
	int64_t replaced = 0, absolute = 0;
};
// What the context remembers of ONE configuration's totals, in three roles: `accepted` (the accepted configuration, valid with cache_valid),
// `trial.totals` (the evaluated trial) and `eval` (the last evaluation waited for).  wait_and_fill fills `eval` and nothing else; the entry
// point that waited decides: a complete energy() re-bases (rebase_on_eval), a full-evaluation trial takes `eval` as its trial record,
// mpmc_trial_accept ends in accepted = trial.totals.
struct ConfigTotals {
	mpmc_result res{};         // UNPENALISED: lj_pairs = the kernels' sum S, so that a trial's delta adds to S and not to S + n 1e40; the penalty of
	                           // cavity_autoreject is put on the copy that leaves the library (contact_deliver, evaluate.cpp)
	int64_t rc_terms = 0;      // rd_crystal: image terms (mpmc_rd_crystal_info's n_image_terms)
	int64_t rdm_terms = 0;     // the rd model: kept terms (mpmc_rd_model_info's n_terms)
	int64_t sg_terms = 0;      // Silvera-Goldman: kept terms (mpmc_silvera_goldman_info's n_terms)
	ContactCounts ca;          // cavity_autoreject: the contact counts
	int64_t frozen_pairs = -1; // cavity_autoreject: unmeasured pairs of two frozen atoms of this composition; -1: the resident list's own (ca_frozen_pairs)
};
// The open trial move (trial.cpp), as far as the host describes it: xch_replace_list carries it across mpmc_set_atoms as a whole.  What
// belongs to buffers or to the device (trial_seq, d_mv_*, mv_inline, the tile lists) stays in the context.
struct TrialState {
	bool open = false, evaluated = false, was_full = false, enqueued = false, noop = false;
	bool polar_delta = false; // took the incremental polarizable path (positions swapped on the device)
	bool inline_move = false; // the move travelled in the kernel arguments (mv_inline)
	int first = 0, count = 0;
	std::vector<double> pos_new, pos_old;
	// exchange trials (mpmc_trial_insert_begin / mpmc_trial_remove_begin): the open trial changes the composition by ONE molecule
	int xch_kind = 0;            // 0 a displacement, +1 an insertion, -1 a removal
	int xch_at = 0;              // index the molecule goes in front of / of its first atom (original order); `count` atoms
	AtomRun xch_mol;             // the molecule: as given (insertion) or copied from the host mirrors (removal)
	AtomRun xch_saved;           // full-evaluation trials: the accepted atom list, which a rejection puts back
	double xch_static[3] = {0, 0, 0}, xch_N = 0; // lrc_pair, lrc_self, es_self and countN of the evaluated trial composition
	ConfigTotals totals;         // of the evaluated trial
	// volume trials (mpmc_trial_volume_begin): every basis element times vol_s, every molecule shifted rigidly by com * vol_s - com
	bool volume = false;         // the open trial is one
	bool vol_swapped = false;    // the trial cell, positions, k tables and structure factors are the resident ones (vol_restore trades them back)
	bool vol_host_pos = false;   // pos_new holds the trial positions [n][3] and pos_old the shift of every molecule [n_molecules][3] (vol_host_positions)
	double vol_s = 1.0;
	Box vol_box{};               // the trial cell
	Box vol_acc_box{};           // what the evaluation of the trial replaced: the accepted cell, its two alphas, its position-independent terms
	double vol_acc_alpha[2] = {0, 0}, vol_acc_static[3] = {0, 0, 0};
	bool vol_acc_static_dirty = false;
	unsigned vol_acc_gen = 0;    // ... and the static_gen they belonged to
};

struct mpmc_ctx {
	mpmc_kept kept;
	int device = 0;
	hipStream_t stream = nullptr;
	// second stream for work that is independent of the main chain inside ONE evaluation (reciprocal space next to the
	// pair sweep; the far-field Jacobi kernel next to the streaming one); always joined back before results are used
	hipStream_t stream2 = nullptr;
	hipEvent_t ev_fork = nullptr, ev_join = nullptr;
	bool two_streams = true; // the side stream is forked in THIS evaluation (set per evaluation from stream_mode and the table size)
	int max_atoms = 0, max_pad = 0;
	int n = 0, n_pad = 0, n_tiles = 0, n_tile_pairs = 0, n_split = 1;
	int n_molecules = 0;
	double N_movable = 0; // countN
	std::string err;

	// host mirrors of the flattened System
	std::vector<double> h_pos, h_q, h_alpha, h_eps, h_sigma, h_mass;
	std::vector<int32_t> h_mol, h_frozen, h_disp;

	// spatial order: device slot k holds original atom perm[k]; slot_of[i] is the slot of original atom i.
	// Atoms are sorted (nested x / y / z bisection of the wrapped fractional coordinates) so that each tile of 64
	// consecutive slots is spatially compact; every result that leaves the library is returned in ORIGINAL order.
	std::vector<int32_t> perm, slot_of;
	int32_t *d_slot_of = nullptr, *d_perm = nullptr;
	bool atoms_dirty = true; // host mirror newer than the device arrays (full upload pending)

	// device atom arrays
	// the per-atom arrays below are pieces of ONE device block laid out like the pinned staging block of upload_atoms
	// ([xyzq][lj][mf][alpha][eps][inv_molmass][perm][slot_of], each max_pad long): an upload of the atoms is one copy
	DevBuf<char> d_atoms_blob;
	double4 *d_xyzq = nullptr;
	double2 *d_lj = nullptr;
	int2 *d_mf = nullptr;
	double *d_alpha = nullptr, *d_eps = nullptr, *d_inv_molmass = nullptr;

	// pair kernel
	// (the five per-tile-pair arrays are sized together, mpmc_set_atoms)
	DevBuf<int2> d_tile_pairs;
	DevBuf<double> d_block_part;    // [ntp][2]
	DevBuf<int> d_block_cnt;        // [ntp][4] (2 used by the pair kernel, 4 by the static-count kernel)
	DevBuf<int> d_cls;              // tile-pair classes (CLS_*), recomputed every evaluation
	DevBuf<double> d_tile_bounds;   // [n_tiles][12]: wrapped fractional lo/hi, raw Cartesian lo/hi
	DevBuf<double4> d_tp_shift;     // [n_tile_pairs] lattice vector components of the common image index (CLS_UNIFORM_X/Y/Z)
	DevBuf<int4> d_panels;          // work table of the panel form of the Jacobi contraction (k_build_panels), rebuilt every evaluation
	DevBuf<int> d_seg;              // [n_tiles + 1] first entry of every j-tile's segment of that table
	DevBuf<double> d_gpart;         // [entries][3][64] j-side partial sums, one slot per entry of the table
	DevBuf<long long> d_trace;      // measurement only (tune.trace_panel): [entries][4] start / end ticks, HW_ID, XCC_ID of every workgroup of the LAST panel launch
	int n_panel_entries = 0, seg_tiles = -1; // entries of the table / the tile count its layout was made for
	bool panels_built = false;       // this evaluation's classes carry CLS_GROUPED bits and d_panels is valid
	// the fast pair sweep (kernels_pair.hip): its erfc table, its work table { J, I0 } (depends on the tile count only) and the list of
	// tile pairs it leaves to k_pair_fused (a tile with a kAtomFlagsMixing atom -- sigma < 0 or dispersion coefficients: rebuilt with every upload)
	DevBuf<double2> d_erf_tab;
	DevBuf<int2> d_sweep_blocks;
	int n_sweep_blocks = 0, sweep_tiles = -1;
	DevBuf<int> d_generic_list;
	int n_generic = 0;
	std::vector<int> h_generic;
	int inflight_hint = 1; // evaluations the caller keeps in flight together with this one (mpmc_hint_in_flight; the PI loops set their bead count)
	bool last_pair_was_sweep = false; // (diagnostics: which kernel the last evaluation's pair pass ran)
	FusedParams last_fp{};            // the pair pass's parameters in the last evaluation: a copy of its plan's (mpmc_debug_time_pair replays it)
	bool last_fp_valid = false;
	int debug_panel_replicas = 1;     // mpmc_debug_configure "panel_replicas": grid repetitions of mpmc_debug_time_panel's launches
	PinnedBuf<double4> h_xyzq;       // PINNED host mirror of d_xyzq (slot order, max_pad entries): position updates copy from it asynchronously;
	hipEvent_t ev_xyzq = nullptr;    // marks the last copy out of it done -- whoever is about to write the mirror waits for that copy only
	bool xyzq_in_flight = false;     // (mirror_guard), not for the evaluations queued behind it
	std::vector<double> h_pos_sorted; // positions at the time of the last spatial sort
	// The spatial order is a locality heuristic: ANY permutation gives the same physics (sums in another order).  A contiguous insertion
	// or removal (uVT / Gibbs) therefore carries the order it finds -- the survivors keep their sequence, inserted atoms are appended --
	// instead of paying an O(N log N) host sort per move; a real sort follows once kTile atoms have come or gone since the last one.
	bool order_sorted = false;  // perm is a spatial sort of the current atom list (not the identity of small / Gauss-Seidel systems)
	bool order_carried = false; // set_atoms has already brought perm / slot_of up to date: upload_atoms does not sort
	bool atoms_dirty_order = false; // a NEW sort was asked for (cell, options, drift) and is pending: nothing is carried across it
	int edits_since_sort = 0;   // atoms inserted + removed since the last real sort
	double sort_origin_f[3] = {0, 0, 0}; // fractional coordinate at which the spatial sort cuts the periodic wrap
	hipStream_t sync_stream = nullptr;  // stream that carries this context's final copies (null: its own)
	std::vector<double> molmass_tmp; // (scratch of upload_atoms)
	PinnedBuf<long long> static_cnt; // pinned [4]: n_intra, n_rd_excluded, n_es_excluded, n_frozen (position independent; copied back behind every upload of the atoms)
	// upload_atoms stages every per-atom array in ONE persistent pinned block (eight truly asynchronous copies, no synchronisation);
	// ev_stage marks the copies done, the next upload waits for it before it refills the block
	PinnedBuf<char> h_kstage; // the same for the k-vector tables of build_k_tables ([kvec][kw][lvec][w_en], each K long: 16-byte types first)
	hipEvent_t ev_kstage = nullptr;
	bool kstage_in_flight = false;
	int lvec_kmax = -1;       // the integer l-vectors on the device belong to this kmax (they depend on nothing else)
	PinnedBuf<char> h_stage;
	hipEvent_t ev_stage = nullptr;
	bool stage_in_flight = false;
	// the position-independent terms (LRC, Ewald self) ride along with the next general evaluation when they are stale: static_gen
	// counts the events that make them stale, static_ride_gen is the count the pending evaluation's ride-along belongs to (0: none)
	unsigned static_gen = 1, static_ride_gen = 0;

	// position-independent scalars (pair LRC, self LRC, Ewald self term): functions of the atom parameters, the cell and the options
	// only -- computed once (k_atom_terms) whenever one of those changed, kept on the host, added when a result is assembled
	bool static_dirty = true;
	double h_static[3] = {0, 0, 0}; // lrc_pair, lrc_self, es_self
	DevBuf<int> d_counter;          // ticket counter of the single-launch small-system kernels (zero between launches)
	bool scal_clean = false;        // d_scal is all zeros (the post kernel of the last evaluation left it so): no clear needed in front of this one
	int poll_budget_us = 1000;      // ... for at most this long before the wait falls back to hipStreamSynchronize
	bool spin_on_post = false;      // the pending evaluation ends in k_post_results and is short: wait_and_fill polls the launch number first
	bool last_was_single = false;   // the pending evaluation wrote h_scal from the device: nothing to copy back
	double single_seq = 0;          // launch number the single-launch kernel posts behind its results (host polls h_scal[S_COUNT + C_COUNT])
	// scalars
	DevBuf<double> d_atom_part;   // scratch of launch_atom_terms (per-block partial sums)
	DevBuf<double> d_scal;
	long long *d_cnt = nullptr;   // (the counts' part of d_scal)
	PinnedBuf<double> h_scal;
	long long *h_cnt = nullptr;   // (the counts' part of h_scal)
	DevBuf<int> d_flag;
	PinnedBuf<int> h_flag;

	// reciprocal tables
	int K = 0;
	DevBuf<double4> d_kvec, d_kw; // the k tables, with d_lvec and d_w_en (build_k_tables sizes the four together)
	DevBuf<double4> d_sf;         // structure factors; trades places with d_sf_trial when a trial move is accepted
	DevBuf<int4> d_lvec;          // integer l-vectors of the k table
	DevBuf<double4> d_sf_part;    // [n_tiles][K] per-tile structure-factor partials (factorised phases)
	DevBuf<double> d_w_en;

	// polarization work
	DevBuf<double> d_e_recip_part, d_part, d_e_static, d_mu[2], d_e_induced, d_rrms;
	DevBuf<double2> d_gs_blocks; // Gauss-Seidel sweeps: the in-tile 3 x 3 blocks (k_gs_blocks)
	DevBuf<double> d_gs_ul; // Gauss-Seidel sweeps (kernels_gs.hip): [2][max_pad][3] induced-field parts from the tiles above / below
	int mu_cur = 0;
	// Fixed-count Jacobi solves (polar_moments_apply): d_k = mu_k - mu_(k-1) of the first ceil(n/2) iterations, slot 0 = mu_0; the energy
	// is the sum of their moments (k_polar_moments).  [ceil(n/2) + 1][3 n_pad]
	DevBuf<double> d_dk_ring;
	// dipoles on demand: the last evaluation stopped after pend_done of pend_target iterations; finish_pending_dipoles runs the rest
	enum { PEND_NONE = 0, PEND_OPEN = 1, PEND_DROPPED = 2 };
	int polar_pending = PEND_NONE; // PEND_DROPPED: the inputs of the open solve were overwritten before anybody asked for the dipoles
	int pend_done = 0, pend_target = 0;
	// dense A rows scratch
	DevBuf<double> d_arows;
	DevBuf<double> d_adense; // solver DENSE: the (3 n_pad)^2 matrix of thole_amatrix without its diagonal blocks
	// compact Thole tensor store: (a,b) per unordered pair, tile-pair major, 64*64 double2 per tile pair
	DevBuf<double2> d_ab;
	int solver_used = MPMC_SOLVER_MATRIX_FREE;
	// direct dipole solve (`polar_iterative off`, kernels_chol.hip): the factor (np x np doubles, lower triangle), the slot list of the
	// polarizable atoms, two vectors of np doubles, { status } on the device and { status, max |r|, max |E0| } on the device / pinned
	DevBuf<double> d_chol, d_chol_v, d_chol_info;
	PinnedBuf<double> h_chol_info;
	DevBuf<int> d_chol_list, d_chol_status;
	bool direct_ran = false;       // the pending / last evaluation solved the dipoles directly
	mpmc_direct_info direct{};     // of the last such evaluation (filled by wait_and_fill)

	Box box{};
	double box_in[20] = {0}; // what mpmc_set_box was last called with (basis, reciprocal, volume, cutoff): an identical call is a no-op
	bool box_in_has_recip = false;
	bool box_set = false, atoms_set = false, opts_set = false, k_dirty = true;
	mpmc_options opts{};      // what the evaluations read: opts_user, and under the Silvera-Goldman term rd_only on and polarization off (effective_options)
	mpmc_options opts_user{}; // what mpmc_set_options was last called with
	double ewald_alpha = 0, polar_ewald_alpha = 0;

	// results of the last evaluation
	bool pending = false;
	bool have_polar = false;
	int iters = 0, failed = 0;
	unsigned run_mask = 0;

	// trial moves (delta energies)
	bool cache_valid = false;   // `accepted` = totals of the accepted configuration, d_sf = its structure factors
	ConfigTotals accepted, eval; // (the three roles of the record: ConfigTotals)
	TrialState trial;
	int trial_last_kind = -1; // (diagnostics) the last enqueued trial: 1 full evaluation, 0 delta energies
	int *d_mv_slot = nullptr, *d_mv_orig = nullptr; // d_mv_slot/d_mv_orig/d_mv_new live in ONE allocation (d_mv_blob)
	double4 *d_mv_new = nullptr;
	DevBuf<int> d_moved_idx;
	DevBuf<double4> d_sf_trial;
	// polarizable boxes: the real-space static field of the accepted configuration (k_field_finalize) and of the trial one
	// (e_real + delta of the pairs with a moved atom); they trade places on accept.  dk_part: scratch of k_field_delta.
	DevBuf<double> d_e_real, d_e_real_trial, d_dk_part;
	bool e_real_valid = false;     // d_e_real describes the accepted configuration
	// the tensor store between trial moves: a trial rebuilds only the tile pairs of the tiles its moved atoms live in; after a REJECTED
	// trial those tiles hold the rejected geometry's tensors and are rebuilt by the next trial (or by any full evaluation)
	std::vector<int> store_dirty_tiles, trial_tiles;
	int touch_n = -1, touch[8] = {0}; // what enqueue(RUN_STORE) passes to the store-only sweep (-1: all tile pairs)
	DevBuf<unsigned char> d_mv_blob; // device / pinned host staging of a trial's moved-atom list
	PinnedBuf<unsigned char> h_mv_blob;
	DevBuf<double> d_delta_out;    // [D_COUNT]
	PinnedBuf<double> h_delta_out; // [kDeltaHostCount]: d_delta_out's D_* slots at delta_host_index, the launch number k_delta_finish posts at kDeltaHostSeq (kernels.h)
	MvInline mv_inline{};          // the pending trial's move when it travelled in the kernel arguments (trial.inline_move)
	double trial_seq = 0;          // launch number of the pending trial's k_delta_finish
	long long *d_delta_cnt = nullptr, *h_delta_cnt = nullptr; // (the counts' part of d_delta_out / h_delta_out)

	// exchange trials (the open one: trial.xch_*)
	DevBuf<XchAtom> d_xch_mol;   // [MPMC_TRIAL_MAX_ATOMS] the staged molecule of the delta path
	PinnedBuf<XchAtom> h_xch_mol;
	// The position-independent terms of the trial composition come from the sums of k_atom_terms_part, kept on the host for the accepted
	// list (made at the first exchange trial after static_gen moved, O(N); an accepted exchange adds or subtracts its molecule, and every
	// kXchResum accepted ones the sums are made afresh so that rounding does not accumulate), with the histogram of the flag classes the
	// position-independent pair counts follow from.
	XchSums xs_acc, xs_trial;
	unsigned xs_gen = 0;         // static_gen of xs_acc (0: none)
	int xs_edits = 0;            // accepted exchanges since xs_acc was summed over the list

	// volume trials (mpmc_trial_volume_begin, kernels_volume.hip): all allocated by the first one.  The trial is evaluated into the
	// alternates -- d_vol_xyzq, the d_vol_k* tables, d_sf_trial -- which trade places with the accepted ones for as long as it is open
	// (d_xyzq is a pointer into the atom block: it points at d_vol_xyzq meanwhile, d_xyzq_acc keeps the block's own)
	DevBuf<double4> d_vol_xyzq;        // [max_pad] trial positions and charges, slot order
	double4 *d_xyzq_acc = nullptr;
	DevBuf<double4> d_vol_kvec, d_vol_kw; // the k tables of the other cell
	DevBuf<double> d_vol_w_en;
	DevBuf<double> d_vol_mass;         // [max_atoms] per-atom masses, ORIGINAL order (a re-sort does not touch them)
	DevBuf<int> d_vol_first;           // [n_molecules + 1] first atom of every molecule, original order; the last entry is n
	unsigned list_gen = 1, vol_list_gen = 0; // counts the atom lists (mpmc_set_atoms, accepted exchanges) / the one the two arrays above were made from (0: none)
	bool vol_zero_mass = false;        // ... and it has a molecule without mass: no centre

	// batched insertion candidates (mpmc_insert_candidates, kernels_insert_batch.hip): all allocated by the first call.  The staging block
	// holds one pass of candidates (kInsStageRecords records at the most), the device scratch one launch chain (kInsBatchChunk candidates).
	PinnedBuf<XchAtom> h_ins_mol;      // [pass][m]
	DevBuf<XchAtom> d_ins_mol;         // [pass][m]
	DevBuf<double4> d_ins_sf;          // [kInsBatchChunk][K] trial structure factors (Ewald electrostatics only)
	DevBuf<double> d_ins_part;         // [kInsBatchChunk][n_tiles + 1][2]
	DevBuf<int> d_ins_cnt;             // likewise
	DevBuf<InsCandOut> d_ins_out;      // [n_cand]
	PinnedBuf<InsCandOut> h_ins_out;   // [n_cand]

	// Axilrod-Teller three-body term (mpmc_set_axilrod_teller, kernels_three_body.hip)
	// (switched on: kept.tb_enabled, kept.tb_mk)
	bool tb_have = false;                   // coefficients set since the last mpmc_set_atoms
	bool tb_dirty = false;                  // d_tb_au is older than h_tb_au or than the spatial order
	std::vector<double> h_tb_au;            // [n][2] (a, u) per atom in original order (three_body_coefficients)
	DevBuf<double2> d_tb_au;                // [max_pad] the same in slot order, padding (0, 1)
	DevBuf<double> d_tb_part;               // [kThreeBodyBlocks] per-workgroup partials

	// dispersion-expansion term (mpmc_set_disp_expansion, kernels_disp.hip): replaces the LJ sums of rd_energy
	// (switched on: kept.de_enabled, kept.de_flags)
	bool de_have = false;      // coefficients set since the last mpmc_set_atoms
	bool de_dirty = false;     // d_de_co / d_de_t10 are older than h_de or than the spatial order
	std::vector<double> h_de;  // [n][5] (alpha, r0, sqrt c6, sqrt c8, t10) per atom in original order (disp_coefficients)
	std::vector<double> h_de_raw; // [n][3] c6, c8, c10 as given: the self LRC takes the unconverted values
	bool de_lrc_valid = false; // de_lrc holds the two long-range corrections of the volume / cutoff / rd_lrc below
	double de_lrc[2] = {0, 0}, de_lrc_volume = 0, de_lrc_cutoff = 0;
	int de_lrc_rd_lrc = 0;
	DevBuf<double4> d_de_co;   // [max_pad] (alpha, r0, sqrt c6, sqrt c8) in slot order, padding zeros
	DevBuf<double> d_de_t10;   // [max_pad]
	DevBuf<double> d_de_part;  // [kDispBlocks] per-workgroup partials

	// `rd_crystal` (mpmc_set_rd_crystal, kernels_crystal.hip; switched on: kept.rc_enabled, kept.rc_order): the lattice sum replaces the LJ
	// sum of rd_energy.  The image table, the cutoff with its thresholds and crystal_self follow the cell and the atom parameters: they
	// belong to the value of static_gen they were made at (crystal_ready, context.cpp); the two long-range corrections are h_static's,
	// taken at the crystal cutoff (lrc_box).
	unsigned rc_gen = 0;                    // static_gen of the table below (0: none)
	int rc_table_order = 0;                 // the order it was made for
	CrystalParams rc_par{};                 // n_img, centre, thresholds (the Feynman-Hibbs fields are filled per launch)
	double rc_cut = 0, rc_self = 0;         // 2 cutoff (order - 0.5); sum of rd_crystal_self
	DevBuf<double4> d_rc_shift;             // [n_img] lattice vectors of the images, reference order
	DevBuf<double> d_rc_part;               // [2 kCrystalBlocks] per-workgroup partials: energies, image-term counts
	struct mpmc_rd_crystal_info rc_info{};         // of the last evaluation with the term (mpmc_rd_crystal_info)

	// the rd model (mpmc_set_rd_model, kernels_rd_model.hip; kept.rdm_form, kept.rdm_mix): another mixing rule / pair function in place of the
	// LJ sums of rd_energy.  The per-atom table follows the spatial order (rebuilt behind every upload of the atoms: rd_model_ready); the LJ
	// form's pair correction follows the parameters, the flags, the volume, the cutoff, rd_lrc and the rule -- never the positions.
	bool rdm_dirty = true;                  // d_rdm_sp is older than the atom list or than the spatial order
	int rdm_bad_atom = -1;                  // first atom with sigma < 0 or epsilon < 0 of the current list (-1: none), found when the table is rebuilt
	DevBuf<double4> d_rdm_sp;               // [max_pad] (sigma, sigma^2, sigma^3, sigma^6) in slot order, padding zeros
	DevBuf<double> d_rdm_part;              // [3 kRdModelBlocks] per-workgroup partials: energies, kept terms, skipped tile pairs
	DevBuf<double> d_rdm_lrc;               // [1] the correction kernel's sum on its way to the host
	bool rdm_lrc_valid = false;             // rdm_lrc belongs to the values below and to the current table
	double rdm_lrc = 0, rdm_lrc_volume = 0, rdm_lrc_cutoff = 0;
	int rdm_lrc_rd_lrc = 0, rdm_lrc_mix = -1;
	struct mpmc_rd_model_info rdm_info{};   // of the last evaluation with a non-default model (mpmc_rd_model_info)

	// the Silvera-Goldman H2 potential (mpmc_set_silvera_goldman, kernels_sg.hip; kept.sg_enabled): sg() in place of lj(), and no electrostatics
	// and no polarization whatever the options say (System::energy :46) -- the context's `opts` are the caller's with rd_only on and
	// polarization off while the term is on, so every reader of the options behaves as on such a box.
	int sg_frozen_atoms = -1;               // frozen atoms of the current list (-1: not counted since the last upload)
	DevBuf<double> d_sg_part;               // [2 kSgBlocks] per-workgroup partials: energies, kept terms
	struct mpmc_silvera_goldman_info sg_info{}; // of the last evaluation with the term (mpmc_silvera_goldman_info)

	// cavity_autoreject (mpmc_set_cavity_autoreject, kernels_contact.hip; kept.ca_rules, kept.ca_scale); the contact counts of a configuration
	// travel in its record, next to the UNPENALISED result they belong to (ConfigTotals: accepted, trial.totals, eval)
	int64_t ca_walked = 0, ca_skipped = 0;        // tile pairs of the last full walk
	bool ca_dirty = true;                         // ca_sigma_max and ca_frozen_pairs are older than the atom list
	double ca_sigma_max = 0.0;                    // largest |sigma| of the list: scale * it bounds the sigma rule's contact distance
	int64_t ca_frozen_pairs = 0;                  // pairs of two frozen atoms of different molecules
	int64_t ca_frozen_atoms = 0;                  // frozen atoms of the list
	DevBuf<int> d_ca_xpart;                       // [candidates of a chain][n_tiles][2] per-tile contacts of a staged molecule (launch_exchange_contact)
	DevBuf<long long> d_ins_ca;                   // [n_cand][2] per-candidate contacts of the last batch of insertion candidates
	PinnedBuf<long long> h_ins_ca;                // likewise, on their way to the host
	std::vector<int64_t> ins_ca;                  // [n_cand][2] the last batch's counts of each candidate's trial composition (mpmc_insert_candidates_contacts)
	int ins_ca_n = -1;                            // candidates of that batch (-1: none yet)
	DevBuf<double> d_ca_part;                     // [3 kContactBlocks] per-workgroup partials
	DevBuf<int> d_ca_cls;                         // [n_tile_pairs] the contact walk's own tile-pair classes (k_contact_classes)
	struct mpmc_cavity_autoreject_info ca_info{}; // of the last result delivered (mpmc_cavity_autoreject_info)

	// `polar_wolf` / `polar_palmo` (mpmc_set_polar_wolf, mpmc_set_polar_palmo, kernels_wolf_field.hip; switched on: kept.pw_enabled, kept.pw_alpha,
	// kept.palmo_enabled)
	bool palmo_ran = false;          // the pending / last evaluation did the extra contraction (Gauss-Seidel sweeps that did not fail)
	double palmo_correction = 0.0;   // of the last evaluation with a dipole solve (wait_and_fill)
	DevBuf<double> d_palmo_f, d_palmo_change; // [max_pad][3]: -(A_off mu) of the final dipoles; ef_induced_change

	// `polar_ewald_full` (mpmc_set_polar_ewald_full, kernels_ewald_full.hip; switched on: kept.pef_enabled, kept.pef_flags)
	DevBuf<double2> d_pef_store;     // [n_tile_pairs][64 * 64] (-s1 / r^3, 3 s2 / r^5), filled once per evaluation
	DevBuf<int> d_pef_cnt;           // [n_tile_pairs] pairs inside the real-space predicate
	DevBuf<double2> d_pef_phases;    // [K][n_pad] (cos, sin)(k . r_i)
	DevBuf<double> d_pef_psum;       // [2 K + 3] Pc, Ps per k; sum of the dipoles
	DevBuf<long long> d_pef_pairs;   // [1] sum of d_pef_cnt
	PinnedBuf<long long> h_pef_pairs;
	bool pef_ran = false;            // the pending / last evaluation solved the dipoles with the term
	mpmc_ewald_full_info pef_info{}; // of the last such evaluation (n_real_pairs filled by wait_and_fill)

	// `polar_sor` / `polar_esor` / `polar_zodid` (mpmc_set_polar_relax; kept.relax_scheme, kept.zodid)
	mpmc_relax_info relax_info{}; // of the pending / last evaluation with a dipole solve

	// `polar_gs_ranked` (mpmc_set_polar_gs_ranked, kernels_gs_rank.hip; switched on: kept.gs_ranked): the rank pass of every evaluation and the
	// second set of per-atom arrays and tile tables, in sweep order, that the sweeps from the second iteration on run on
	DevBuf<char> d_gr_atoms;          // the view's per-atom arrays, laid out like d_atoms_blob
	DevBuf<double> d_gr_vec;          // [5][max_pad][3]: E0, the two dipole vectors, the induced field; rrms per atom in the last third
	DevBuf<int> d_gr_rank;            // [2][max_pad]: rank_metric, order (atom order = slot order: the sweeps keep the identity)
	DevBuf<GsRankInfoDev> d_gr_info;
	PinnedBuf<GsRankInfoDev> h_gr_info;
	DevBuf<double2> d_gr_blocks;      // k_gs_blocks of the view
	DevBuf<double> d_gr_bounds;       // tile bounding boxes, classes and common images of the view's tiles
	DevBuf<int> d_gr_cls;
	DevBuf<double4> d_gr_shift;
	bool gr_ran = false;              // the pending / last evaluation made a rank pass
	unsigned gr_pos_gen = 0, gr_static_gen = 0; // ... at these values of pos_gen / static_gen (mpmc_polar_gs_ranked_get asks for the current ones)
	mpmc_gs_ranked_info gr_info{};    // of the last evaluation with a dipole solve (rmin, max_rank, n_moved filled by wait_and_fill)

	// the cavity-bias grid of uVT moves (mpmc_set_cavity_grid / mpmc_cavity_update, cavity.cpp, kernels_cavity.hip; switched on: kept.cav_grid,
	// kept.cav_radius).  Nothing here is read or written by an evaluation or a trial; every buffer is made by the first update.
	unsigned pos_gen = 1;                 // counts the events that change h_pos (atom list, position updates, accepted trials)
	bool cav_valid = false;               // the results below are those of an update ...
	unsigned cav_pos_gen = 0, cav_static_gen = 0; // ... made at these values of pos_gen / static_gen (cavity_current)
	int cav_done_grid = 0;                // ... with this grid size
	double cav_done_radius = 0.0;         // ... and radius
	int64_t cav_open = 0;                 // cavities_open of that update
	double cav_basis[9] = {0};            // the cell h_cav_grid / d_cav_grid were made for, with cav_grid_G (0: none)
	int cav_grid_G = 0;
	std::vector<double> h_cav_grid;       // [G^3][3] sphere centres, enumeration order (i outermost, k innermost)
	std::vector<int32_t> h_cav_open;      // the open list on the host, fetched by the first mpmc_cavity_point / mpmc_cavity_get behind an update
	bool cav_open_cached = false;
	DevBuf<double> d_cav_grid;            // [G^3][3]
	DevBuf<double> d_cav_in;              // [n][3] wrapped positions, then [n_darts][3] fractional darts
	PinnedBuf<double> h_cav_in;           // their staging
	DevBuf<int> d_cav_part;               // [slices][points padded to 64] occupancy partials
	DevBuf<int> d_cav_occ;                // [points padded to 64]
	DevBuf<int> d_cav_wave;               // [point waves] empty points per wave, then their exclusive prefix
	DevBuf<int> d_cav_open;               // [points] flat indices of the empty points, ascending
	DevBuf<unsigned long long> d_cav_mask; // [open slices][dart waves] hit masks
	DevBuf<long long> d_cav_res;          // { cavities_open, hits }
	PinnedBuf<long long> h_cav_res;
	hipEvent_t cav_ev[4] = {nullptr, nullptr, nullptr, nullptr}; // profiling: around the three kernel groups of the last update
	float cav_ms[3] = {0, 0, 0};          // occupancy, compaction, darts of the last update made under mpmc_set_profiling

	std::vector<EvPair> ev_free, ev_used; // profiling (kept.prof): event pairs to reuse / recorded and not yet harvested into kept.tim

	int64_t bytes_total = 0; // device memory held by this context's DevBuf members (mpmc_memory_usage)
};

// ---------------------------------------------------------------------------------------------------------
#define HIP_TRY(ctx, call)                                                                                        \
	do {                                                                                                          \
		hipError_t _e = (call);                                                                                   \
		if (_e != hipSuccess) {                                                                                   \
			(ctx)->err = std::string(#call) + ": " + hipGetErrorString(_e);                                       \
			return MPMC_ERR_HIP;                                                                                  \
		}                                                                                                         \
	} while (0)

template <class T, bool kPinned>
inline void DevBuf<T, kPinned>::release(mpmc_ctx *c) {
	if (p) (void)(kPinned ? pinned_free(p) : hipFree(p));
	if (p && c && !kPinned) c->bytes_total -= (int64_t)(cap * sizeof(T));
	p = nullptr, cap = 0;
}
template <class T, bool kPinned>
inline int DevBuf<T, kPinned>::reserve(mpmc_ctx *c, size_t need, size_t grow_to) {
	if (need <= cap) return MPMC_OK;
	release(c);
	const size_t count = std::max(need, grow_to), bytes = std::max<size_t>(count, 1) * sizeof(T);
	hipError_t e = kPinned ? pinned_alloc(&p, bytes) : hipMalloc((void **)&p, bytes);
	if (e != hipSuccess) p = nullptr;
	// Every device buffer starts from zeros: what a kernel finds in a slot it has not written yet must not depend on what an earlier process
	// left in that memory.  The fill is WAITED for -- the first writer may be a side-stream kernel that is not ordered behind a fill on the
	// main stream (seen when evaluations still allocated after the side stream was forked: structure factors zeroed under the
	// reciprocal-space kernels; an evaluation now makes all its room before its first launch, make_room in evaluate.cpp, and the wait
	// stays for every other caller).  Allocations happen once per context, the wait costs nothing in steady state.
	// (The fill is on the context's stream; nothing in this library touches the null stream, which is unordered against our non-blocking ones.)
	if (e == hipSuccess && !kPinned && (e = hipMemsetAsync(p, 0, bytes, c->stream)) == hipSuccess) e = hipStreamSynchronize(c->stream);
	if (e != hipSuccess) {
		release(nullptr);
		c->err = std::string(kPinned ? "pinned host" : "device") + " allocation of " + std::to_string(bytes) + " bytes: " + hipGetErrorString(e);
		return MPMC_ERR_HIP;
	}
	cap = count;
	if (!kPinned) c->bytes_total += (int64_t)(count * sizeof(T));
	return MPMC_OK;
}

namespace mpmc { // internal helpers: mangled names, nothing here can collide with a symbol of the host program

constexpr size_t kAtomRecordBytes = sizeof(double4) + sizeof(double2) + sizeof(int2) + 3 * sizeof(double) + 2 * sizeof(int32_t); // per atom, all arrays of the block
// carve the per-atom arrays out of a block of P records (device block and pinned staging block share the layout)
template <typename F>
inline void atom_block_layout(char *base, size_t P, F &&set) {
	double4 *xyzq = reinterpret_cast<double4 *>(base);
	double2 *lj = reinterpret_cast<double2 *>(xyzq + P);
	int2 *mf = reinterpret_cast<int2 *>(lj + P);
	double *al = reinterpret_cast<double *>(mf + P), *ep = al + P, *imm = ep + P;
	int32_t *perm = reinterpret_cast<int32_t *>(imm + P), *slot = perm + P;
	set(xyzq, lj, mf, al, ep, imm, perm, slot);
}
// before the slot-ordered mirror is written: the last asynchronous copy out of it must have read it
inline int mirror_guard(mpmc_ctx *c) {
	if (c->xyzq_in_flight) {
		HIP_TRY(c, hipEventSynchronize(c->ev_xyzq));
		c->xyzq_in_flight = false;
	}
	return MPMC_OK;
}

inline int fail(mpmc_ctx *c, int code, const std::string &msg) {
	if (c) c->err = msg;
	else g_create_error = msg;
	return code;
}

// Poll a pinned word the device posts behind its results (system-scope release on the device side) until `seen()` or until `budget` has
// passed; true = seen.  A short evaluation ends a few microseconds earlier this way than through the driver's completion path.  Past
// 50 us the poller yields between checks: on a host with fewer free cores than polling / OpenMP threads (one run of fourteen in round 2
// took 3.5 ms per Monte Carlo step instead of 0.13 -- the signature of spinning threads time-slicing on too few cores) a spinning thread
// must not keep the thread that would feed the device off the CPU.  The counters tell afterwards which way the waits went.
template <class Pred>
inline bool poll_posted(mpmc_ctx *c, Pred seen, std::chrono::microseconds budget) {
	const auto t0 = std::chrono::steady_clock::now();
	for (int spins = 0;; ++spins) {
		if (seen()) {
			std::atomic_thread_fence(std::memory_order_acquire);
			c->kept.n_poll_hits++;
			return true;
		}
		if ((spins & 255) == 255) {
			const auto dt = std::chrono::steady_clock::now() - t0;
			if (dt > budget) {
				c->kept.n_poll_timeouts++;
				return false;
			}
			if (dt > std::chrono::microseconds(50)) {
				c->kept.n_poll_yields++;
				std::this_thread::yield();
			}
		}
	}
}

// ---- profiling ------------------------------------------------------------------------------------------
inline void prof_begin(mpmc_ctx *c, int cls, int &cur, hipStream_t st) {
	cur = -1;
	if (!c->kept.prof) return;
	EvPair e;
	if (!c->ev_free.empty()) {
		e = c->ev_free.back();
		c->ev_free.pop_back();
	} else {
		if (hipEventCreate(&e.a) != hipSuccess || hipEventCreate(&e.b) != hipSuccess) return;
	}
	e.cls = cls;
	(void)hipEventRecord(e.a, st);
	c->ev_used.push_back(e);
	cur = (int)c->ev_used.size() - 1;
}
inline void prof_end(mpmc_ctx *c, int cur, hipStream_t st) {
	if (cur >= 0 && cur < (int)c->ev_used.size()) (void)hipEventRecord(c->ev_used[cur].b, st);
}
inline void prof_harvest(mpmc_ctx *c) { // stream must be idle
	for (auto &e : c->ev_used) {
		float ms = 0;
		if (hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) {
			c->kept.tim.ms[e.cls] += ms;
			c->kept.tim.launches[e.cls] += 1;
		}
		c->ev_free.push_back(e);
	}
	c->ev_used.clear();
}
struct ProfScope { // HIP-event bracket on the stream the kernels are launched on
	mpmc_ctx *c;
	int cur;
	hipStream_t st;
	ProfScope(mpmc_ctx *c_, int cls, hipStream_t st_ = nullptr) : c(c_), st(st_ ? st_ : c_->stream) { prof_begin(c, cls, cur, st); }
	~ProfScope() { prof_end(c, cur, st); }
};
// side stream: starts after everything enqueued so far on the main stream / main stream waits for the side stream
inline hipStream_t fork_side(mpmc_ctx *c) {
	if (!c->two_streams) return c->stream;
	if (!c->stream2 && hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking) != hipSuccess) { // (lazy_side_stream)
		c->stream2 = nullptr;
		c->two_streams = false;
		return c->stream;
	}
	(void)hipEventRecord(c->ev_fork, c->stream);
	(void)hipStreamWaitEvent(c->stream2, c->ev_fork, 0);
	return c->stream2;
}
inline void join_side(mpmc_ctx *c) {
	if (!c->two_streams || !c->stream2) return;
	(void)hipEventRecord(c->ev_join, c->stream2);
	(void)hipStreamWaitEvent(c->stream, c->ev_join, 0);
}


// ---- shared between the translation units ---------------------------------------------------------------------
enum : unsigned {
	RUN_PAIR = 1, RUN_PAIR_ES = 2, RUN_RECIP = 4, RUN_ATOMTERMS = 8, RUN_FIELD = 16, RUN_SOLVE = 32, RUN_WOLF = 64,
	RUN_STORE = 128, // tile classes + the Thole tensor store alone (no energies, no field): trial moves of polarizable boxes
	RUN_THREE_BODY = 256, // the Axilrod-Teller sum (contexts with the term switched on)
	RUN_DISP = 512,       // the disp-expansion sum (contexts with the term switched on: it replaces the LJ part of rd_energy)
	RUN_CRYSTAL = 1024,   // the rd_crystal lattice sum (contexts with the term switched on and disp-expansion off: it replaces the LJ sum)
	RUN_RDM = 2048,       // the rd-model sum (contexts with a non-default model: it replaces the LJ part of rd_energy)
	RUN_CONTACT = 4096,   // the contact walk of cavity_autoreject (contexts with a rule on; never the single-launch form)
	RUN_SG = 8192         // the Silvera-Goldman sum (contexts with the term switched on: it is the whole of rd_energy, and no pair pass runs beside it)
};
// 3 x the unit factor of System::axilrod_teller (hartree bohr^9 -> K A^9, src/System.Energy.cpp:1709): the mixing rule's 3 and the units,
// applied once to the sum of the per-triple terms
constexpr double kThreeBodyScale = 3.0 * (0.0032539449 / (3.166811429 * 0.000001));
int three_body_ready(mpmc_ctx *c); // the term is on and its coefficients are on the device in the current slot order (context.cpp)
int disp_ready(mpmc_ctx *c);       // the same for the disp-expansion term, and its long-range corrections for the current box (context.cpp)
DispParams disp_params(const mpmc_ctx *c);
inline bool rd_model_on(const mpmc_ctx *c) { return c->kept.rdm_form != 0 || c->kept.rdm_mix != 0; }
// (disp_expansion() ignores rd_crystal, and so do lj_buffered_14_7() and dreiding())
// (... and so does sg())
inline bool crystal_on(const mpmc_ctx *c) { return c->kept.rc_enabled && !c->kept.de_enabled && c->kept.rdm_form == 0 && !c->kept.sg_enabled; }
inline bool sg_on(const mpmc_ctx *c) { return c->kept.sg_enabled; }
int sg_ready(mpmc_ctx *c);         // the term's combinations and the list are valid (no model, no disp-expansion, no sigma rule, fewer than two frozen atoms), the partials stand (context.cpp)
SgParams sg_params(const mpmc_ctx *c); // feynman_hibbs and its constant at this temperature (context.cpp)
// the options the evaluations read: the caller's, and under the Silvera-Goldman term rd_only on and polarization off (System::energy :46)
inline mpmc_options effective_options(const mpmc_ctx *c, const mpmc_options &user) {
	mpmc_options o = user;
	if (c->kept.sg_enabled) o.rd_only = 1, o.polarization = 0;
	return o;
}
void apply_options(mpmc_ctx *c, const mpmc_options &eff); // the evaluations' options change: the order rule, the open solve, the k tables, the static terms, the accepted totals (context.cpp)
int rd_model_ready(mpmc_ctx *c);   // the model's combinations and atom parameters are valid, its table is on the device in the current slot order, its correction is current (context.cpp)
RdModelParams rd_model_params(const mpmc_ctx *c); // form, rule, distance test and this evaluation's Feynman-Hibbs constants (evaluate.cpp)
inline bool contact_on(const mpmc_ctx *c) { return c->kept.ca_rules != 0; }
int contact_ready(mpmc_ctx *c);    // the rules' combinations are valid, the list's largest sigma and frozen pairs are current, the buffers stand (context.cpp)
ContactParams contact_params(const mpmc_ctx *c); // rules, scale, the rd function's distance test and mixing, dmax (context.cpp)
// the copy of a result that leaves the library: the sigma rule's n 1e40 on lj_pairs (rd_energy, energy, NU follow), and the info struct of
// this delivery (evaluate.cpp)
// (t: the record of the delivered configuration; its contact counts and its unmeasured frozen pairs)
void contact_deliver(mpmc_ctx *c, mpmc_result *r, const ConfigTotals &t);
void contact_penalise(const mpmc_ctx *c, mpmc_result *r, int64_t n_replaced); // the sigma rule's n 1e40 on lj_pairs; rd_energy, energy, NU follow
// The one composition of a result's totals (evaluate.cpp): rd_energy from lj_pairs, lrc_pair and lrc_self in the given form, then energy
// and NU from the components and N already in *r.  A trial's delta adds to the accepted totals because everybody composes here, in one
// association order.  The caller names the form: an evaluation by what it ran, a trial by the terms that are on (rd_form_of).
enum class RdForm {
	PLAIN,          // (lj_pairs + lrc_pair) + lrc_self
	CRYSTAL_SELF,   // ((lj_pairs + lrc_pair) + crystal_self) + lrc_self: rd_crystal, in lj()'s order
	NO_CORRECTIONS  // lj_pairs: lj_buffered_14_7(), dreiding() and sg() have no long-range correction
};
void compose_totals(const mpmc_ctx *c, RdForm form, mpmc_result *r);
inline RdForm rd_form_of(const mpmc_ctx *c) { // by the terms switched on (the trial paths, contact_penalise)
	if (sg_on(c)) return RdForm::NO_CORRECTIONS;
	if (rd_model_on(c)) return c->kept.rdm_form == RD_FORM_LJ ? RdForm::PLAIN : RdForm::NO_CORRECTIONS;
	return crystal_on(c) ? RdForm::CRYSTAL_SELF : RdForm::PLAIN;
}
int crystal_ready(mpmc_ctx *c);    // the image table, cutoff, thresholds and crystal_self of the current cell and atoms are in place (context.cpp)
CrystalParams crystal_params(const mpmc_ctx *c); // rc_par with this evaluation's Feynman-Hibbs constants (evaluate.cpp)
Box lrc_box(const mpmc_ctx *c);    // the cell as the long-range corrections see it: rd_crystal puts its own cutoff in (evaluate.cpp)
int prepare(mpmc_ctx *c, bool defer_static = false); // uploads what is dirty, (re)builds the k tables; the position-independent terms unless deferred (evaluate.cpp)
// one evaluation (the pieces in `mask`) on the context's streams (evaluate.cpp: a plan, the room it needs, then the stages); on_demand: where
// the energy comes from the moments of the first half of the iterations, stop there and leave the rest to finish_pending_dipoles
// (volume_trial: the one caller that evaluates while a volume trial is open, the trial's own evaluation; every other is refused)
int enqueue(mpmc_ctx *c, unsigned mask, bool on_demand = false, bool volume_trial = false);
// waits for it and assembles the result into *out and c->eval (evaluate.cpp).  It FILLS: the accepted record and cache_valid are its
// callers' -- mpmc_energy_wait and the component entry points re-base (where run_mask == full_mask), the trial paths do not
int wait_and_fill(mpmc_ctx *c, mpmc_result *out);
inline void rebase_on_eval(mpmc_ctx *c) { c->accepted = c->eval, c->cache_valid = true; }
unsigned full_mask(const mpmc_ctx *c);           // what double System::energy() runs under the current options
// The polarization energy of a Jacobi solve with a fixed iteration count n and mu_0 = alpha E0 is -1/2 sum_k m_k over the moments of the
// first ceil(n/2) dipole differences: not for polar_gamma != 1, precision-terminated or rrms-reporting solves,
// Gauss-Seidel sweeps (the only place where `polar_palmo` acts) or the direct solve.
// `polar_gs_ranked` acts where thole_iterative sweeps (:3450-3543): polarization with polar_iterative on, not under zodid (:3470) and not
// under ewald_full, which has its own pass loop
inline bool gs_ranked_acts(const mpmc_ctx *c, const mpmc_options &o) {
	return c->kept.gs_ranked && o.polarization && !o.rd_only && o.polar_iterative && !c->kept.zodid && !c->kept.pef_enabled;
}
inline bool gs_ranked_on(const mpmc_ctx *c) { return gs_ranked_acts(c, c->opts); }
// Gauss-Seidel sweeps run in the reference's atom order (:3569), so the atoms then keep the caller's order on the device: under polar_gs
// (not under ewald_full, where it changes nothing) and wherever the ranked sweeps act.  Whoever changes one of the inputs compares the
// rule before and after and asks for a new upload when it moved (order_rule_changed).
inline bool sweeps_keep_atom_order(const mpmc_ctx *c, const mpmc_options &o) {
	return (o.polar_gs && o.polarization && !o.rd_only && !c->kept.pef_enabled) || gs_ranked_acts(c, o);
}
inline void order_rule_changed(mpmc_ctx *c, bool was) {
	if (c->opts_set && was != sweeps_keep_atom_order(c, c->opts)) c->atoms_dirty = c->atoms_dirty_order = true;
}
inline bool polar_moments_apply(const mpmc_ctx *c) {
	const mpmc_options &o = c->opts;
	if (gs_ranked_on(c)) return false; // (sweeps, like polar_gs below)
	if (c->kept.relax_scheme != 0 || c->kept.zodid) return false; // (relaxed iterations are no longer powers of one symmetric operator; zodid has none)
	if (c->kept.pef_enabled) return false; // (ewald_full is not the symmetric Jacobi iteration; the setting acts only where the line below holds anyway)
	return o.polarization && !o.rd_only && o.polar_iterative && o.polar_max_iter >= 1 && o.polar_max_iter <= kMomentsMaxIter && o.polar_gamma == 1.0 && o.polar_precision == 0.0 && !o.polar_rrms &&
	       !o.polar_gs; // (`polar_palmo` acts under Gauss-Seidel sweeps only: under Jacobi its correction is zero and nothing runs)
}
inline int moments_half(int n) { return (n + 1) / 2; } // iterations whose differences the moments of n iterations need
inline int reserve_dk_ring(mpmc_ctx *c) { return c->d_dk_ring.reserve(c, (size_t)(moments_half(c->opts.polar_max_iter) + 1) * 3 * (size_t)c->max_pad); }
// Every reader of the dipoles, the induced field or anything else the remaining iterations write calls this first: runs what an on-demand
// evaluation left undone and waits for it (nothing to do otherwise); MPMC_ERR_ARG when the open solve's inputs are gone (evaluate.cpp)
int finish_pending_dipoles(mpmc_ctx *c);
// `polar_ewald_full` acts with polarization on and rd_only off, and then replaces the whole dipole solve: System::polar() tries it first (:2558)
inline bool ewald_full_on(const mpmc_ctx *c) { return c->kept.pef_enabled && c->opts.polarization && !c->opts.rd_only; }
// the static field is the Ewald one: `polar_ewald on`, or ewald_full (recip_term + real_term whatever polar_ewald says, :2790-2793)
inline bool field_is_ewald(const mpmc_ctx *c) { return c->opts.polar_ewald || ewald_full_on(c); }
// whoever is about to overwrite positions, cell, options, tensor store or dipole vectors: the open solve can no longer be finished
inline void drop_pending_dipoles(mpmc_ctx *c) {
	if (c->polar_pending == mpmc_ctx::PEND_OPEN) c->polar_pending = mpmc_ctx::PEND_DROPPED;
}
inline bool direct_solve(const mpmc_ctx *c) { // `polar_iterative off` (ewald_full comes first, :2558-2563)
	return c->opts.polarization && !c->opts.rd_only && !c->opts.polar_iterative && !ewald_full_on(c);
}
// `polar_zodid` acts where thole_iterative runs (:3470): polarization with polar_iterative on, and not under ewald_full (System::polar :2558)
inline bool zodid_on(const mpmc_ctx *c) {
	return c->kept.zodid && c->opts.polarization && !c->opts.rd_only && c->opts.polar_iterative && !ewald_full_on(c);
}
// the factor on mu_0 = alpha E0: polar_gamma, unless a relaxation scheme is on (init_dipoles :3555) or the solve is ewald_full's (:2944-2956)
inline double start_gamma(const mpmc_ctx *c) { return (ewald_full_on(c) || c->kept.relax_scheme != 0) ? 1.0 : c->opts.polar_gamma; }
// `polar_wolf` replaces the static field whenever polar_ewald is off (thole_field :3289-3294: polar_ewald wins)
inline bool wolf_field_on(const mpmc_ctx *c) { return c->kept.pw_enabled && c->opts.polarization && !c->opts.rd_only && !field_is_ewald(c); }
void ext_params(const mpmc_ctx *c, FusedParams &fp, bool wolf_on); // Wolf / Feynman-Hibbs fields of the pair parameters (evaluate.cpp)
AtomsDev atoms_view(const mpmc_ctx *c);
RecipDev recip_view(const mpmc_ctx *c);
int upload_atoms(mpmc_ctx *c);                   // spatial order + device atom arrays (context.cpp)
// the Box of a cell: basis, reciprocal, volume, cutoff, the squared-distance thresholds of the cutoff predicates, ortho (context.cpp)
void box_from_cell(const double basis[9], const double R[9], double volume, double cutoff, Box &out);
void vol_abandon(mpmc_ctx *c); // an open volume trial is closed and the accepted device state put back in place (trial.cpp); nothing to do otherwise
// the AF_* word of one atom as upload_atoms packs it
inline int atom_flag_word(const mpmc_ctx *c, int frozen, double eps, double sigma, int disp, double q, double alpha) {
	int fl = 0;
	if (frozen) fl |= AF_FROZEN;
	if (eps == 0.0 || sigma == 0.0) fl |= AF_NULL_RD;
	if (disp) fl |= c->kept.de_enabled ? AF_DISP_RD : AF_HAS_DISP; // (disp-expansion: LJ mixing no longer matters, pair_math.h)
	if (sigma < 0.0) fl |= AF_NEG_SIGMA;
	if (sigma == 0.0) fl |= AF_ZERO_SIGMA;
	if (q == 0.0) fl |= AF_ZERO_Q;
	if (alpha == 0.0) fl |= AF_ZERO_ALPHA;
	return fl;
}
// exchange trials (context.cpp): the host list with atoms [at, at + n_remove) taken out and `ins` (may be null) put in their place, the
// spatial order carried, the tables that follow the tile count resized; everything else of the context stays (totals, structure factors)
int splice_atoms(mpmc_ctx *c, int at, int n_remove, const AtomRun *ins);
void copy_atom_run(const mpmc_ctx *c, int first, int count, AtomRun &out); // out = atoms [first, first + count) of the host mirrors
int set_atoms_from(mpmc_ctx *c, const AtomRun &list);                     // mpmc_set_atoms with a whole list
// the host sums: of the current list / one atom added (sg = +1) or taken out (-1) / lrc_pair, lrc_self, es_self from them (k_atom_terms_finish)
void xch_sum_list(const mpmc_ctx *c, XchSums &out);
void xch_sum_atom(const mpmc_ctx *c, XchSums &xs, double sg, int fl, double sigma, double eps, double q);
void xch_static_terms(const mpmc_ctx *c, const XchSums &xs, double out3[3]);
// update_com + wrap_all over the host mirror (evaluate.cpp): centres of mass, lattice shifts, wrapped positions; any pointer may be null
void wrap_molecules(const mpmc_ctx *c, double *com, double *wrapped_com, double *wrapped_pos);

} // namespace mpmc
