// context.cpp -- host side of libmpmc_energy.so: the C ABI of include/mpmc_energy.h.
//
// One mpmc_ctx = the device-resident state of one reference `System` (one box / one PI bead):
// its own HIP stream, struct-of-arrays atom buffers, k-vector tables, work buffers and result scalars.
// Replaces, for the energy path only, the per-System pair lists (reference src/System.Pairs.cpp:21) and the
// A matrix (src/System.cpp:1430-1473).  There is no CPU fallback anywhere in this file.
#include "context.h"

using namespace mpmc;

thread_local std::string mpmc::g_create_error;

// ---- library --------------------------------------------------------------------------------------------
extern "C" int mpmc_abi_version(void) { return MPMC_ABI_VERSION; }

extern "C" int mpmc_device_count(int *count) {
	int n = 0;
	hipError_t e = hipGetDeviceCount(&n);
	if (count) *count = (e == hipSuccess) ? n : 0;
	return (e == hipSuccess) ? MPMC_OK : MPMC_ERR_NO_DEVICE;
}

// (ABI 6) what a host program without its own HIP binding needs around the path: a fence over everything this process enqueued on a
// device (the timing bracket of a benchmark, the reference's MPI_Barrier companion) and the device's marketing name for its log
extern "C" int mpmc_device_synchronize(int device) {
	if (hipSetDevice(device) != hipSuccess) return MPMC_ERR_NO_DEVICE;
	return hipDeviceSynchronize() == hipSuccess ? MPMC_OK : MPMC_ERR_HIP;
}
extern "C" int mpmc_device_name(int device, char *name, int capacity) {
	if (!name || capacity < 1) return MPMC_ERR_ARG;
	name[0] = 0;
	hipDeviceProp_t prop;
	if (hipGetDeviceProperties(&prop, device) != hipSuccess) return MPMC_ERR_NO_DEVICE;
	std::snprintf(name, (size_t)capacity, "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
	return MPMC_OK;
}

extern "C" const char *mpmc_last_error(const mpmc_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

// PeriodicBoundary::update, reference src/PeriodicBoundary.cpp:31-101 (same association order)
extern "C" int mpmc_pbc_compute(const double b[9], double R[9], double *volume, double *cutoff) {
	if (!b || !R || !volume || !cutoff) return MPMC_ERR_ARG;
#define B(i, j) b[3 * (i) + (j)]
	double vol;
	vol = B(0, 0) * (B(1, 1) * B(2, 2) - B(1, 2) * B(2, 1));
	vol += B(0, 1) * (B(1, 2) * B(2, 0) - B(1, 0) * B(2, 2));
	vol += B(0, 2) * (B(1, 0) * B(2, 1) - B(1, 1) * B(2, 0));
	*volume = vol;
	if (vol <= 0) {
		*cutoff = kMaxValue;
	} else {
		double shortest = kMaxValue;
		for (int i = -15; i <= 15; i++)
			for (int j = -15; j <= 15; j++)
				for (int k = -15; k <= 15; k++) {
					if (!i && !j && !k) continue;
					double v[3];
					for (int p = 0; p < 3; p++) v[p] = i * B(0, p) + j * B(1, p) + k * B(2, p);
					double m = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
					if (m < shortest) shortest = m;
				}
		*cutoff = 0.5 * shortest;
	}
	const double iv = 1.0 / vol;
	R[0] = iv * (B(1, 1) * B(2, 2) - B(1, 2) * B(2, 1));
	R[1] = iv * (B(0, 2) * B(2, 1) - B(0, 1) * B(2, 2));
	R[2] = iv * (B(0, 1) * B(1, 2) - B(0, 2) * B(1, 1));
	R[3] = iv * (B(1, 2) * B(2, 0) - B(1, 0) * B(2, 2));
	R[4] = iv * (B(0, 0) * B(2, 2) - B(0, 2) * B(2, 0));
	R[5] = iv * (B(0, 2) * B(1, 0) - B(0, 0) * B(1, 2));
	R[6] = iv * (B(1, 0) * B(2, 1) - B(1, 1) * B(2, 0));
	R[7] = iv * (B(0, 1) * B(2, 0) - B(0, 0) * B(2, 1));
	R[8] = iv * (B(0, 0) * B(1, 1) - B(0, 1) * B(1, 0));
#undef B
	return (vol > 0) ? MPMC_OK : MPMC_ERR_BOX;
}

extern "C" void mpmc_default_options(mpmc_options *o) {
	if (!o) return;
	std::memset(o, 0, sizeof(*o));
	o->rd_lrc = 1;          // reference src/System.h: rd_lrc default on
	o->polar_max_iter = 10; // polar_max_iter default
	o->ewald_kmax = 7;      // ewald_kmax default
	o->polar_gamma = 1.0;
	o->damp_type = MPMC_DAMPING_EXPONENTIAL;
	o->solver = MPMC_SOLVER_AUTO;
}

// largest double t >= 0 with pred(t) true, for a predicate that is true below and false above some point near rc^2
template <typename Pred>
static double bisect_threshold(double rc, Pred pred) {
	double lo = rc * rc * (1.0 - 1e-6), hi = rc * rc * (1.0 + 1e-6) + 1e-300;
	if (!pred(lo) || pred(hi)) return pred(hi) ? hi : -1.0; // degenerate box; callers validated rc > 0
	uint64_t a, b;
	std::memcpy(&a, &lo, 8);
	std::memcpy(&b, &hi, 8);
	while (b - a > 1) { // positive doubles order like their bit patterns
		uint64_t m = a + (b - a) / 2;
		double x;
		std::memcpy(&x, &m, 8);
		if (pred(x)) a = m;
		else b = m;
	}
	double out;
	std::memcpy(&out, &a, 8);
	return out;
}

// per-device result of the lane-rotation self-test (0 unknown, 1 ok): every symmetric kernel rotates its j-side accumulators with
// v_mov_b32_dpp wave_rol:1; a device on which that does not deliver lane (l + 1) & 63 cannot run this library
static std::atomic<int> g_rot_ok[64];
static int rot_selftest(mpmc_ctx *c) {
	if (c->device < 64 && g_rot_ok[c->device].load(std::memory_order_acquire)) return MPMC_OK;
	DevBuf<int> d; // scratch
	int h[64], rc = d.reserve(c, 64);
	if (rc != MPMC_OK) return rc;
	rc = [&] {
		launch_rot_selftest(c->stream, d);
		HIP_TRY(c, hipGetLastError());
		HIP_TRY(c, hipMemcpyAsync(h, d, sizeof(h), hipMemcpyDeviceToHost, c->stream));
		HIP_TRY(c, hipStreamSynchronize(c->stream));
		return (int)MPMC_OK;
	}();
	d.release(c); // on every way out: the context's byte count never keeps the scratch
	if (rc != MPMC_OK) return rc;
	for (int l = 0; l < 64; l++)
		if (h[l] != ((l + 1) & 63)) {
			c->err = "lane-rotation self-test failed (v_mov_b32_dpp wave_rol:1): not a gfx950 device?";
			return MPMC_ERR_INTERNAL;
		}
	if (c->device < 64) g_rot_ok[c->device].store(1, std::memory_order_release);
	return MPMC_OK;
}

static mpmc_tuning g_tuning_default; // what contexts created from now on start from (mpmc_debug_configure with a null context)
static std::mutex g_tuning_mu;       // ... written by mpmc_debug_configure(NULL, ...) and copied by mpmc_ctx_create on any thread

// ---- lifetime --------------------------------------------------------------------------------------------
extern "C" int mpmc_ctx_create(int device, int max_atoms, mpmc_ctx **out) {
	if (!out || max_atoms <= 0) return fail(nullptr, MPMC_ERR_ARG, "mpmc_ctx_create: bad argument");
	*out = nullptr;
	int ndev = 0;
	hipError_t e = hipGetDeviceCount(&ndev);
	if (e != hipSuccess || ndev <= 0)
		return fail(nullptr, MPMC_ERR_NO_DEVICE,
		            std::string("mpmc_ctx_create: no HIP device (") + hipGetErrorString(e) + "); this library has no CPU path");
	if (device < 0 || device >= ndev) return fail(nullptr, MPMC_ERR_ARG, "mpmc_ctx_create: device index out of range");
	if (hipSetDevice(device) != hipSuccess) return fail(nullptr, MPMC_ERR_NO_DEVICE, "mpmc_ctx_create: hipSetDevice failed");

	mpmc_ctx *c = new mpmc_ctx();
	c->device = device;
	c->max_atoms = max_atoms;
	c->max_pad = ((max_atoms + kTile - 1) / kTile) * kTile;
	mpmc_default_options(&c->opts);
	int rc = MPMC_OK;
	auto A = [&](int r) { if (rc == MPMC_OK) rc = r; };
	{
		std::lock_guard<std::mutex> lk(g_tuning_mu);
		c->kept.tune = g_tuning_default;
	}
	if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
	    (!c->kept.tune.lazy_side_stream && hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking) != hipSuccess) ||
	    hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess ||
	    hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess) {
		delete c;
		return fail(nullptr, MPMC_ERR_HIP, "mpmc_ctx_create: hipStreamCreate failed");
	}
	c->two_streams = (c->kept.tune.stream_mode != 0);
	const size_t P = (size_t)c->max_pad;
	A(c->d_atoms_blob.reserve(c, P * kAtomRecordBytes)); // every per-atom array, one block (layout: atom_block_layout)
	if (rc == MPMC_OK)
		atom_block_layout(c->d_atoms_blob, P, [c](double4 *xyzq, double2 *lj, int2 *mf, double *al, double *ep, double *imm, int32_t *perm, int32_t *slot) {
			c->d_xyzq = xyzq, c->d_lj = lj, c->d_mf = mf, c->d_alpha = al, c->d_eps = ep, c->d_inv_molmass = imm, c->d_perm = perm, c->d_slot_of = slot;
		});
	A(c->d_tile_bounds.reserve(c, 12 * (P / kTile)));
	A(c->d_scal.reserve(c, (size_t)S_COUNT + (size_t)C_COUNT)); // scalars and counts share one buffer: one clear, one read-back
	if (rc == MPMC_OK) c->d_cnt = reinterpret_cast<long long *>(c->d_scal + S_COUNT);
	A(c->d_flag.reserve(c, 4)); // [0]: Gauss-Seidel's per-sweep flag; [1..3]: iteration control of the precision-terminated Jacobi solve
	A(c->d_counter.reserve(c, 1));
	A(c->d_atom_part.reserve(c, kAtomTermScratch));
	A(c->d_erf_tab.reserve(c, kErfTableDouble2));
	if (rc == MPMC_OK) { // the erfc table of the pair sweep: 24 KB, once per context
		std::vector<double2> tab(kErfTableDouble2);
		erfc_table_device_layout(tab.data());
		if (hipMemcpyAsync(c->d_erf_tab, tab.data(), tab.size() * sizeof(double2), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
		    hipStreamSynchronize(c->stream) != hipSuccess)
			rc = MPMC_ERR_HIP;
	}
	static_assert(sizeof(long long) == sizeof(double), "scalars and counts share one buffer");
	A(c->h_scal.reserve(c, S_COUNT + C_COUNT + 1));
	if (rc == MPMC_OK) {
		c->h_cnt = reinterpret_cast<long long *>(c->h_scal + S_COUNT);
		std::memset(c->h_scal, 0, (S_COUNT + C_COUNT + 1) * sizeof(double)); // (the launch-number slot the waits poll starts at 0: a recycled pinned block may hold an old context's 1.0)
	}
	A(c->h_flag.reserve(c, 4));
	if (rc == MPMC_OK) rc = rot_selftest(c);
	if (rc != MPMC_OK) {
		g_create_error = "mpmc_ctx_create: device allocation failed: " + c->err;
		mpmc_ctx_destroy(c);
		return rc;
	}
	*out = c;
	return MPMC_OK;
}

extern "C" int mpmc_ctx_destroy(mpmc_ctx *c) {
	if (!c) return MPMC_ERR_ARG;
	(void)hipSetDevice(c->device);
	if (c->stream2) (void)hipStreamSynchronize(c->stream2);
	if (c->stream) (void)hipStreamSynchronize(c->stream);
	if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
	if (c->ev_join) (void)hipEventDestroy(c->ev_join);
	if (c->stream2) (void)hipStreamDestroy(c->stream2);
	for (auto &e : c->ev_used) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
	for (auto &e : c->ev_free) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
	if (c->ev_xyzq) (void)hipEventDestroy(c->ev_xyzq);
	if (c->ev_kstage) (void)hipEventDestroy(c->ev_kstage);
	if (c->ev_stage) (void)hipEventDestroy(c->ev_stage);
	for (hipEvent_t e : c->cav_ev)
		if (e) (void)hipEventDestroy(e);
	if (c->stream) (void)hipStreamDestroy(c->stream);
	// the buffers free themselves, behind the destruction of the streams: both were synchronised above, so nothing enqueued can still
	// touch the memory, and freeing needs no stream
	delete c;
	return MPMC_OK;
}

// ---- box / options ---------------------------------------------------------------------------------------
void mpmc::box_from_cell(const double basis[9], const double R[9], double vol, double cut, Box &out) {
	std::memcpy(out.b, basis, sizeof(out.b));
	std::memcpy(out.r, R, sizeof(out.r));
	out.volume = vol;
	out.cutoff = cut;
	// squared-distance forms of the reference's cutoff predicates (see pair_math.h Box)
	out.t_lj = bisect_threshold(cut, [cut](double t) { return std::sqrt(t) - kSmallDR < cut; });
	out.t_es = bisect_threshold(cut, [cut](double t) { return !(std::sqrt(t) > cut); });
	out.t_wolf = bisect_threshold(cut, [cut](double t) { return std::sqrt(t) < cut; });
	out.ortho = 1;
	for (int i = 0; i < 3; i++)
		for (int j = 0; j < 3; j++)
			if (i != j && (basis[3 * i + j] != 0.0 || R[3 * i + j] != 0.0)) out.ortho = 0;
}

extern "C" int mpmc_set_box(mpmc_ctx *c, const double basis[9], const double *reciprocal, double volume, double cutoff) {
	if (!c || !basis) return MPMC_ERR_ARG;
	// the same cell again (a caller that hands the box over before every evaluation): nothing to invalidate
	double in[20];
	std::memcpy(in, basis, 9 * sizeof(double));
	if (reciprocal) std::memcpy(in + 9, reciprocal, 9 * sizeof(double));
	else std::memset(in + 9, 0, 9 * sizeof(double));
	in[18] = volume;
	in[19] = cutoff;
	// (not while a volume trial is open: the call closes it, and the accepted totals go as with any other cell)
	const bool vol_open = c->trial.open && c->trial.volume;
	if (!vol_open && c->box_set && c->box_in_has_recip == (reciprocal != nullptr) && std::memcmp(in, c->box_in, sizeof(in)) == 0) return MPMC_OK;
	double R[9], vol = 0, cut = 0;
	int rc = mpmc_pbc_compute(basis, R, &vol, &cut);
	if (rc != MPMC_OK) return fail(c, MPMC_ERR_BOX, "mpmc_set_box: non-positive cell volume");
	if (reciprocal) std::memcpy(R, reciprocal, sizeof(R));
	if (volume > 0) vol = volume;
	if (cutoff > 0) cut = cutoff;
	if (!(vol > 0) || !(cut > 0)) return fail(c, MPMC_ERR_BOX, "mpmc_set_box: invalid volume / cutoff");
	vol_abandon(c);          // (an open volume trial belongs to the old cell too)
	drop_pending_dipoles(c); // (an open on-demand solve belongs to the old cell)
	box_from_cell(basis, R, vol, cut, c->box);
	c->box_set = true;
	std::memcpy(c->box_in, in, sizeof(in)); // (only a call that was accepted is remembered)
	c->box_in_has_recip = (reciprocal != nullptr);
	c->k_dirty = true;
	c->static_dirty = true;
	c->static_gen++;
	// (No re-sort, no upload of the atoms: the spatial order is a locality heuristic and a new cell leaves it as good as the positions
	// leave it -- a volume move scales both together; atoms that really wander are caught by the drift check of mpmc_update_positions.
	// The fractional origin of the last sort stays valid too: it only says where the tile bounds cut the periodic wrap.)
	c->cache_valid = false;
	return MPMC_OK;
}

extern "C" int mpmc_set_options(mpmc_ctx *c, const mpmc_options *o) {
	if (!c || !o) return MPMC_ERR_ARG;
	// (Wolf / Feynman-Hibbs travel in their own option fields, matrix inversion is polar_iterative == 0)
	if (o->unsupported_flags & ~(uint64_t)(MPMC_FLAG_WOLF | MPMC_FLAG_FEYNMAN_HIBBS | MPMC_FLAG_POLAR_MATRIX_INVERSION)) {
		char buf[160];
		std::snprintf(buf, sizeof buf, "mpmc_set_options: reference option(s) outside the energy hot path are ON (flag mask 0x%llx)",
		              (unsigned long long)o->unsupported_flags);
		return fail(c, MPMC_ERR_UNSUPPORTED, buf);
	}
	if (o->polarization && !o->rd_only) {
		if (o->damp_type != MPMC_DAMPING_EXPONENTIAL)
			return fail(c, MPMC_ERR_UNSUPPORTED, "mpmc_set_options: only polar_damp_type exponential is supported");
		if (o->polar_iterative && o->polar_precision == 0.0 && o->polar_max_iter < 1)
			return fail(c, MPMC_ERR_INVALID_SETTING, "mpmc_set_options: polar_max_iter must be >= 1 when polar_precision is 0 (the reference never terminates)");
		if (o->polar_iterative && o->polar_precision < 0.0) return fail(c, MPMC_ERR_INVALID_SETTING, "mpmc_set_options: polar_precision < 0");
		if (o->polar_iterative && (o->solver < MPMC_SOLVER_AUTO || o->solver > MPMC_SOLVER_DENSE)) return fail(c, MPMC_ERR_INVALID_SETTING, "mpmc_set_options: bad solver");
	}
	if (o->ewald_kmax < 0 || o->ewald_kmax > 64) return fail(c, MPMC_ERR_INVALID_SETTING, "mpmc_set_options: ewald_kmax out of range");
	if (o->feynman_hibbs) {
		if (!(o->temperature > 0)) return fail(c, MPMC_ERR_INVALID_SETTING, "mpmc_set_options: feynman_hibbs requires positive temperature"); // SimulationControl.cpp:2509
		if (o->wolf && !o->rd_only) return fail(c, MPMC_ERR_INCOMPATIBLE, "mpmc_set_options: FH + es_wolf is not implemented"); // System.Energy.cpp:1448-1450
	}
	// unchanged: keep the accepted configuration's totals (not while a volume trial is open: the call closes it, as with changed options)
	if (!(c->trial.open && c->trial.volume) && c->opts_set && std::memcmp(&c->opts_user, o, sizeof(mpmc_options)) == 0) return MPMC_OK;
	c->opts_user = *o;
	apply_options(c, effective_options(c, *o));
	return MPMC_OK;
}

// the options the evaluations read change (mpmc_set_options; mpmc_set_silvera_goldman, under which they differ from the caller's)
void mpmc::apply_options(mpmc_ctx *c, const mpmc_options &eff) {
	const mpmc_options *o = &eff;
	// Gauss-Seidel sweeps run in the reference's atom order (System.Energy.cpp:3569): whenever "this evaluation sweeps in atom order"
	// changes -- through polar_gs, polarization, rd_only or polar_iterative (the ranked sweeps), or on the first options after an upload
	// under the defaults -- re-upload (not under `polar_ewald_full`, where polar_gs changes nothing: the spatial order stays)
	if ((c->opts_set && sweeps_keep_atom_order(c, c->opts)) != sweeps_keep_atom_order(c, *o)) c->atoms_dirty = c->atoms_dirty_order = true;
	vol_abandon(c);
	drop_pending_dipoles(c); // (... and to the old options)
	c->opts = *o;
	c->opts_set = true;
	c->k_dirty = true;
	c->static_dirty = true;
	c->static_gen++;
	c->cache_valid = false;
}

// ---- atoms -----------------------------------------------------------------------------------------------
// nested bisection sort of the wrapped fractional coordinates: nx slabs in x, ny strips in y per slab, z order inside a
// strip; consecutive groups of 64 slots (tiles) are then roughly cubic cells.  Pure host code, O(N log N).
constexpr double kResortDrift = 2.0; // Angstrom; a tile is ~16 A wide at liquid density
constexpr int kSortGridMinTiles = 100; // the aligned-grid order from this many tiles on (about 6400 atoms)
static void compute_spatial_order(mpmc_ctx *c) {
	const int n = c->n;
	c->perm.resize(n);
	c->slot_of.resize(n);
	for (int i = 0; i < n; i++) c->perm[i] = i;
	bool enable = c->box_set && n > 2 * kTile;
	if (c->opts_set && sweeps_keep_atom_order(c, c->opts)) enable = false; // the sweep order IS the atom order (:3569)
	if (c->kept.tune.no_sort) enable = false;
	if (enable) {
		// fractional coordinates counted from the smallest one in each dimension: with all atoms inside one period (the usual case) the
		// periodic wrap is cut at the edge of the occupied range, so tiles are compact in the RAW coordinates too -- which is what lets
		// whole tile pairs share one periodic image index (k_classify)
		std::vector<double> f(3 * (size_t)n);
		double org[3] = {1e300, 1e300, 1e300};
		for (int i = 0; i < n; i++)
			for (int p = 0; p < 3; p++) {
				double v = 0;
				for (int q = 0; q < 3; q++) v += c->box.r[3 * q + p] * c->h_pos[3 * i + q];
				f[3 * (size_t)i + p] = v;
				if (v < org[p]) org[p] = v;
			}
		for (int p = 0; p < 3; p++) c->sort_origin_f[p] = org[p];
		for (int i = 0; i < n; i++)
			for (int p = 0; p < 3; p++) {
				double v = f[3 * (size_t)i + p] - org[p];
				v -= std::floor(v);
				f[3 * (size_t)i + p] = v;
			}
		// The aligned grid (round 4).  A dimension costs the Jacobi walk and the pair sweep three instructions per pair when the tile pair has
		// no common periodic image in it, i.e. when tile A's interval meets the half-period image of tile B's.  With count-based boundaries
		// (the nested bisection below) that happens for a fraction (len_A + len_B) / L of the tile pairs -- 1.38 dimensions per far pair at the
		// benchmark box.  Slabs and strips on a FIXED grid of the fractional coordinates with an EVEN number of cells per dimension map onto
		// themselves under a shift by half a period, so an interval meets the image of exactly one other: 0.99 dimensions per far pair, -2.0 %
		// instructions in the contraction, -3.7 % in the sweep, +1.4 % evaluations/s with 32 beads in flight (profiles/r04_sort_grid.txt).
		// The columns are walked in serpentine order, z up one and down the next, so that a tile that runs over the end of a column
		// continues in the neighbouring one at the same z edge and stays compact.  Cells per dimension: 2 ceil(|b_d| / 2e) for the edge e of a
		// cube of one tile's volume; used when every column holds at least two tiles (below that the bisection's cubes are better).
		int grid_x = c->kept.tune.sort_nx, grid_y = c->kept.tune.sort_ny;
		if ((grid_x <= 0 || grid_y <= 0) && c->kept.tune.sort_grid != 0) {
			const int T = (n + kTile - 1) / kTile;
			const double e = std::cbrt(std::fabs(c->box.volume) * (double)kTile / (double)n);
			double len[2];
			for (int p = 0; p < 2; p++) len[p] = std::sqrt(c->box.b[3 * p] * c->box.b[3 * p] + c->box.b[3 * p + 1] * c->box.b[3 * p + 1] + c->box.b[3 * p + 2] * c->box.b[3 * p + 2]);
			const int ax = 2 * std::max(1, (int)std::ceil(len[0] / (2.0 * e))), ay = 2 * std::max(1, (int)std::ceil(len[1] / (2.0 * e)));
			// (measured over sizes, profiles/r04_sort_grid.txt: +1.4 to +1.7 % evaluations/s in flight at 7000 and 10 000 atoms, +1 % at 20 000, but -4 % at
			// 4000 atoms, where four cells per dimension leave the bisection's tiles aligned already: from kSortGridMinTiles tiles on)
			if (e > 0.0 && T >= kSortGridMinTiles && (long long)ax * ay * 2 <= T) grid_x = ax, grid_y = ay;
		}
		if (grid_x > 0 && grid_y > 0) {
			const int gx = grid_x, gy = grid_y;
			std::vector<long long> key((size_t)n);
			std::vector<double> zk((size_t)n);
			for (int i = 0; i < n; i++) {
				int sx = std::min(gx - 1, (int)(f[3 * (size_t)i] * gx)), sy = std::min(gy - 1, (int)(f[3 * (size_t)i + 1] * gy));
				if (sx & 1) sy = gy - 1 - sy;
				const long long col = (long long)sx * gy + sy;
				key[i] = col;
				zk[i] = (col & 1) ? -f[3 * (size_t)i + 2] : f[3 * (size_t)i + 2];
			}
			std::sort(c->perm.begin(), c->perm.end(), [&](int a, int b) {
				if (key[a] != key[b]) return key[a] < key[b];
				if (zk[a] != zk[b]) return zk[a] < zk[b];
				return a < b;
			});
			for (int k = 0; k < n; k++) c->slot_of[c->perm[k]] = k;
			c->order_sorted = true;
			c->edits_since_sort = 0;
			return;
		}
		const int T = (n + kTile - 1) / kTile;
		const int nx = std::max(1, (int)std::lround(std::cbrt((double)T)));
		const int tiles_per_slab = (T + nx - 1) / nx;
		const int ny = std::max(1, (int)std::lround(std::sqrt((double)tiles_per_slab)));
		const int tiles_per_strip = (tiles_per_slab + ny - 1) / ny;
		auto by = [&](int dim) { return [&f, dim](int a, int b) { return f[3 * (size_t)a + dim] < f[3 * (size_t)b + dim] || (f[3 * (size_t)a + dim] == f[3 * (size_t)b + dim] && a < b); }; };
		std::sort(c->perm.begin(), c->perm.end(), by(0));
		const int slab = tiles_per_slab * kTile, strip = tiles_per_strip * kTile;
		for (int s0 = 0; s0 < n; s0 += slab) {
			const int s1 = std::min(n, s0 + slab);
			std::sort(c->perm.begin() + s0, c->perm.begin() + s1, by(1));
			for (int t0 = s0; t0 < s1; t0 += strip) {
				const int t1 = std::min(s1, t0 + strip);
				std::sort(c->perm.begin() + t0, c->perm.begin() + t1, by(2));
			}
		}
	}
	for (int k = 0; k < n; k++) c->slot_of[c->perm[k]] = k;
	c->order_sorted = enable;
	c->edits_since_sort = 0;
}

// set_atoms with a list that differs from the one before by ONE contiguous run of atoms (inserted or removed): positions before the run
// and behind it are bitwise those of the old list.  Brings perm / slot_of up to date without sorting; false = not such an edit.
static bool carry_spatial_order(mpmc_ctx *c, const double *new_pos, int n_new) {
	const int n_old = (int)c->perm.size();
	if (!c->order_sorted || c->atoms_dirty_order || n_old == 0 || (int)c->h_pos.size() != 3 * n_old) return false;
	if (n_new <= 2 * kTile || n_new == n_old) return false; // (small systems keep the identity order; same size = not an insertion / removal)
	const int diff = n_new - n_old, m = diff > 0 ? diff : -diff, lo = std::min(n_old, n_new);
	if (m > kTile || c->edits_since_sort + m > kTile) return false; // time for a real sort
	const double *old_pos = c->h_pos.data();
	int p = 0;
	while (p < lo && old_pos[3 * p] == new_pos[3 * p] && old_pos[3 * p + 1] == new_pos[3 * p + 1] && old_pos[3 * p + 2] == new_pos[3 * p + 2]) p++;
	int s = 0;
	while (s < lo - p && old_pos[3 * (n_old - 1 - s)] == new_pos[3 * (n_new - 1 - s)] && old_pos[3 * (n_old - 1 - s) + 1] == new_pos[3 * (n_new - 1 - s) + 1] &&
	       old_pos[3 * (n_old - 1 - s) + 2] == new_pos[3 * (n_new - 1 - s) + 2])
		s++;
	if (p + s != lo) return false; // more than one run changed (or atoms moved as well): sort
	std::vector<int32_t> np_;
	np_.reserve(n_new);
	for (int k = 0; k < n_old; k++) {
		const int i = c->perm[k];
		if (i < p) np_.push_back(i);
		else if (i >= n_old - s) np_.push_back(i + diff);
		// else: removed
	}
	for (int i = p; i < n_new - s; i++) np_.push_back(i); // inserted atoms: appended (the last tile loses some locality until the next sort)
	if ((int)np_.size() != n_new) return false;
	c->perm.swap(np_);
	c->slot_of.assign(n_new, -1);
	for (int k = 0; k < n_new; k++) c->slot_of[c->perm[k]] = k;
	c->edits_since_sort += m;
	return true;
}

int mpmc::upload_atoms(mpmc_ctx *c) {
	// (atoms_dirty_order: somebody asked for a NEW order since the list was carried -- a set_options that switches Gauss-Seidel sweeps on
	// needs the identity order of System.Energy.cpp:3569, not the carried spatial one)
	if (!c->order_carried || c->atoms_dirty_order || c->kept.tune.no_order_carry || (int)c->perm.size() != c->n) {
		compute_spatial_order(c);
		c->kept.n_uploads_sorted++;
	} else {
		c->kept.n_uploads_carried++;
	}
	c->order_carried = false;
	c->atoms_dirty_order = false;
	const int n = c->n, np = c->n_pad;
	// One persistent pinned staging block for all per-atom arrays: the copies below are asynchronous for real (from pageable vectors
	// every one of them was a staged, blocking copy, and a stream synchronisation kept the vectors alive) -- an insertion or removal
	// (uVT, Gibbs) pays for a sort and eight enqueues here, nothing else.
	const size_t P = (size_t)c->max_pad;
	if (!c->static_cnt) {
		int rc;
		if ((rc = c->h_stage.reserve(c, P * kAtomRecordBytes)) != MPMC_OK) return rc;
		if ((rc = c->h_xyzq.reserve(c, P)) != MPMC_OK) return rc;
		if (!c->ev_xyzq) HIP_TRY(c, hipEventCreateWithFlags(&c->ev_xyzq, hipEventDisableTiming));
		if (!c->ev_stage) HIP_TRY(c, hipEventCreateWithFlags(&c->ev_stage, hipEventDisableTiming));
		if ((rc = c->static_cnt.reserve(c, 4)) != MPMC_OK) return rc;
		for (int k = 0; k < 4; k++) c->static_cnt[k] = 0;
	}
	if (c->stage_in_flight) { // (an upload per evaluation at most, and evaluations are waited for: normally long done)
		HIP_TRY(c, hipEventSynchronize(c->ev_stage));
		c->stage_in_flight = false;
	}
	double4 *xyzq = nullptr;
	double2 *lj = nullptr;
	int2 *mf = nullptr;
	double *al = nullptr, *ep = nullptr, *imm = nullptr;
	int32_t *perm = nullptr, *slot = nullptr;
	atom_block_layout(c->h_stage, P, [&](double4 *a0, double2 *a1, int2 *a2, double *a3, double *a4, double *a5, int32_t *a6, int32_t *a7) {
		xyzq = a0, lj = a1, mf = a2, al = a3, ep = a4, imm = a5, perm = a6, slot = a7;
	});
	c->molmass_tmp.assign(n, 0.0); // Molecule::mass = sum of its atoms' masses (System.cpp:687), per atom
	std::vector<double> &molmass = c->molmass_tmp;
	if (!c->h_mass.empty())
		for (int i0 = 0; i0 < n;) {
			int i1 = i0;
			double m = 0;
			while (i1 < n && c->h_mol[i1] == c->h_mol[i0]) m += c->h_mass[i1++];
			for (int i = i0; i < i1; i++) molmass[i] = m;
			i0 = i1;
		}
	for (int k = 0; k < np; k++) slot[k] = -1;
	for (int k = 0; k < np; k++) {
		if (k < n) {
			const int i = c->perm[k];
			perm[k] = i;
			slot[i] = k;
			xyzq[k] = make_double4(c->h_pos[3 * i], c->h_pos[3 * i + 1], c->h_pos[3 * i + 2], c->h_q[i]);
			lj[k] = make_double2(std::fabs(c->h_sigma[i]), std::sqrt(c->h_eps[i]));
			const int fl = atom_flag_word(c, c->h_frozen[i], c->h_eps[i], c->h_sigma[i], c->h_disp[i], c->h_q[i], c->h_alpha[i]);
			mf[k] = make_int2(c->h_mol[i], fl);
			al[k] = c->h_alpha[i];
			ep[k] = c->h_eps[i];
			imm[k] = (molmass[i] > 0.0) ? 1.0 / molmass[i] : 0.0;
		} else {
			perm[k] = -1;
			al[k] = ep[k] = imm[k] = 0.0;
			xyzq[k] = make_double4(0, 0, 0, 0);
			lj[k] = make_double2(0, 0);
			mf[k] = make_int2(-1 - k, AF_PAD | AF_FROZEN | AF_NULL_RD | AF_ZERO_SIGMA | AF_ZERO_Q | AF_ZERO_ALPHA);
		}
	}
	{ // tile pairs with an atom whose flags change lj_mix (sigma < 0, dispersion coefficients) are the generic pair kernel's (the sweep masks
	  // everything else itself): their list, in tile-pair order
		constexpr int kSpecial = kAtomFlagsMixing; // (pair_math.h: the same constant the sweep skips tile pairs by)
		const int nt = c->n_tiles;
		std::vector<char> special((size_t)nt, 0);
		bool any = false;
		for (int k = 0; k < n; k++)
			if (mf[k].y & kSpecial) special[k / kTile] = 1, any = true;
		c->h_generic.clear();
		if (any)
			for (int I = 0, t = 0; I < nt; I++)
				for (int J = I; J < nt; J++, t++)
					if (special[I] || special[J]) c->h_generic.push_back(t);
		c->n_generic = (int)c->h_generic.size();
		if (c->n_generic > 0) {
			// (room for every tile pair at once: the list changes with every upload, and no later one can then outgrow it)
			const int rc_a = c->d_generic_list.reserve(c, (size_t)c->n_generic, (size_t)c->n_tile_pairs);
			if (rc_a != MPMC_OK) return rc_a;
			HIP_TRY(c, hipMemcpyAsync(c->d_generic_list, c->h_generic.data(), (size_t)c->n_generic * sizeof(int), hipMemcpyHostToDevice, c->stream));
			HIP_TRY(c, hipStreamSynchronize(c->stream)); // pageable source that the next upload clears: wait, as the tile-pair and block tables do
		}
	}
	// ONE copy: the device block has the layout of the staging block (the tails beyond n_pad travel along; nobody reads them)
	if (np < (int)P && (size_t)np * 2 >= P)
		for (size_t k = (size_t)np; k < P; k++) { // (the tails travel along with the single copy: defined values)
			xyzq[k] = make_double4(0, 0, 0, 0);
			lj[k] = make_double2(0, 0);
			mf[k] = make_int2(-1 - (int)k, AF_PAD | AF_FROZEN | AF_NULL_RD | AF_ZERO_SIGMA | AF_ZERO_Q | AF_ZERO_ALPHA);
			al[k] = ep[k] = imm[k] = 0.0;
			perm[k] = slot[k] = -1;
		}
	if ((size_t)np * 2 >= P) {
		HIP_TRY(c, hipMemcpyAsync(c->d_atoms_blob, c->h_stage, P * kAtomRecordBytes, hipMemcpyHostToDevice, c->stream));
	} else { // a context created with much more room than atoms: the used prefix of every array instead of the whole block
		HIP_TRY(c, hipMemcpyAsync(c->d_xyzq, xyzq, np * sizeof(double4), hipMemcpyHostToDevice, c->stream));
		HIP_TRY(c, hipMemcpyAsync(c->d_lj, lj, np * sizeof(double2), hipMemcpyHostToDevice, c->stream));
		HIP_TRY(c, hipMemcpyAsync(c->d_mf, mf, np * sizeof(int2), hipMemcpyHostToDevice, c->stream));
		HIP_TRY(c, hipMemcpyAsync(c->d_alpha, al, np * sizeof(double), hipMemcpyHostToDevice, c->stream));
		HIP_TRY(c, hipMemcpyAsync(c->d_eps, ep, np * sizeof(double), hipMemcpyHostToDevice, c->stream));
		HIP_TRY(c, hipMemcpyAsync(c->d_inv_molmass, imm, np * sizeof(double), hipMemcpyHostToDevice, c->stream));
		HIP_TRY(c, hipMemcpyAsync(c->d_perm, perm, np * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
		HIP_TRY(c, hipMemcpyAsync(c->d_slot_of, slot, np * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
	}
	HIP_TRY(c, hipEventRecord(c->ev_stage, c->stream));
	c->stage_in_flight = true;
	// position-independent pair-flag counts (diagnostics of pair_exclusions), once per upload; they arrive in pinned memory in front of
	// the evaluation that follows on this stream, and are read when that evaluation has been waited for
	{
		launch_static_counts(c->stream, atoms_view(c), c->d_tile_pairs, c->n_tile_pairs, c->d_block_cnt, c->d_cnt);
		c->scal_clean = false; // (d_cnt is part of the scalar block: the next evaluation clears it instead of trusting which kernel overwrites what)
		HIP_TRY(c, hipGetLastError());
		HIP_TRY(c, hipMemcpyAsync(c->static_cnt, c->d_cnt, 4 * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
	}
	{ // slot-ordered mirror for later position updates
		const int rc_g = mirror_guard(c);
		if (rc_g != MPMC_OK) return rc_g;
		std::memcpy(c->h_xyzq, xyzq, (size_t)np * sizeof(double4));
	}
	c->h_pos_sorted = c->h_pos;        // where every atom stood when this order was made
	c->atoms_dirty = false;
	if (c->tb_have) c->tb_dirty = true; // (the three-body coefficients follow the order at the next evaluation that needs them)
	if (c->de_have) c->de_dirty = true; // (so do the disp-expansion coefficients)
	c->rdm_dirty = true;                // (and the rd model's per-atom table)
	c->ca_dirty = true;                 // (and what cavity_autoreject takes from the list)
	c->sg_frozen_atoms = -1;            // (and the Silvera-Goldman term's count of frozen atoms)
	return MPMC_OK;
}

// A context that has to hold more atoms than it was created for is rebuilt in place: a fresh context of the larger capacity takes
// over the caller's handle (same device, box, options, profiling state), the old device buffers are released.  Everything sized by
// the capacity is allocated on first use, so nothing else has to know.
static int grow_capacity(mpmc_ctx *c, int n) {
	(void)hipSetDevice(c->device);
	if (c->stream2) (void)hipStreamSynchronize(c->stream2);
	(void)hipStreamSynchronize(c->stream);
	mpmc_ctx *f = nullptr;
	const int cap = n + n / 4 + kTile;
	int rc = mpmc_ctx_create(c->device, cap, &f);
	if (rc != MPMC_OK) return fail(c, rc, "mpmc_set_atoms: cannot grow the context to " + std::to_string(cap) + " atoms: " + g_create_error);
	// (the cell as the caller gave it, box_in: a basis alone stays a basis alone, which a volume trial can scale; handing over the derived
	// reciprocal, volume and cutoff made every volume trial behind a growth "a caller-supplied override".  The derived values are the same bits.)
	if (c->box_set) rc = mpmc_set_box(f, c->box_in, c->box_in_has_recip ? c->box_in + 9 : nullptr, c->box_in[18], c->box_in[19]);
	if (rc == MPMC_OK && c->opts_set) rc = mpmc_set_options(f, &c->opts_user);
	if (rc != MPMC_OK) {
		c->err = "mpmc_set_atoms: growing the context failed: " + f->err;
		mpmc_ctx_destroy(f);
		return rc;
	}
	f->kept = c->kept; // (the switched-on terms survive, their coefficients go with the atom list that is being replaced; the new context sorts)
	if (f->opts_set && sg_on(f)) apply_options(f, effective_options(f, f->opts_user)); // (the Silvera-Goldman term reads its own view of the options)
	std::swap(*c, *f);
	mpmc_ctx_destroy(f); // now owns the old, smaller buffers
	return MPMC_OK;
}

// what follows the tile count of the current atom list: the upper-triangular tile-pair schedule, the work table of the fast sweep, the
// j-range split of the row kernels
static int size_tile_tables(mpmc_ctx *c) {
	int rc = MPMC_OK;
	// upper-triangular tile-pair schedule of the pair kernel
	const int nt = c->n_tiles;
	const size_t ntp = (size_t)nt * (nt + 1) / 2;
	if ((rc = c->d_tile_pairs.reserve(c, ntp)) != MPMC_OK) return rc;
	if ((rc = c->d_block_part.reserve(c, 2 * ntp)) != MPMC_OK) return rc;
	if ((rc = c->d_block_cnt.reserve(c, 4 * ntp)) != MPMC_OK) return rc;
	if ((rc = c->d_cls.reserve(c, ntp)) != MPMC_OK) return rc;
	if ((rc = c->d_tp_shift.reserve(c, ntp)) != MPMC_OK) return rc;
	std::vector<int2> tp;
	tp.reserve(ntp);
	for (int I = 0; I < nt; I++)
		for (int J = I; J < nt; J++) tp.push_back(make_int2(I, J));
	HIP_TRY(c, hipMemcpyAsync(c->d_tile_pairs, tp.data(), ntp * sizeof(int2), hipMemcpyHostToDevice, c->stream));
	HIP_TRY(c, hipStreamSynchronize(c->stream)); // `tp` dies with this function
	c->n_tile_pairs = (int)ntp;

	if (c->sweep_tiles != nt) { // work table of the fast pair sweep: a function of the tile count
		const int nb = pair_sweep_blocks(nt, nullptr);
		std::vector<int2> blocks((size_t)nb);
		pair_sweep_blocks(nt, blocks.data());
		if (c->kept.tune.sweep_order == 1) std::reverse(blocks.begin(), blocks.end()); // j-tiles descending (measurement)
		if ((rc = c->d_sweep_blocks.reserve(c, (size_t)nb)) != MPMC_OK) return rc;
		HIP_TRY(c, hipMemcpyAsync(c->d_sweep_blocks, blocks.data(), (size_t)nb * sizeof(int2), hipMemcpyHostToDevice, c->stream));
		HIP_TRY(c, hipStreamSynchronize(c->stream)); // `blocks` dies here
		c->n_sweep_blocks = nb;
		c->sweep_tiles = nt;
	}

	// j-range split of the per-atom (row) kernels: aim for >= ~4096 one-wave blocks
	c->n_split = std::max(1, std::min(nt, (4096 + nt - 1) / nt));
	return MPMC_OK;
}

extern "C" int mpmc_set_atoms(mpmc_ctx *c, int n, const double *pos, const double *charge, const double *polarizability, const double *epsilon,
                              const double *sigma, const int32_t *mol_id, const int32_t *frozen, const int32_t *has_disp, const double *mass) {
	if (!c || n <= 0 || !pos || !charge || !polarizability || !epsilon || !sigma || !mol_id || !frozen) return MPMC_ERR_ARG;
	vol_abandon(c); // (an open volume trial: the accepted device state goes back in place before the list is replaced)
	const bool solve_open = c->polar_pending != mpmc_ctx::PEND_NONE;
	if (n > c->max_atoms) { // insertions (uVT / Gibbs callers) outgrew the capacity hint given at creation
		const int rc_grow = grow_capacity(c, n);
		if (rc_grow != MPMC_OK) return rc_grow;
	}
	if (solve_open) c->polar_pending = mpmc_ctx::PEND_DROPPED; // (an open on-demand solve belongs to the old atom list, and to the old buffers)
	for (int i = 0; i < n; i++) {
		if (!std::isfinite(pos[3 * i]) || !std::isfinite(pos[3 * i + 1]) || !std::isfinite(pos[3 * i + 2]))
			return fail(c, MPMC_ERR_INVALID_DATUM, "mpmc_set_atoms: non-finite position");
		if (epsilon[i] < 0.0 || !std::isfinite(epsilon[i]) || !std::isfinite(sigma[i]) || !std::isfinite(charge[i]) || !std::isfinite(polarizability[i]))
			return fail(c, MPMC_ERR_INVALID_DATUM, "mpmc_set_atoms: epsilon < 0 or non-finite atom parameter");
	}
	{ // molecules are contiguous runs of the atom list (reference System.cpp:672): an id may not reappear later
		std::vector<int32_t> firsts;
		for (int i = 0; i < n; i++)
			if (i == 0 || mol_id[i] != mol_id[i - 1]) firsts.push_back(mol_id[i]);
		std::vector<int32_t> sorted = firsts;
		std::sort(sorted.begin(), sorted.end());
		if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
			return fail(c, MPMC_ERR_INVALID_DATUM, "mpmc_set_atoms: atoms of one molecule (equal mol_id) must be contiguous");
	}
	HIP_TRY(c, hipSetDevice(c->device));
	c->n = n;
	c->n_pad = ((n + kTile - 1) / kTile) * kTile;
	c->n_tiles = c->n_pad / kTile;
	// (before the old positions go: is this the list of before with one run of atoms inserted or removed?  Then the spatial order is carried)
	c->order_carried = carry_spatial_order(c, pos, n);
	c->h_pos.assign(pos, pos + 3 * (size_t)n);
	c->pos_gen++;
	c->list_gen++;
	c->h_q.assign(charge, charge + n);
	c->h_alpha.assign(polarizability, polarizability + n);
	c->h_eps.assign(epsilon, epsilon + n);
	c->h_sigma.assign(sigma, sigma + n);
	c->h_mol.assign(mol_id, mol_id + n);
	c->h_frozen.assign(frozen, frozen + n);
	if (has_disp) c->h_disp.assign(has_disp, has_disp + n);
	else c->h_disp.assign(n, 0);
	if (mass) c->h_mass.assign(mass, mass + n);
	else c->h_mass.clear();

	// countN (reference src/System.cpp:909-931): molecules that are not frozen.  A molecule's flag is the
	// flag of its last atom row (the PQR reader overwrites molecule->frozen per atom, src/System.cpp:687).
	c->n_molecules = 0;
	c->N_movable = 0;
	for (int i = 0; i < n; i++) {
		const bool last_of_mol = (i == n - 1) || (mol_id[i + 1] != mol_id[i]);
		if (last_of_mol) {
			c->n_molecules++;
			if (!frozen[i]) c->N_movable += 1.0;
		}
	}

	int rc = MPMC_OK;
	c->atoms_dirty = true; // uploaded (in spatial order) by the next evaluation, when the box is known too
	c->static_dirty = true;
	c->static_gen++;

	if ((rc = size_tile_tables(c)) != MPMC_OK) return rc;
	c->atoms_set = true;
	c->pending = false;
	c->cache_valid = false;
	c->trial.open = false;
	c->tb_have = false; // per-atom three-body coefficients belong to the old list (mpmc_set_axilrod_teller again)
	c->tb_dirty = false;
	c->h_tb_au.clear();
	c->de_have = c->de_dirty = c->de_lrc_valid = false; // so do the disp-expansion coefficients (mpmc_set_disp_expansion again)
	c->h_de.clear();
	c->h_de_raw.clear();
	return MPMC_OK;
}

// ---- exchange trials: editing the atom list in place, and the position-independent terms on the host ---------------------------------------
void mpmc::copy_atom_run(const mpmc_ctx *c, int first, int count, AtomRun &out) {
	const size_t a = (size_t)first, b = (size_t)first + (size_t)count;
	out.pos.assign(c->h_pos.begin() + 3 * a, c->h_pos.begin() + 3 * b);
	out.q.assign(c->h_q.begin() + a, c->h_q.begin() + b);
	out.alpha.assign(c->h_alpha.begin() + a, c->h_alpha.begin() + b);
	out.eps.assign(c->h_eps.begin() + a, c->h_eps.begin() + b);
	out.sigma.assign(c->h_sigma.begin() + a, c->h_sigma.begin() + b);
	out.mol.assign(c->h_mol.begin() + a, c->h_mol.begin() + b);
	out.frozen.assign(c->h_frozen.begin() + a, c->h_frozen.begin() + b);
	out.disp.assign(c->h_disp.begin() + a, c->h_disp.begin() + b);
	if (c->h_mass.empty()) out.mass.clear();
	else out.mass.assign(c->h_mass.begin() + a, c->h_mass.begin() + b);
}

int mpmc::set_atoms_from(mpmc_ctx *c, const AtomRun &l) {
	return mpmc_set_atoms(c, l.size(), l.pos.data(), l.q.data(), l.alpha.data(), l.eps.data(), l.sigma.data(), l.mol.data(), l.frozen.data(), l.disp.data(),
	                      l.mass.empty() ? nullptr : l.mass.data());
}

template <class T>
static void splice_vec(std::vector<T> &v, size_t at, size_t n_remove, const std::vector<T> *ins, size_t per = 1) {
	v.erase(v.begin() + per * at, v.begin() + per * (at + n_remove));
	if (ins) v.insert(v.begin() + per * at, ins->begin(), ins->end());
}

// The accepted exchange of the delta path.  The caller has checked the range and the capacity (n_new <= max_atoms).  Nothing on the device
// is touched here: the next evaluation or trial uploads the list (atoms_dirty) in the carried order, as after mpmc_set_atoms -- but the
// accepted totals, the structure factors and the position-independent terms stay the caller's.
int mpmc::splice_atoms(mpmc_ctx *c, int at, int n_remove, const AtomRun *ins) {
	const int n_ins = ins ? ins->size() : 0, n_new = c->n - n_remove + n_ins;
	if (at < 0 || n_remove < 0 || at + n_remove > c->n || n_new <= 0 || n_new > c->max_atoms) return fail(c, MPMC_ERR_ARG, "exchange trial: bad splice of the atom list");
	if (ins && !c->h_mass.empty() && ins->mass.empty()) return fail(c, MPMC_ERR_INVALID_DATUM, "exchange trial: the atom list has masses, the inserted molecule has none");
	std::vector<double> np_(c->h_pos);
	splice_vec(np_, (size_t)at, (size_t)n_remove, ins ? &ins->pos : nullptr, 3);
	c->order_carried = carry_spatial_order(c, np_.data(), n_new); // (before the old positions go)
	c->h_pos.swap(np_);
	c->pos_gen++;
	c->list_gen++;
	splice_vec(c->h_q, (size_t)at, (size_t)n_remove, ins ? &ins->q : nullptr);
	splice_vec(c->h_alpha, (size_t)at, (size_t)n_remove, ins ? &ins->alpha : nullptr);
	splice_vec(c->h_eps, (size_t)at, (size_t)n_remove, ins ? &ins->eps : nullptr);
	splice_vec(c->h_sigma, (size_t)at, (size_t)n_remove, ins ? &ins->sigma : nullptr);
	splice_vec(c->h_mol, (size_t)at, (size_t)n_remove, ins ? &ins->mol : nullptr);
	splice_vec(c->h_frozen, (size_t)at, (size_t)n_remove, ins ? &ins->frozen : nullptr);
	splice_vec(c->h_disp, (size_t)at, (size_t)n_remove, ins ? &ins->disp : nullptr);
	if (!c->h_mass.empty()) splice_vec(c->h_mass, (size_t)at, (size_t)n_remove, ins ? &ins->mass : nullptr);
	const int nt_old = c->n_tiles;
	c->n = n_new;
	c->n_pad = ((n_new + kTile - 1) / kTile) * kTile;
	c->n_tiles = c->n_pad / kTile;
	c->n_molecules = 0;
	c->N_movable = 0;
	for (int i = 0; i < n_new; i++)
		if (i == n_new - 1 || c->h_mol[i + 1] != c->h_mol[i]) {
			c->n_molecules++;
			if (!c->h_frozen[i]) c->N_movable += 1.0;
		}
	c->atoms_dirty = true;
	if (c->n_tiles != nt_old) {
		HIP_TRY(c, hipSetDevice(c->device));
		const int rc = size_tile_tables(c);
		if (rc != MPMC_OK) return rc;
	}
	return MPMC_OK;
}

static const double kHostBinom6[7] = {1, 6, 15, 20, 15, 6, 1};
static const double kHostBinom12[13] = {1, 12, 66, 220, 495, 792, 924, 792, 495, 220, 66, 12, 1};
static int xch_class(int fl) { return ((fl & AF_FROZEN) ? 1 : 0) | ((fl & AF_NULL_RD) ? 2 : 0) | ((fl & (AF_HAS_DISP | AF_DISP_RD)) ? 4 : 0) | ((fl & AF_ZERO_Q) ? 8 : 0); }

// one atom's share of the sums of k_atom_terms_part (slot for slot), times sg
void mpmc::xch_sum_atom(const mpmc_ctx *c, XchSums &xs, double sg, int fl, double sigma, double eps, double q) {
	const Box bx = lrc_box(c);
	const int rd_lrc = c->opts.rd_lrc;
	const double lx = std::fabs(sigma), ly = std::sqrt(eps);
	double *s = xs.s;
	xs.cls[xch_class(fl)] += (sg > 0) ? 1 : -1;
	if (rd_lrc && !(fl & (AF_NULL_RD | AF_NEG_SIGMA))) {
		double pw = ly;
		const bool fr = (fl & AF_FROZEN) != 0;
		for (int k = 0; k < 13; ++k) {
			s[2 + k] += sg * pw;
			if (fr) s[15 + k] += sg * pw;
			pw *= lx;
		}
		const double t2 = 2.0 * lx, t6 = (t2 * t2 * t2) * (t2 * t2 * t2), e2 = ly * ly;
		s[28] += sg * (e2 * t6);
		s[29] += sg * (e2 * t6 * t6);
		s[32] += sg;
		if (fr) {
			s[30] += sg * (e2 * t6);
			s[31] += sg * (e2 * t6 * t6);
			s[33] += sg;
		}
	}
	if (fl & AF_FROZEN) return;
	s[0] -= sg * (c->ewald_alpha * q * q / std::sqrt(kPi));
	if (rd_lrc && !(fl & AF_NULL_RD)) s[1] += sg * lrc_term(lx, eps, bx.cutoff, bx.volume);
}

void mpmc::xch_sum_list(const mpmc_ctx *c, XchSums &out) {
	out = XchSums{};
	int32_t mx = c->n > 0 ? c->h_mol[0] : 0;
	for (int i = 0; i < c->n; i++) {
		xch_sum_atom(c, out, 1.0, atom_flag_word(c, c->h_frozen[i], c->h_eps[i], c->h_sigma[i], c->h_disp[i], c->h_q[i], c->h_alpha[i]), c->h_sigma[i], c->h_eps[i], c->h_q[i]);
		mx = std::max(mx, c->h_mol[i]);
	}
	out.mol_max = mx;
}

// lrc_pair, lrc_self, es_self from the sums: k_atom_terms_finish, line by line
void mpmc::xch_static_terms(const mpmc_ctx *c, const XchSums &xs, double out3[3]) {
	const Box bx = lrc_box(c);
	const double *s = xs.s, *m = s + 2, *mf = s + 15;
	const double d6 = s[28], d12 = s[29], df6 = s[30], df12 = s[31];
	double s6 = 0, s12 = 0, f6 = 0, f12 = 0;
	for (int k = 0; k <= 6; ++k) {
		s6 += kHostBinom6[k] * m[k] * m[6 - k];
		f6 += kHostBinom6[k] * mf[k] * mf[6 - k];
	}
	for (int k = 0; k <= 12; ++k) {
		s12 += kHostBinom12[k] * m[k] * m[12 - k];
		f12 += kHostBinom12[k] * mf[k] * mf[12 - k];
	}
	const double p6 = (0.5 * (s6 - d6) - 0.5 * (f6 - df6)) / 64.0;
	const double p12 = (0.5 * (s12 - d12) - 0.5 * (f12 - df12)) / 4096.0;
	const double rc3 = bx.cutoff * bx.cutoff * bx.cutoff, rc9 = rc3 * rc3 * rc3;
	const bool no_pair = s[32] * (s[32] - 1.0) == s[33] * (s[33] - 1.0);
	out3[0] = (c->opts.rd_lrc && !no_pair) ? (16.0 / 3.0) * kPi * (p12 / (3.0 * rc9) - p6 / rc3) / bx.volume : 0.0;
	out3[1] = s[1];
	out3[2] = s[0];
}

// ---- `polar_wolf` / `polar_palmo` ------------------------------------------------------------------------------------------------------
extern "C" int mpmc_set_polar_wolf(mpmc_ctx *c, int enabled, double polar_wolf_alpha) {
	if (!c) return MPMC_ERR_ARG;
	if (c->pending || c->trial.open) return fail(c, MPMC_ERR_ARG, "mpmc_set_polar_wolf: an evaluation or a trial move is open");
	if (enabled && (!std::isfinite(polar_wolf_alpha) || polar_wolf_alpha < 0.0 || polar_wolf_alpha > 1.0)) // SimulationControl.cpp:2652-2660
		return fail(c, MPMC_ERR_INVALID_SETTING, "mpmc_set_polar_wolf: polar_wolf_alpha must be in [0, 1]");
	const bool on = enabled != 0;
	if (on != c->kept.pw_enabled || (on && polar_wolf_alpha != c->kept.pw_alpha)) {
		c->cache_valid = false; // (the accepted totals and the resident real-space field belong to the other static field)
		c->e_real_valid = false;
	}
	c->kept.pw_enabled = on;
	c->kept.pw_alpha = on ? polar_wolf_alpha : 0.0;
	return MPMC_OK;
}
extern "C" int mpmc_set_polar_palmo(mpmc_ctx *c, int enabled) {
	if (!c) return MPMC_ERR_ARG;
	if (c->pending || c->trial.open) return fail(c, MPMC_ERR_ARG, "mpmc_set_polar_palmo: an evaluation or a trial move is open");
	if ((enabled != 0) != c->kept.palmo_enabled) c->cache_valid = false; // (the accepted totals carry the correction)
	c->kept.palmo_enabled = enabled != 0;
	return MPMC_OK;
}

// ---- `polar_sor` / `polar_esor` / `polar_zodid` (thole_iterative :3450-3560, new_dipoles :3181-3211) ------------------------------------------
extern "C" int mpmc_set_polar_relax(mpmc_ctx *c, int scheme, int zodid) {
	if (!c) return MPMC_ERR_ARG;
	if (c->pending || c->trial.open) return fail(c, MPMC_ERR_ARG, "mpmc_set_polar_relax: an evaluation or a trial move is open");
	if (scheme != MPMC_POLAR_RELAX_NONE && scheme != MPMC_POLAR_RELAX_SOR && scheme != MPMC_POLAR_RELAX_ESOR)
		return fail(c, MPMC_ERR_INVALID_SETTING, "mpmc_set_polar_relax: unknown scheme (MPMC_POLAR_RELAX_NONE, _SOR or _ESOR)");
	const bool z = zodid != 0;
	if (scheme != c->kept.relax_scheme || z != c->kept.zodid) {
		c->cache_valid = false; // (the accepted totals, the tensor store and an open on-demand solve belong to the other solve)
		c->e_real_valid = false; // (the next trial move evaluates in full: zodid keeps no tensor store for a store-only sweep to patch)
		drop_pending_dipoles(c);
	}
	const bool kept_order = c->opts_set && sweeps_keep_atom_order(c, c->opts);
	c->kept.relax_scheme = scheme;
	c->kept.zodid = z;
	order_rule_changed(c, kept_order); // (`polar_gs_ranked` does not act under zodid)
	return MPMC_OK;
}
extern "C" int mpmc_polar_relax_info(mpmc_ctx *c, mpmc_relax_info *out) {
	if (!c || !out) return MPMC_ERR_ARG;
	if (c->pending) return fail(c, MPMC_ERR_ARG, "mpmc_polar_relax_info: an evaluation is in flight");
	*out = c->relax_info;
	return MPMC_OK;
}

// ---- `polar_gs_ranked` (System::pairs :1001-1029, thole_iterative :3450-3543, update_ranking :3631-3656) -----------------------------------
extern "C" int mpmc_set_polar_gs_ranked(mpmc_ctx *c, int enabled) {
	if (!c) return MPMC_ERR_ARG;
	if (c->pending || c->trial.open) return fail(c, MPMC_ERR_ARG, "mpmc_set_polar_gs_ranked: an evaluation or a trial move is open");
	const bool on = enabled != 0;
	if (on == c->kept.gs_ranked) return MPMC_OK;
	c->cache_valid = false; // (the accepted totals, the tensor store and an open on-demand solve belong to the other solve)
	c->e_real_valid = false;
	drop_pending_dipoles(c);
	c->gr_pos_gen = c->gr_static_gen = 0; // (mpmc_polar_gs_ranked_get: nothing of the other setting is handed out)
	const bool kept_order = c->opts_set && sweeps_keep_atom_order(c, c->opts);
	c->kept.gs_ranked = on;
	order_rule_changed(c, kept_order);
	return MPMC_OK;
}
extern "C" int mpmc_polar_gs_ranked_info(mpmc_ctx *c, mpmc_gs_ranked_info *out) {
	if (!c || !out) return MPMC_ERR_ARG;
	if (c->pending) return fail(c, MPMC_ERR_ARG, "mpmc_polar_gs_ranked_info: an evaluation is in flight");
	*out = c->gr_info;
	out->enabled = c->kept.gs_ranked ? 1 : 0;
	return MPMC_OK;
}
extern "C" int mpmc_polar_gs_ranked_get(mpmc_ctx *c, int32_t *rank_metric, int32_t *order) {
	if (!c) return MPMC_ERR_ARG;
	if (c->pending) return fail(c, MPMC_ERR_ARG, "mpmc_polar_gs_ranked_get: an evaluation is in flight");
	if (!c->kept.gs_ranked || !c->gr_ran || c->gr_pos_gen != c->pos_gen || c->gr_static_gen != c->static_gen)
		return fail(c, MPMC_ERR_ARG, "mpmc_polar_gs_ranked_get: no evaluation under polar_gs_ranked has been made since the atoms, the cell or the setting last changed");
	HIP_TRY(c, hipSetDevice(c->device));
	// (the sweeps keep the caller's atom order on the device: slot = atom)
	const size_t bytes = (size_t)c->n * sizeof(int32_t);
	if (rank_metric) HIP_TRY(c, hipMemcpyAsync(rank_metric, c->d_gr_rank, bytes, hipMemcpyDeviceToHost, c->stream));
	if (order) HIP_TRY(c, hipMemcpyAsync(order, c->d_gr_rank + c->max_pad, bytes, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	return MPMC_OK;
}

// (diagnostics) the device's sort on keys of the caller's: what the sweeps would run in if these were the ranks
extern "C" int mpmc_debug_gs_rank_order(mpmc_ctx *c, const int32_t *keys, int32_t *order) {
	if (!c || !keys || !order) return MPMC_ERR_ARG;
	if (c->pending || c->trial.open) return fail(c, MPMC_ERR_ARG, "mpmc_debug_gs_rank_order: an evaluation or a trial move is open");
	int rc = prepare(c);
	if (rc != MPMC_OK) return rc;
	if ((rc = c->d_gr_rank.reserve(c, 2 * (size_t)c->max_pad)) != MPMC_OK) return rc;
	if ((rc = c->d_gr_info.reserve(c, 1)) != MPMC_OK) return rc;
	c->gr_pos_gen = c->gr_static_gen = 0; // (the rank pass's results are overwritten)
	const size_t bytes = (size_t)c->n * sizeof(int32_t);
	int *d_order = c->d_gr_rank + c->max_pad;
	HIP_TRY(c, hipMemcpyAsync(c->d_gr_rank, keys, bytes, hipMemcpyHostToDevice, c->stream));
	HIP_TRY(c, hipMemsetAsync(c->d_gr_info, 0, sizeof(GsRankInfoDev), c->stream));
	launch_gs_rank_order(c->stream, atoms_view(c), c->d_gr_rank, d_order, &c->d_gr_info.p->max_rank);
	HIP_TRY(c, hipGetLastError());
	HIP_TRY(c, hipMemcpyAsync(order, d_order, bytes, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	return MPMC_OK;
}

// ---- `polar_ewald_full` (System::ewald_full :2785-2830) ------------------------------------------------------------------------------------
extern "C" int mpmc_set_polar_ewald_full(mpmc_ctx *c, int enabled, int flags) {
	if (!c) return MPMC_ERR_ARG;
	if (c->pending || c->trial.open) return fail(c, MPMC_ERR_ARG, "mpmc_set_polar_ewald_full: an evaluation or a trial move is open");
	if (flags & ~MPMC_PEF_VECTOR_KWEIGHT) return fail(c, MPMC_ERR_INVALID_SETTING, "mpmc_set_polar_ewald_full: unknown flag bits");
	const bool on = enabled != 0;
	if (on != c->kept.pef_enabled || (on && flags != c->kept.pef_flags)) {
		c->cache_valid = false; // (the accepted totals, the resident real-space field and an open on-demand solve belong to the other solve)
		c->e_real_valid = false;
		drop_pending_dipoles(c);
	}
	// (Gauss-Seidel sweeps run in atom order, the term keeps the spatial order whatever polar_gs and polar_gs_ranked say: sweeps_keep_atom_order)
	const bool kept_order = c->opts_set && sweeps_keep_atom_order(c, c->opts);
	c->kept.pef_enabled = on;
	c->kept.pef_flags = on ? flags : 0;
	order_rule_changed(c, kept_order);
	return MPMC_OK;
}
extern "C" int mpmc_polar_ewald_full_info(mpmc_ctx *c, mpmc_ewald_full_info *out) {
	if (!c || !out) return MPMC_ERR_ARG;
	if (c->pending) return fail(c, MPMC_ERR_ARG, "mpmc_polar_ewald_full_info: an evaluation is in flight");
	*out = c->pef_info;
	return MPMC_OK;
}

// ---- `rd_crystal` (System::lj :916-963, rd_crystal_self :1152-1208) ----------------------------------------------------------------------
extern "C" int mpmc_set_rd_crystal(mpmc_ctx *c, int enabled, int order) {
	if (!c) return MPMC_ERR_ARG;
	if (c->pending || c->trial.open) return fail(c, MPMC_ERR_ARG, "mpmc_set_rd_crystal: an evaluation or a trial move is open");
	if (enabled && order < 1) return fail(c, MPMC_ERR_INVALID_SETTING, "mpmc_set_rd_crystal: rd_crystal_order must be at least 1"); // SimulationControl.cpp:1688-1692
	if (enabled && order > MPMC_RD_CRYSTAL_MAX_ORDER)
		return fail(c, MPMC_ERR_INVALID_SETTING, "mpmc_set_rd_crystal: rd_crystal_order above MPMC_RD_CRYSTAL_MAX_ORDER");
	const bool on = enabled != 0;
	if (on != c->kept.rc_enabled || (on && order != c->kept.rc_order)) {
		c->cache_valid = false;  // (the accepted totals carry the other LJ term)
		c->static_dirty = true;  // (the long-range corrections are taken at the other cutoff: lrc_box)
		c->static_gen++;
	}
	c->kept.rc_enabled = on;
	c->kept.rc_order = on ? order : 0;
	return MPMC_OK;
}
extern "C" int mpmc_rd_crystal_info(mpmc_ctx *c, struct mpmc_rd_crystal_info *out) {
	if (!c || !out) return MPMC_ERR_ARG;
	*out = c->rc_info;
	return MPMC_OK;
}

// ---- the rd model (pair_exclusions, src/System.cpp:1069-1177; lj :897-1032, lj_buffered_14_7 :1212-1248, dreiding :2098-2215) ------------------
static_assert(MPMC_RD_FORM_LJ == RD_FORM_LJ && MPMC_RD_FORM_BUFFERED_14_7 == RD_FORM_BUFFERED_14_7 && MPMC_RD_FORM_DREIDING == RD_FORM_DREIDING, "pair_math.h mirrors the header");
static_assert(MPMC_RD_MIX_LB == RD_MIX_LB && MPMC_RD_MIX_WALDMAN_HAGLER == RD_MIX_WALDMAN_HAGLER && MPMC_RD_MIX_HALGREN == RD_MIX_HALGREN && MPMC_RD_MIX_C6 == RD_MIX_C6,
              "pair_math.h mirrors the header");
extern "C" int mpmc_set_rd_model(mpmc_ctx *c, int form, int mixing) {
	if (!c) return MPMC_ERR_ARG;
	if (c->pending || c->trial.open) return fail(c, MPMC_ERR_ARG, "mpmc_set_rd_model: an evaluation or a trial move is open");
	if (form < 0 || form >= RD_FORM_COUNT) return fail(c, MPMC_ERR_INVALID_SETTING, "mpmc_set_rd_model: unknown potential form (MPMC_RD_FORM_*)");
	if (mixing < 0 || mixing >= RD_MIX_COUNT) return fail(c, MPMC_ERR_INVALID_SETTING, "mpmc_set_rd_model: unknown mixing rule (MPMC_RD_MIX_*)");
	if (form != c->kept.rdm_form || mixing != c->kept.rdm_mix) {
		c->cache_valid = false; // (the accepted totals carry the other term)
		// (14-7 and DREIDING ignore rd_crystal: the long-range corrections move between the crystal cutoff and the box cutoff, lrc_box)
		if (c->kept.rc_enabled && (form != 0) != (c->kept.rdm_form != 0)) c->static_dirty = true, c->static_gen++;
	}
	c->kept.rdm_form = form;
	c->kept.rdm_mix = mixing;
	return MPMC_OK;
}
extern "C" int mpmc_rd_model_info(mpmc_ctx *c, struct mpmc_rd_model_info *out) {
	if (!c || !out) return MPMC_ERR_ARG;
	*out = c->rdm_info;
	return MPMC_OK;
}

// ---- `sg`: the Silvera-Goldman potential (System::sg, src/System.Energy.cpp:1763-1867) -----------------------------------------------------------
extern "C" int mpmc_set_silvera_goldman(mpmc_ctx *c, int enabled) {
	if (!c) return MPMC_ERR_ARG;
	if (c->pending || c->trial.open) return fail(c, MPMC_ERR_ARG, "mpmc_set_silvera_goldman: an evaluation or a trial move is open");
	const bool on = enabled != 0;
	if (on == c->kept.sg_enabled) return MPMC_OK;
	c->kept.sg_enabled = on;
	c->cache_valid = false; // (the accepted totals carry the other term)
	if (c->kept.rc_enabled) c->static_dirty = true, c->static_gen++; // (sg() ignores rd_crystal: the long-range corrections move between the crystal cutoff and the box cutoff, lrc_box)
	if (!on) c->sg_info = {};
	// no electrostatics and no polarization under the term (System::energy :46): the evaluations read the caller's options with rd_only on
	// and polarization off
	if (c->opts_set) apply_options(c, effective_options(c, c->opts_user));
	return MPMC_OK;
}
extern "C" int mpmc_silvera_goldman_info(mpmc_ctx *c, struct mpmc_silvera_goldman_info *out) {
	if (!c || !out) return MPMC_ERR_ARG;
	*out = c->sg_info;
	out->enabled = c->kept.sg_enabled ? 1 : 0;
	return MPMC_OK;
}

int mpmc::sg_ready(mpmc_ctx *c) {
	if (!sg_on(c)) return fail(c, MPMC_ERR_INVALID_SETTING, "the Silvera-Goldman term is off (mpmc_set_silvera_goldman)");
	if (rd_model_on(c))
		return fail(c, MPMC_ERR_INCOMPATIBLE, "mpmc_set_silvera_goldman with a non-default mpmc_set_rd_model: sg() mixes nothing and comes before dreiding and lj_buffered_14_7 "
		                                      "in the reference's dispatch (System.Energy.cpp:113-127); choose one");
	if (c->kept.de_enabled)
		return fail(c, MPMC_ERR_INCOMPATIBLE, "mpmc_set_silvera_goldman with mpmc_set_disp_expansion: sg() comes before disp_expansion() in the reference's dispatch "
		                                      "(System.Energy.cpp:113-127); choose one");
	if (c->kept.ca_rules & CA_RULE_SIGMA)
		return fail(c, MPMC_ERR_UNSUPPORTED, "mpmc_set_silvera_goldman with the sigma rule of cavity_autoreject: the rule lives inside lj(), which sg() replaces; use the absolute rule");
	if (c->sg_frozen_atoms < 0) { // (the flags change with the atom list only: one scan per upload, none per trial move)
		int nf = 0;
		for (int i = 0; i < c->n; i++) nf += c->h_frozen[i] ? 1 : 0;
		c->sg_frozen_atoms = nf;
	}
	if (c->sg_frozen_atoms >= 2)
		return fail(c, MPMC_ERR_UNSUPPORTED, "Silvera-Goldman with two or more frozen atoms: the reference never measures a pair of two frozen atoms here, and the reference's "
		                                     "value is not finite (inf - inf)");
	return c->d_sg_part.reserve(c, (size_t)2 * kSgBlocks);
}

SgParams mpmc::sg_params(const mpmc_ctx *c) {
	SgParams sp{};
	sp.fh = c->opts.feynman_hibbs ? 1 : 0;
	if (sp.fh) { // System::sg :1845: M2A^2 hBar^2 / (24 kB T AMU2KG mass), with hBar itself squared (constants.h:15)
		const double hBar = 1.054571e-34, kB = 1.3806503e-23, amu = 1.66053873e-27;
		sp.fh_c = 1.0e20 * (hBar * hBar / (24.0 * kB * c->opts.temperature * amu));
	}
	return sp;
}

// ---- cavity_autoreject (System.Energy.cpp:1001-1004, 1237-1239, 2182-2185; System.Cavity.cpp:211-228; SimulationControl.cpp:2139-2154) ----------
static_assert(MPMC_AUTOREJECT_SIGMA == CA_RULE_SIGMA && MPMC_AUTOREJECT_ABSOLUTE == CA_RULE_ABSOLUTE, "kernels.h mirrors the header");
extern "C" int mpmc_set_cavity_autoreject(mpmc_ctx *c, int rules, double scale, double repulsion) {
	if (!c) return MPMC_ERR_ARG;
	if (c->pending || c->trial.open) return fail(c, MPMC_ERR_ARG, "mpmc_set_cavity_autoreject: an evaluation or a trial move is open");
	if (rules & ~(MPMC_AUTOREJECT_SIGMA | MPMC_AUTOREJECT_ABSOLUTE)) return fail(c, MPMC_ERR_INVALID_SETTING, "mpmc_set_cavity_autoreject: unknown rule bits (MPMC_AUTOREJECT_*)");
	if (rules && !(scale > 0.0 && scale <= 1.0)) // SimulationControl.cpp:2139-2154 (a NaN fails the test too)
		return fail(c, MPMC_ERR_INVALID_SETTING, "mpmc_set_cavity_autoreject: cavity_autoreject_scale must be in (0, 1]");
	if (rules != c->kept.ca_rules || (rules && (scale != c->kept.ca_scale || repulsion != c->kept.ca_repulsion)))
		c->cache_valid = false; // (the accepted contact counts belong to the other setting: the next trial needs a re-basing evaluation)
	c->kept.ca_rules = rules;
	c->kept.ca_scale = rules ? scale : 0.0;
	c->kept.ca_repulsion = rules ? repulsion : 0.0;
	if (!rules) c->ca_info = {};
	return MPMC_OK;
}
extern "C" int mpmc_cavity_autoreject_info(mpmc_ctx *c, struct mpmc_cavity_autoreject_info *out) {
	if (!c || !out) return MPMC_ERR_ARG;
	if (c->pending) return fail(c, MPMC_ERR_ARG, "mpmc_cavity_autoreject_info: an evaluation is in flight");
	*out = c->ca_info;
	out->rules = c->kept.ca_rules;
	out->scale = c->kept.ca_scale;
	out->repulsion = c->kept.ca_repulsion;
	return MPMC_OK;
}

extern "C" int mpmc_insert_candidates_contacts(mpmc_ctx *c, int n_cand, int64_t *n_replaced, int64_t *n_absolute) {
	if (!c) return MPMC_ERR_ARG;
	if (c->ins_ca_n < 0) return fail(c, MPMC_ERR_ARG, "mpmc_insert_candidates_contacts: no batch of insertion candidates has run");
	if (n_cand != c->ins_ca_n) return fail(c, MPMC_ERR_ARG, "mpmc_insert_candidates_contacts: n_cand differs from the last batch's");
	for (int q = 0; q < n_cand; q++) {
		if (n_replaced) n_replaced[q] = c->ins_ca[2 * (size_t)q];
		if (n_absolute) n_absolute[q] = c->ins_ca[2 * (size_t)q + 1];
	}
	return MPMC_OK;
}

int mpmc::contact_ready(mpmc_ctx *c) {
	if (!contact_on(c)) return fail(c, MPMC_ERR_INVALID_SETTING, "cavity_autoreject is off (mpmc_set_cavity_autoreject)");
	if (c->kept.ca_rules & CA_RULE_SIGMA) {
		if (crystal_on(c))
			return fail(c, MPMC_ERR_UNSUPPORTED, "cavity_autoreject with rd_crystal: the reference tests intramolecular pairs there, which rejects every multi-site "
			                                     "molecule (System.Energy.cpp:916-1004); use the absolute rule, or rd_crystal without the sigma rule");
	}
	if (c->ca_dirty) { // (the parameters and the molecules change with the atom list only: one scan per new list, none per trial move)
		double smax = 0.0;
		int64_t frozen = 0, same = 0, run = 0;
		bool sorted = true; // (a molecule's atoms stand together in every list the readers make: one pass; otherwise the ids are sorted first)
		int32_t last = 0;
		for (int i = 0; i < c->n; i++) {
			smax = std::max(smax, std::fabs(c->h_sigma[i]));
			if (!c->h_frozen[i]) continue;
			if (frozen && c->h_mol[i] < last) sorted = false;
			if (frozen && c->h_mol[i] == last) run++;
			else same += run * (run - 1) / 2, run = 1;
			last = c->h_mol[i];
			frozen++;
		}
		same += run * (run - 1) / 2;
		if (!sorted) { // (frozen atoms of one molecule apart in the list: count by sorted ids)
			std::vector<int32_t> ids;
			for (int i = 0; i < c->n; i++)
				if (c->h_frozen[i]) ids.push_back(c->h_mol[i]);
			std::sort(ids.begin(), ids.end());
			same = 0, run = 0;
			for (size_t k = 0; k < ids.size(); k++) {
				if (k && ids[k] == ids[k - 1]) run++;
				else same += run * (run - 1) / 2, run = 1;
			}
			same += run * (run - 1) / 2;
		}
		c->ca_frozen_atoms = frozen;
		c->ca_sigma_max = smax;
		c->ca_frozen_pairs = frozen * (frozen - 1) / 2 - same;
		c->ca_dirty = false;
	}
	int rc;
	if ((rc = c->d_ca_part.reserve(c, (size_t)3 * kContactBlocks)) != MPMC_OK) return rc;
	if ((rc = c->d_ca_cls.reserve(c, (size_t)std::max(1, c->n_tile_pairs))) != MPMC_OK) return rc;
	return MPMC_OK;
}

ContactParams mpmc::contact_params(const mpmc_ctx *c) {
	ContactParams cp{};
	cp.rules = c->kept.ca_rules;
	cp.model = rd_model_on(c) ? 1 : 0;
	cp.mix = c->kept.rdm_mix;
	cp.measure_frozen = c->opts.polarization ? 1 : 0;
	cp.scale = c->kept.ca_scale;
	cp.disp = c->kept.de_enabled ? 1 : 0; // (disp_expansion() replaces lj(): its own sigma test and, with a threshold, its repulsion test)
	cp.schmidt = (c->kept.de_flags & MPMC_DISP_SCHMIDT) ? 1 : 0;
	cp.repulsion = cp.disp ? c->kept.ca_repulsion : 0.0;
	cp.t_in = (c->kept.rdm_form == RD_FORM_LJ) ? c->box.t_lj : c->box.t_es;
	// no contact at or beyond dmax: every mixing rule's sigma_ij is a mean of the two sigmas, so at most the larger one (the margin covers
	// the rounding of the mixed value and of the product)
	// (disp-expansion: sigma is r0 and r0_ij their mean; its repulsion test has no distance bound here: HUGE_VAL, everything is walked)
	const double d_sigma = !(cp.rules & CA_RULE_SIGMA) ? 0.0 : (cp.repulsion != 0.0) ? HUGE_VAL : cp.scale * c->ca_sigma_max * (1.0 + 1e-9);
	const double d_abs = (cp.rules & CA_RULE_ABSOLUTE) ? cp.scale : 0.0;
	cp.dmax = std::max(d_sigma, d_abs);
	return cp;
}

int mpmc::rd_model_ready(mpmc_ctx *c) {
	if (!rd_model_on(c)) return fail(c, MPMC_ERR_INVALID_SETTING, "the rd model is the default one (mpmc_set_rd_model)");
	if (c->kept.de_enabled)
		return fail(c, MPMC_ERR_INCOMPATIBLE, "mpmc_set_rd_model with mpmc_set_disp_expansion: the reference mixes by waldmanhagler / halgren_mixing before it reaches "
		                                      "the disp-expansion coefficients (System.cpp:1072-1158), and dreiding / lj_buffered_14_7 never read them");
	if (c->kept.rc_enabled && c->kept.rdm_form == RD_FORM_LJ)
		return fail(c, MPMC_ERR_UNSUPPORTED, "rd_crystal with a mixing rule other than Lorentz-Berthelot: the lattice sum (kernels_crystal.hip) mixes by Lorentz-Berthelot only");
	if (c->rdm_dirty) { // (the parameters change with the atom list only, and every new list is uploaded: one scan per upload, none per trial move)
		c->rdm_bad_atom = -1;
		for (int i = 0; i < c->n && c->rdm_bad_atom < 0; i++)
			if (c->h_sigma[i] < 0.0 || c->h_eps[i] < 0.0) c->rdm_bad_atom = i;
	}
	if (c->rdm_bad_atom >= 0) {
		const int i = c->rdm_bad_atom;
		if (c->h_sigma[i] < 0.0) return fail(c, MPMC_ERR_INVALID_DATUM, "rd model: atom " + std::to_string(i) + " has sigma < 0 (attractive-only sites exist under the plain Lennard-Jones term only)");
		return fail(c, MPMC_ERR_INVALID_DATUM, "rd model: atom " + std::to_string(i) + " has epsilon < 0");
	}
	int rc;
	if ((rc = c->d_rdm_sp.reserve(c, (size_t)c->max_pad)) != MPMC_OK) return rc;
	if ((rc = c->d_rdm_part.reserve(c, (size_t)3 * kRdModelBlocks)) != MPMC_OK) return rc;
	if ((rc = c->d_rdm_lrc.reserve(c, 1)) != MPMC_OK) return rc;
	if (c->rdm_dirty) { // slot order, like every other per-atom array (upload_atoms)
		std::vector<double4> sp((size_t)c->n_pad, make_double4(0.0, 0.0, 0.0, 0.0));
		for (int k = 0; k < c->n; k++) {
			const double s = c->h_sigma[c->perm[k]], s2 = s * s, s3 = s2 * s;
			sp[k] = make_double4(s, s2, s3, s3 * s3);
		}
		HIP_TRY(c, hipMemcpyAsync(c->d_rdm_sp, sp.data(), sp.size() * sizeof(double4), hipMemcpyHostToDevice, c->stream));
		HIP_TRY(c, hipStreamSynchronize(c->stream)); // (`sp` dies here; once per upload of the atoms)
		c->rdm_dirty = false;
		c->rdm_lrc_valid = false;
	}
	// the LJ form's pair correction: every pair once, whenever the atoms, the box, rd_lrc or the rule changed (never with the positions)
	const bool want = c->kept.rdm_form == RD_FORM_LJ && c->opts.rd_lrc;
	if (!c->rdm_lrc_valid || c->rdm_lrc_volume != c->box.volume || c->rdm_lrc_cutoff != c->box.cutoff || c->rdm_lrc_rd_lrc != (want ? 1 : 0) ||
	    c->rdm_lrc_mix != c->kept.rdm_mix) {
		c->rdm_lrc = 0.0;
		if (want) {
			launch_rd_model_lrc(c->stream, atoms_view(c), c->d_rdm_sp, c->d_tile_pairs, c->n_tile_pairs, c->kept.rdm_mix, c->box.cutoff, c->box.volume, c->d_rdm_part,
			                    c->d_rdm_lrc);
			HIP_TRY(c, hipGetLastError());
			HIP_TRY(c, hipMemcpyAsync(&c->rdm_lrc, c->d_rdm_lrc, sizeof(double), hipMemcpyDeviceToHost, c->stream));
			HIP_TRY(c, hipStreamSynchronize(c->stream));
		}
		c->rdm_lrc_volume = c->box.volume;
		c->rdm_lrc_cutoff = c->box.cutoff;
		c->rdm_lrc_rd_lrc = want ? 1 : 0;
		c->rdm_lrc_mix = c->kept.rdm_mix;
		c->rdm_lrc_valid = true;
	}
	return MPMC_OK;
}

// The image table S(n) in the reference's loop and association order, the cutoff with its two squared-distance thresholds, and
// crystal_self: sum over the atoms with sigma or epsilon != 0 of 4 eps_i (t12 - t6), t6 = |sigma_i|^6 sum_{n != 0, |S(n)| <= cut} 0.5 /
// |S(n)|^6 (the reference forms pow(|sigma_i| / |S(n)|, 6) per image: the same to a few ulp), t12 = 0 for sigma_i < 0.
int mpmc::crystal_ready(mpmc_ctx *c) {
	const int order = c->kept.rc_order;
	int rc;
	if ((rc = c->d_rc_part.reserve(c, (size_t)2 * kCrystalBlocks)) != MPMC_OK) return rc;
	if (c->rc_gen == c->static_gen && c->rc_table_order == order) return MPMC_OK;
	const int w = 2 * order - 1, n_img = w * w * w;
	const double cut = 2.0 * c->box.cutoff * ((double)order - 0.5);
	std::vector<double4> sh((size_t)n_img);
	const double *b = c->box.b; // b[3 q + p] = basis[q][p]
	double h6 = 0.0, h12 = 0.0;
	int k = 0, centre = 0;
	for (int i0 = -(order - 1); i0 <= order - 1; i0++)
		for (int i1 = -(order - 1); i1 <= order - 1; i1++)
			for (int i2 = -(order - 1); i2 <= order - 1; i2++, k++) {
				double a[3];
				for (int p = 0; p < 3; p++) a[p] = ((0.0 + b[p] * i0) + b[3 + p] * i1) + b[6 + p] * i2;
				sh[k] = make_double4(a[0], a[1], a[2], 0.0);
				if (!i0 && !i1 && !i2) {
					centre = k;
					continue;
				}
				const double r = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
				if (r > cut) continue;
				const double ir = 1.0 / r, ir6 = std::pow(ir, 6);
				h6 += 0.5 * ir6;
				h12 += 0.5 * (ir6 * ir6);
			}
	double self = 0.0;
	for (int i = 0; i < c->n; i++) {
		const double sg = c->h_sigma[i], ep = c->h_eps[i];
		if (sg == 0.0 && ep == 0.0) continue;
		const double s = std::fabs(sg), s2 = s * s, s6 = s2 * s2 * s2;
		const double t6 = s6 * h6, t12 = (sg < 0.0) ? 0.0 : (s6 * s6) * h12;
		self += 4.0 * ep * (t12 - t6);
	}
	if ((rc = c->d_rc_shift.reserve(c, (size_t)n_img)) != MPMC_OK) return rc;
	HIP_TRY(c, hipMemcpyAsync(c->d_rc_shift, sh.data(), sh.size() * sizeof(double4), hipMemcpyHostToDevice, c->stream));
	HIP_TRY(c, hipStreamSynchronize(c->stream)); // (`sh` dies here; once per change of the cell, the atom list or the order)
	c->rc_par = CrystalParams{};
	c->rc_par.n_img = n_img;
	c->rc_par.centre = centre;
	c->rc_par.t_pair = bisect_threshold(cut, [cut](double t) { return std::sqrt(t) - kSmallDR < cut; });
	c->rc_par.t_img = bisect_threshold(cut, [cut](double t) { return !(std::sqrt(t) > cut); });
	c->rc_cut = cut;
	c->rc_self = self;
	c->rc_gen = c->static_gen;
	c->rc_table_order = order;
	return MPMC_OK;
}

// ---- Axilrod-Teller coefficients (System::axilrod_teller, src/System.Energy.cpp:1685-1709) ------------------------------------------------
// Per atom a_i = 6.7483345 alpha_i and u_i = a_i^3 / c9_i, so that c9_abc = 3 a_a a_b a_c / (u_a + u_b + u_c) times the unit factor
// (kThreeBodyScale).  The reference gives 0 for a triple with alpha = 0 (explicitly) or c9 = 0 (1 / (c9 / a^3) is infinite); such an atom
// carries a = 0, u = 1 here, which gives the same 0 without an infinity on the device.
static void three_body_coefficients(int n, const double *alpha, int mk, const double *c6, const double *c9, std::vector<double> &au) {
	au.assign(2 * (size_t)n, 0.0);
	for (int i = 0; i < n; i++) {
		const double a = alpha[i] * 6.7483345;
		const double c9i = mk ? 3.0 / 4.0 * alpha[i] * 6.7483345 * c6[i] : c9[i]; // (Midzuno-Kihara: :1693-1697)
		const double u = 1.0 / (c9i / std::pow(a, 3));
		const bool zero = (alpha[i] == 0.0) || !std::isfinite(u) || u == 0.0;
		au[2 * (size_t)i] = zero ? 0.0 : a;
		au[2 * (size_t)i + 1] = zero ? 1.0 : u;
	}
}

extern "C" int mpmc_set_axilrod_teller(mpmc_ctx *c, int enabled, int mk, const double *c6, const double *c9) {
	if (!c) return MPMC_ERR_ARG;
	if (c->pending || c->trial.open) return fail(c, MPMC_ERR_ARG, "mpmc_set_axilrod_teller: an evaluation or a trial move is open");
	if (!enabled) {
		if (c->kept.tb_enabled) c->cache_valid = false; // (the accepted totals carry the term)
		c->kept.tb_enabled = c->kept.tb_mk = c->tb_have = c->tb_dirty = false;
		c->h_tb_au.clear();
		return MPMC_OK;
	}
	if (!c->atoms_set) return fail(c, MPMC_ERR_ARG, "mpmc_set_axilrod_teller: set the atoms first (the coefficients are per atom)");
	const double *src = mk ? c6 : c9;
	if (!src) return fail(c, MPMC_ERR_ARG, mk ? "mpmc_set_axilrod_teller: midzuno_kihara_approx needs c6" : "mpmc_set_axilrod_teller: c9 is NULL");
	for (int i = 0; i < c->n; i++)
		if (!std::isfinite(src[i])) return fail(c, MPMC_ERR_INVALID_DATUM, "mpmc_set_axilrod_teller: non-finite coefficient");
	if (three_body_tile_triples(c->n_tiles) > 0x7fffffffLL)
		return fail(c, MPMC_ERR_ARG, "mpmc_set_axilrod_teller: more tile triples than one launch can index");
	three_body_coefficients(c->n, c->h_alpha.data(), mk, c6, c9, c->h_tb_au);
	c->kept.tb_enabled = c->tb_have = c->tb_dirty = true;
	c->kept.tb_mk = mk != 0;
	c->cache_valid = false; // (the accepted totals of trial moves lack the term until the next mpmc_energy)
	return MPMC_OK;
}

// ---- disp-expansion coefficients (System::disp_expansion, src/System.Energy.cpp:1939-2080; mixing src/System.cpp:1139-1156) ------------------
// Per atom (alpha, r0) = (epsilon, sigma) of the atom list and s_n = sqrt(k_n c_n) for n = 6, 8, so that c_n,ij = s_n,i s_n,j carries the
// unit factor k_n (pair_math.h); s10 = sqrt(k10 c10), or under extrapolate_disp_coeffs sqrt(49/40 k8^2 / k6) c8 / sqrt(c6) (0 when c6 or c8
// is 0), so that s10_i s10_j is the pair's 49/40 c8_ij^2 / c6_ij.
static void disp_coefficients(int n, const double *alpha, const double *r0, int flags, const double *c6, const double *c8, const double *c10,
                              std::vector<double> &de, std::vector<double> &raw) {
	const double q6 = std::sqrt(kDispK6), q8 = std::sqrt(kDispK8), q10 = std::sqrt(kDispK10);
	const double q10x = std::sqrt(49.0 / 40.0) * kDispK8 / q6;
	de.assign(5 * (size_t)n, 0.0);
	raw.assign(3 * (size_t)n, 0.0);
	for (int i = 0; i < n; i++) {
		const double a6 = c6[i], a8 = c8[i], a10 = c10 ? c10[i] : 0.0;
		double *d = &de[5 * (size_t)i];
		d[0] = alpha[i];
		d[1] = r0[i];
		d[2] = q6 * std::sqrt(a6);
		d[3] = q8 * std::sqrt(a8);
		d[4] = (flags & MPMC_DISP_EXTRAPOLATE_C10) ? ((a6 != 0.0 && a8 != 0.0) ? q10x * (a8 / std::sqrt(a6)) : 0.0) : q10 * std::sqrt(a10);
		raw[3 * (size_t)i] = a6, raw[3 * (size_t)i + 1] = a8, raw[3 * (size_t)i + 2] = a10;
	}
}

DispParams mpmc::disp_params(const mpmc_ctx *c) {
	DispParams dp;
	dp.damp = (c->kept.de_flags & MPMC_DISP_DAMP) ? 1 : 0;
	dp.schmidt = (c->kept.de_flags & MPMC_DISP_SCHMIDT) ? 1 : 0;
	return dp;
}

// the two long-range corrections (disp_expansion_lrc over every pair that is not frozen -- rd_excluded ones included -- and
// disp_expansion_lrc_self over every atom that is not frozen, with the atom's unconverted coefficients, :2022-2034, :2056-2080).  The pair
// sum is the moment form sum_{i<j} s_i s_j = ((sum s)^2 - sum s^2) / 2 over all atoms minus the same over the frozen ones, in long double.
static void disp_lrc(mpmc_ctx *c) {
	c->de_lrc[0] = c->de_lrc[1] = 0.0;
	if (c->opts.rd_lrc) {
		const double rc = c->box.cutoff, V = c->box.volume;
		long double S[3][2] = {{0, 0}, {0, 0}, {0, 0}}, Q[3][2] = {{0, 0}, {0, 0}, {0, 0}}; // [coefficient][all, frozen]
		double self = 0.0;
		const bool ex = (c->kept.de_flags & MPMC_DISP_EXTRAPOLATE_C10) != 0;
		for (int i = 0; i < c->n; i++) {
			const double *d = &c->h_de[5 * (size_t)i];
			const bool fr = c->h_frozen[i] != 0;
			for (int k = 0; k < 3; k++) {
				const long double v = d[2 + k];
				S[k][0] += v, Q[k][0] += v * v;
				if (fr) S[k][1] += v, Q[k][1] += v * v;
			}
			if (!fr) {
				const double *r = &c->h_de_raw[3 * (size_t)i];
				const double c10 = ex ? ((r[0] != 0.0 && r[1] != 0.0) ? 49.0 / 40.0 * r[1] * r[1] / r[0] : 0.0) : r[2];
				self += disp_lrc_term(r[0], r[1], c10, rc, V);
			}
		}
		double P[3];
		for (int k = 0; k < 3; k++) P[k] = (double)(((S[k][0] * S[k][0] - Q[k][0]) - (S[k][1] * S[k][1] - Q[k][1])) * 0.5L);
		c->de_lrc[0] = disp_lrc_term(P[0], P[1], P[2], rc, V); // (the unit factors ride in the per-atom values)
		c->de_lrc[1] = self;
	}
	c->de_lrc_volume = c->box.volume;
	c->de_lrc_cutoff = c->box.cutoff;
	c->de_lrc_rd_lrc = c->opts.rd_lrc;
	c->de_lrc_valid = true;
}

extern "C" int mpmc_set_disp_expansion(mpmc_ctx *c, int enabled, int flags, const double *c6, const double *c8, const double *c10) {
	if (!c) return MPMC_ERR_ARG;
	if (c->pending || c->trial.open) return fail(c, MPMC_ERR_ARG, "mpmc_set_disp_expansion: an evaluation or a trial move is open");
	if (flags & ~(MPMC_DISP_DAMP | MPMC_DISP_EXTRAPOLATE_C10 | MPMC_DISP_SCHMIDT)) return fail(c, MPMC_ERR_ARG, "mpmc_set_disp_expansion: unknown flag bits");
	// (a context with rd_crystal set takes its long-range corrections at the crystal cutoff only while this term is off: lrc_box)
	if ((enabled != 0) != c->kept.de_enabled && c->kept.rc_enabled) c->static_dirty = true, c->static_gen++;
	if (!enabled) {
		if (c->kept.de_enabled) c->cache_valid = false, c->atoms_dirty = true; // (the accepted totals carry the term; the atoms' flags change back)
		c->kept.de_enabled = c->de_have = c->de_dirty = c->de_lrc_valid = false;
		c->kept.de_flags = 0;
		c->h_de.clear();
		c->h_de_raw.clear();
		return MPMC_OK;
	}
	if (!c->atoms_set) return fail(c, MPMC_ERR_ARG, "mpmc_set_disp_expansion: set the atoms first (the coefficients are per atom)");
	if (!c6 || !c8) return fail(c, MPMC_ERR_ARG, "mpmc_set_disp_expansion: c6 and c8 are required (c10 may be NULL: zeros)");
	for (int i = 0; i < c->n; i++) {
		const double v[3] = {c6[i], c8[i], c10 ? c10[i] : 0.0};
		for (double x : v)
			if (!std::isfinite(x) || x < 0.0) return fail(c, MPMC_ERR_INVALID_DATUM, "mpmc_set_disp_expansion: coefficients must be finite and >= 0");
	}
	disp_coefficients(c->n, c->h_eps.data(), c->h_sigma.data(), flags, c6, c8, c10, c->h_de, c->h_de_raw);
	if (!c->kept.de_enabled) c->atoms_dirty = true; // (the atoms' dispersion flag becomes AF_DISP_RD: upload_atoms)
	c->kept.de_enabled = c->de_have = c->de_dirty = true;
	c->de_lrc_valid = false;
	c->kept.de_flags = flags;
	c->cache_valid = false; // (the accepted totals of trial moves lack the term until the next mpmc_energy)
	return MPMC_OK;
}

int mpmc::disp_ready(mpmc_ctx *c) {
	if (!c->kept.de_enabled) return fail(c, MPMC_ERR_INVALID_SETTING, "the disp-expansion term is off (mpmc_set_disp_expansion)");
	if (!c->de_have)
		return fail(c, MPMC_ERR_ARG, "the disp-expansion term is on but has no coefficients for this atom list (mpmc_set_disp_expansion after mpmc_set_atoms)");
	int rc;
	if ((rc = c->d_de_co.reserve(c, (size_t)c->max_pad)) != MPMC_OK) return rc;
	if ((rc = c->d_de_t10.reserve(c, (size_t)c->max_pad)) != MPMC_OK) return rc;
	if ((rc = c->d_de_part.reserve(c, (size_t)kDispBlocks)) != MPMC_OK) return rc;
	if (c->de_dirty) { // slot order, like every other per-atom array (upload_atoms)
		std::vector<double4> co((size_t)c->n_pad, make_double4(0.0, 0.0, 0.0, 0.0));
		std::vector<double> t10((size_t)c->n_pad, 0.0);
		for (int k = 0; k < c->n; k++) {
			const double *d = &c->h_de[5 * (size_t)c->perm[k]];
			co[k] = make_double4(d[0], d[1], d[2], d[3]);
			t10[k] = d[4];
		}
		HIP_TRY(c, hipMemcpyAsync(c->d_de_co, co.data(), co.size() * sizeof(double4), hipMemcpyHostToDevice, c->stream));
		HIP_TRY(c, hipMemcpyAsync(c->d_de_t10, t10.data(), t10.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
		HIP_TRY(c, hipStreamSynchronize(c->stream)); // (`co`, `t10` die here; once per upload of the atoms)
		c->de_dirty = false;
	}
	// the corrections follow the box (mpmc_set_box: volume moves) and rd_lrc, never the positions
	if (!c->de_lrc_valid || c->de_lrc_volume != c->box.volume || c->de_lrc_cutoff != c->box.cutoff || c->de_lrc_rd_lrc != c->opts.rd_lrc) disp_lrc(c);
	return MPMC_OK;
}

int mpmc::three_body_ready(mpmc_ctx *c) {
	if (!c->kept.tb_enabled) return fail(c, MPMC_ERR_INVALID_SETTING, "the Axilrod-Teller term is off (mpmc_set_axilrod_teller)");
	if (!c->tb_have)
		return fail(c, MPMC_ERR_ARG, "the Axilrod-Teller term is on but has no coefficients for this atom list (mpmc_set_axilrod_teller after mpmc_set_atoms)");
	int rc;
	if ((rc = c->d_tb_au.reserve(c, (size_t)c->max_pad)) != MPMC_OK) return rc;
	if ((rc = c->d_tb_part.reserve(c, (size_t)kThreeBodyBlocks)) != MPMC_OK) return rc;
	if (c->tb_dirty) { // slot order, like every other per-atom array (upload_atoms)
		std::vector<double2> au((size_t)c->n_pad, make_double2(0.0, 1.0));
		for (int k = 0; k < c->n; k++) {
			const int i = c->perm[k];
			au[k] = make_double2(c->h_tb_au[2 * (size_t)i], c->h_tb_au[2 * (size_t)i + 1]);
		}
		HIP_TRY(c, hipMemcpyAsync(c->d_tb_au, au.data(), au.size() * sizeof(double2), hipMemcpyHostToDevice, c->stream));
		HIP_TRY(c, hipStreamSynchronize(c->stream)); // (`au` dies here; once per upload of the atoms)
		c->tb_dirty = false;
	}
	return MPMC_OK;
}

extern "C" int mpmc_update_positions(mpmc_ctx *c, int first, int count, const double *pos) {
	if (!c || !pos || first < 0 || count < 0) return MPMC_ERR_ARG;
	if (!c->atoms_set || first + count > c->n) return fail(c, MPMC_ERR_ARG, "mpmc_update_positions: range outside the atom list");
	if (count == 0) return MPMC_OK;
	HIP_TRY(c, hipSetDevice(c->device));
	vol_abandon(c);
	for (int t = 0; t < count; t++) {
		if (!std::isfinite(pos[3 * t]) || !std::isfinite(pos[3 * t + 1]) || !std::isfinite(pos[3 * t + 2]))
			return fail(c, MPMC_ERR_INVALID_DATUM, "mpmc_update_positions: non-finite position");
	}
	for (int t = 0; t < count; t++) {
		const int i = first + t;
		c->h_pos[3 * i] = pos[3 * t];
		c->h_pos[3 * i + 1] = pos[3 * t + 1];
		c->h_pos[3 * i + 2] = pos[3 * t + 2];
	}
	c->pos_gen++;
	c->cache_valid = false; // the accepted totals no longer describe the resident configuration
	drop_pending_dipoles(c); // (... nor can an open on-demand solve be finished on them)
	if (c->atoms_dirty) return MPMC_OK; // a full (re-sorted) upload is pending anyway
	if (count > 256) { // bulk update (typically: all positions handed over in host memory for every evaluation)
		// The atoms keep their slots -- the spatial order only matters for speed, the tile classes are recomputed from the actual
		// bounding boxes every evaluation -- and the whole position array goes up in ONE copy.  The order is refreshed (full upload)
		// once some atom has drifted further than kResortDrift from where it stood at the last sort.
		double worst = 0.0;
		for (int t = 0; t < count; t++) {
			const int i = first + t;
			double d2 = 0;
			for (int p = 0; p < 3; p++) {
				const double d = pos[3 * t + p] - c->h_pos_sorted[3 * (size_t)i + p];
				d2 += d * d;
			}
			if (d2 > worst) worst = d2;
		}
		if (c->h_pos_sorted.empty() || !(worst <= kResortDrift * kResortDrift)) {
			c->atoms_dirty = c->atoms_dirty_order = true;
			return MPMC_OK;
		}
	}
	// the atoms keep their slots; their new positions go through the pinned slot-ordered mirror: one asynchronous copy of the whole array
	// (a handful of atoms: one small copy each), an event behind it.  No stream synchronisation: the next writer of the mirror waits
	// for this copy (mirror_guard), nobody waits for the evaluations that may be queued in front of it.
	{
		const int rc_g = mirror_guard(c);
		if (rc_g != MPMC_OK) return rc_g;
	}
	for (int t = 0; t < count; t++) {
		const int i = first + t;
		c->h_xyzq[c->slot_of[i]] = make_double4(pos[3 * t], pos[3 * t + 1], pos[3 * t + 2], c->h_q[i]);
	}
	if (count > 4) {
		HIP_TRY(c, hipMemcpyAsync(c->d_xyzq, c->h_xyzq, (size_t)c->n_pad * sizeof(double4), hipMemcpyHostToDevice, c->stream));
	} else {
		for (int t = 0; t < count; t++) {
			const int k = c->slot_of[first + t];
			HIP_TRY(c, hipMemcpyAsync(c->d_xyzq + k, c->h_xyzq + k, sizeof(double4), hipMemcpyHostToDevice, c->stream));
		}
	}
	HIP_TRY(c, hipEventRecord(c->ev_xyzq, c->stream));
	c->xyzq_in_flight = true;
	return MPMC_OK;
}

extern "C" int mpmc_set_positions_device(mpmc_ctx *c, const double *pos_device) {
	if (!c || !pos_device) return MPMC_ERR_ARG;
	if (!c->atoms_set) return fail(c, MPMC_ERR_ARG, "mpmc_set_positions_device: no atoms set");
	if (c->trial.open) return fail(c, MPMC_ERR_ARG, "mpmc_set_positions_device: a trial move is open (accept or reject it first)");
	if (c->pending) return fail(c, MPMC_ERR_ARG, "mpmc_set_positions_device: an evaluation is in flight (mpmc_energy_wait first)");
	c->cache_valid = false; // the accepted totals / structure factors no longer describe the resident configuration
	drop_pending_dipoles(c);
	HIP_TRY(c, hipSetDevice(c->device));
	if (c->atoms_dirty) { // need the slot order first
		int rc = upload_atoms(c);
		if (rc != MPMC_OK) return rc;
	}
	launch_set_positions(c->stream, pos_device, c->d_perm, c->d_xyzq, c->n);
	HIP_TRY(c, hipGetLastError());
	// keep the host mirror coherent (update_com / later partial updates read it)
	HIP_TRY(c, hipMemcpyAsync(c->h_pos.data(), pos_device, 3 * (size_t)c->n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
	c->pos_gen++;
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	{
		const int rc_g = mirror_guard(c);
		if (rc_g != MPMC_OK) return rc_g;
	}
	for (int i = 0; i < c->n; i++) { // ... and the slot-ordered mirror a later mpmc_update_positions uploads as a whole
		double4 &v = c->h_xyzq[c->slot_of[i]];
		v.x = c->h_pos[3 * (size_t)i], v.y = c->h_pos[3 * (size_t)i + 1], v.z = c->h_pos[3 * (size_t)i + 2];
	}
	return MPMC_OK;
}


// ---- measurement -----------------------------------------------------------------------------------------
extern "C" int mpmc_set_profiling(mpmc_ctx *c, int enabled) {
	if (!c) return MPMC_ERR_ARG;
	c->kept.prof = enabled != 0;
	return MPMC_OK;
}
extern "C" int mpmc_get_timings(mpmc_ctx *c, mpmc_timings *out, int reset) {
	if (!c || !out) return MPMC_ERR_ARG;
	HIP_TRY(c, hipSetDevice(c->device));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	prof_harvest(c);
	*out = c->kept.tim;
	if (reset) std::memset(&c->kept.tim, 0, sizeof(c->kept.tim));
	return MPMC_OK;
}
extern "C" int mpmc_synchronize(mpmc_ctx *c) {
	if (!c) return MPMC_ERR_ARG;
	HIP_TRY(c, hipSetDevice(c->device));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	return MPMC_OK;
}
extern "C" int mpmc_get_tile_stats(mpmc_ctx *c, int64_t out4[4]) {
	if (!c || !out4) return MPMC_ERR_ARG;
	if (!c->atoms_set || !c->d_cls) return fail(c, MPMC_ERR_ARG, "mpmc_get_tile_stats: no evaluation has run");
	HIP_TRY(c, hipSetDevice(c->device));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	std::vector<int> cls((size_t)c->n_tile_pairs);
	HIP_TRY(c, hipMemcpyAsync(cls.data(), c->d_cls, cls.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	out4[0] = c->n_tile_pairs;
	out4[1] = out4[2] = out4[3] = 0;
	for (int v : cls) {
		if (v & CLS_THOLE_FAR) out4[2]++;
		else out4[1]++;
		if (v & CLS_BEYOND_CUTOFF) out4[3]++;
	}
	return MPMC_OK;
}

// measurement (bench.py's roofline): exact ATOM-pair counts behind the tile-pair classes of the last evaluation.  out[12] =
//   0 all pairs N(N-1)/2      1 pairs of the tile pairs whose tensors are stored      2 ... of the far-field tile pairs      3 ... of the
//   tile pairs beyond the cutoff      4 / 5  sum over the stored / far tile pairs of pairs x (dimensions WITHOUT a tile-pair-wide image)
//   6 pairs the pair sweep walks (not beyond the cutoff, or stored)      7 the same sum of pairs x non-uniform dimensions over those
//   8 tile pairs      9 stored      10 far      11 beyond the cutoff
extern "C" int mpmc_debug_pair_stats(mpmc_ctx *c, int64_t out[12]) {
	if (!c || !out) return MPMC_ERR_ARG;
	if (!c->atoms_set || !c->d_cls) return fail(c, MPMC_ERR_ARG, "mpmc_debug_pair_stats: no evaluation has run");
	HIP_TRY(c, hipSetDevice(c->device));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	std::vector<int> cls((size_t)c->n_tile_pairs);
	HIP_TRY(c, hipMemcpyAsync(cls.data(), c->d_cls, cls.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	for (int k = 0; k < 12; k++) out[k] = 0;
	const int nt = c->n_tiles;
	const bool uni = !(c->kept.tune.no_uniform || c->kept.tune.no_classes);
	auto real = [&](int T) { return (int64_t)std::max(0, std::min(kTile, c->n - T * kTile)); };
	size_t t = 0;
	for (int I = 0; I < nt; I++)
		for (int J = I; J < nt; J++, t++) {
			const int v = cls[t];
			const int64_t pairs = (I == J) ? real(I) * (real(I) - 1) / 2 : real(I) * real(J);
			const int um = uni ? ((v / CLS_UNIFORM_X) & 7) : 0;
			const int64_t nu = 3 - ((um & 1) + ((um >> 1) & 1) + ((um >> 2) & 1));
			const bool far = (v & CLS_THOLE_FAR) != 0, beyond = (v & CLS_BEYOND_CUTOFF) != 0;
			out[0] += pairs;
			out[far ? 2 : 1] += pairs;
			out[far ? 5 : 4] += pairs * nu;
			if (beyond) out[3] += pairs;
			if (!beyond || !far) {
				out[6] += pairs;
				out[7] += pairs * nu;
			}
			out[8]++;
			out[far ? 10 : 9]++;
			if (beyond) out[11]++;
		}
	return MPMC_OK;
}

// (diagnostics, read-only) the tile-pair classes of the RANKED VIEW of the last evaluation (build_ranked_view: rebuilt from the gathered atoms),
// as mpmc_debug_pair_stats counts those of the atom order.  out[6] =
//   0 tile pairs      1 off-diagonal tile pairs      2 far      3 beyond the cutoff      4 with one image index for the whole tile pair in
//   some dimension      5 ... where that common image is not the zero image (4 and 5: 0 with uniform_images or tile_classes off)
extern "C" int mpmc_debug_gs_ranked_pair_stats(mpmc_ctx *c, int64_t out[6]) {
	if (!c || !out) return MPMC_ERR_ARG;
	if (c->pending || c->trial.open) return fail(c, MPMC_ERR_ARG, "mpmc_debug_gs_ranked_pair_stats: an evaluation or a trial move is open");
	if (!c->kept.gs_ranked || !c->gr_ran || c->gr_info.ranked_sweeps < 1 || c->gr_pos_gen != c->pos_gen || c->gr_static_gen != c->static_gen || !c->d_gr_cls)
		return fail(c, MPMC_ERR_ARG, "mpmc_debug_gs_ranked_pair_stats: the last evaluation swept no ranked view");
	HIP_TRY(c, hipSetDevice(c->device));
	const bool uni = !(c->kept.tune.no_uniform || c->kept.tune.no_classes) && c->d_gr_shift;
	std::vector<int> cls((size_t)c->n_tile_pairs);
	std::vector<double4> shift(uni ? (size_t)c->n_tile_pairs : 0);
	HIP_TRY(c, hipMemcpyAsync(cls.data(), c->d_gr_cls, cls.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
	if (uni) HIP_TRY(c, hipMemcpyAsync(shift.data(), c->d_gr_shift, shift.size() * sizeof(double4), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	for (int k = 0; k < 6; k++) out[k] = 0;
	const int nt = c->n_tiles;
	size_t t = 0;
	for (int I = 0; I < nt; I++)
		for (int J = I; J < nt; J++, t++) {
			out[0]++;
			if (I == J) continue;
			const int v = cls[t];
			out[1]++;
			if (v & CLS_THOLE_FAR) out[2]++;
			if (v & CLS_BEYOND_CUTOFF) out[3]++;
			const int um = uni ? ((v / CLS_UNIFORM_X) & 7) : 0;
			if (!um) continue;
			out[4]++;
			const double sh[3] = {shift[t].x, shift[t].y, shift[t].z};
			bool moved = false;
			// orthorhombic cell: component d belongs to dimension d; any other: the shift is the sum over the common lattice directions
			for (int d = 0; d < 3; d++) moved = moved || (sh[d] != 0.0 && (!c->box.ortho || ((um >> d) & 1)));
			if (moved) out[5]++;
		}
	return MPMC_OK;
}

// Measurement / A-B switches (struct mpmc_tuning, context.h).  With a context: that context, from its next evaluation on; with a null
// context: the default that contexts created afterwards in this process start from.  The library reads no environment variable for
// any of this.  Keys (value 1 = on, 0 = off unless said otherwise):
//   side_stream -1 | 0 | 1     pair_kernel 0 | 1 | 2     pair_waves 0 | 1 | 4     panels     uniform_images     tile_classes
//   single_launch     recip_table     spatial_sort     order_carry     polar_delta     inline_move     trace_panel     tensor_budget_mb N
//   direct_budget_mb N (-1: free device memory)     dipoles_on_demand (0: every evaluation runs all its Jacobi iterations at once)
//   pef_phase_table (0: `polar_ewald_full` recomputes its phases in every pass)
//   contact_skip (0: the contact walk of cavity_autoreject walks every tile pair)
extern "C" int mpmc_debug_configure(mpmc_ctx *c, const char *key, double value) {
	if (!key) return MPMC_ERR_ARG;
	std::unique_lock<std::mutex> tuning_lk(g_tuning_mu, std::defer_lock);
	if (!c) tuning_lk.lock();
	mpmc_tuning &t = c ? c->kept.tune : g_tuning_default;
	const std::string k(key);
	const int v = (int)value;
	const bool on = (value != 0.0);
	if (k == "side_stream") {
		if (v < -1 || v > 1) return MPMC_ERR_ARG;
		t.stream_mode = v;
	} else if (k == "pair_kernel") {
		if (v < 0 || v > 2) return MPMC_ERR_ARG;
		t.pair_kernel = v;
	} else if (k == "pair_waves") {
		if (v != 0 && v != 1 && v != 4) return MPMC_ERR_ARG;
		t.pair_waves = v;
	} else if (k == "fast_geometry") t.fast_geometry = on;
	else if (k == "dense_symmetric") t.dense_symmetric = on;
	else if (k == "sort_grid") {
		if (v < -1 || v > 0) return MPMC_ERR_ARG;
		t.sort_grid = v;
		if (c) c->atoms_dirty = c->atoms_dirty_order = true;
	} else if (k == "sort_nx") {
		t.sort_nx = v;
		if (c) c->atoms_dirty = c->atoms_dirty_order = true;
	} else if (k == "sort_ny") {
		t.sort_ny = v;
		if (c) c->atoms_dirty = c->atoms_dirty_order = true;
	}
	else if (k == "side_after_sweep") t.side_after_sweep = on;
	else if (k == "poll_long") t.poll_long = on;
	else if (k == "poll_retire") t.poll_retire = on;
	else if (k == "lazy_side_stream") t.lazy_side_stream = on;
	else if (k == "pair_split_tail") {
		if (v < -1 || v > 1000) return MPMC_ERR_ARG;
		t.pair_split_tail = v;
	} else if (k == "pair_split") {
		if (v < -1 || v > 1) return MPMC_ERR_ARG;
		t.pair_split = v;
	} else if (k == "panels") t.use_panels = on;
	else if (k == "sweep_order") {
		if (v < 0 || v > 1) return MPMC_ERR_ARG;
		t.sweep_order = v;
		if (c) c->sweep_tiles = -1, c->atoms_dirty = true; // (the table is rebuilt with the next upload)
	} else if (k == "sweep_lds_pad") {
		if (v < 0 || v > 65536) return MPMC_ERR_ARG;
		t.sweep_lds_pad = v;
	}
	else if (k == "uniform_images") t.no_uniform = !on;
	else if (k == "tile_classes") t.no_classes = !on;
	else if (k == "single_launch") t.single_launch = on;
	else if (k == "recip_table") t.no_recip_tab = !on;
	else if (k == "spatial_sort") {
		t.no_sort = !on;
		if (c) c->atoms_dirty = c->atoms_dirty_order = true; // (the order changes with the next upload)
	} else if (k == "order_carry") t.no_order_carry = !on;
	else if (k == "polar_delta") t.no_polar_delta = !on;
	else if (k == "inline_move") t.no_inline_move = !on;
	else if (k == "contact_skip") t.no_contact_skip = !on;
	else if (k == "trace_panel") t.trace_panel = on;
	else if (k == "dipoles_on_demand") t.dipoles_on_demand = on;
	else if (k == "pef_phase_table") t.pef_phase_table = on;
	else if (k == "virtual_device") {
		if (!c || v < -1 || v > 63) return MPMC_ERR_ARG;
		t.virtual_device = v;
	} else if (k == "fail_next_wait") {
		if (!c) return MPMC_ERR_ARG;
		t.fail_next_wait = on ? 1 : 0;
	}
	else if (k == "panel_replicas") {
		if (!c || v < 1 || v > 64) return MPMC_ERR_ARG;
		c->debug_panel_replicas = v;
	} else if (k == "direct_budget_mb") {
		t.direct_budget_mb = (long long)value;
	} else if (k == "tensor_budget_mb") {
		if (value < 0) return MPMC_ERR_ARG;
		t.tensor_budget_mb = (long long)value;
	} else return MPMC_ERR_ARG;
	// an open on-demand solve was enqueued under the old switches (the keys that only steer a measurement or a wait leave it alone)
	if (c && k != "panel_replicas" && k != "fail_next_wait" && k != "virtual_device" && k != "trace_panel") drop_pending_dipoles(c);
	return MPMC_OK;
}
// the last evaluated trial move: 1 = a full evaluation of the trial configuration, 0 = per-move delta energies, -1 = none
extern "C" int mpmc_debug_last_trial_was_full(mpmc_ctx *c) { return (c && c->trial_last_kind >= 0) ? c->trial_last_kind : -1; }
// which kernel ran the pair pass of the last evaluation: 1 the fast sweep, 0 k_pair_fused
extern "C" int mpmc_debug_last_pair_kernel(mpmc_ctx *c) { return c ? (c->last_pair_was_sweep ? 1 : 0) : -1; }

// how this context's host waits ended since it was created: out[4] = polls that saw the device's post, polls that ran out of their
// budget (the wait then synchronised the stream), stream synchronisations, yields taken inside long polls (poll_posted, context.h)
extern "C" int mpmc_debug_wait_counters(mpmc_ctx *c, long long *out4) {
	if (!c || !out4) return -1;
	out4[0] = c->kept.n_poll_hits;
	out4[1] = c->kept.n_poll_timeouts;
	out4[2] = c->kept.n_stream_syncs;
	out4[3] = c->kept.n_poll_yields;
	return 0;
}

// diagnostics only (tests assert that the order was really carried): uploads of the atom list that kept the order / that sorted
extern "C" int mpmc_debug_upload_counts(mpmc_ctx *c, long long *out2) {
	if (!c || !out2) return -1;
	out2[0] = c->kept.n_uploads_carried;
	out2[1] = c->kept.n_uploads_sorted;
	return 0;
}

// diagnostics only (tests assert which path an exchange trial took and that the host sums were re-made): exchange trials evaluated on the
// delta path / in full, and summations of xs_acc over the whole list
extern "C" int mpmc_debug_exchange_counts(mpmc_ctx *c, long long *out3) {
	if (!c || !out3) return -1;
	out3[0] = c->kept.n_xch_delta;
	out3[1] = c->kept.n_xch_full;
	out3[2] = c->kept.n_xch_resums;
	return 0;
}

// measurement only: per-workgroup time stamps of the last panel launch (tools/panel_trace.py); 0 entries unless the context was configured with trace_panel = 1
extern "C" int mpmc_debug_panel_trace(mpmc_ctx *c, long long *out4, int max_entries) {
	if (!c || !out4) return -1;
	if (!c->d_trace) return 0;
	const int n = std::min(max_entries, c->n_panel_entries);
	if (hipSetDevice(c->device) != hipSuccess) return -1;
	if (hipMemcpyAsync(out4, c->d_trace, (size_t)n * 4 * sizeof(long long), hipMemcpyDeviceToHost, c->stream) != hipSuccess) return -1;
	if (hipStreamSynchronize(c->stream) != hipSuccess) return -1;
	return n;
}

// measurement only: the work table of the panel kernel, { tile pair A, tile pair B or -1, uniform mask | far << 3 | diagonal << 4, J } per workgroup
extern "C" int mpmc_debug_panel_table(mpmc_ctx *c, int *out4, int max_entries) {
	if (!c || !out4) return -1;
	if (!c->d_panels || !c->panels_built) return 0;
	const int n = std::min(max_entries, c->n_panel_entries);
	if (hipSetDevice(c->device) != hipSuccess) return -1;
	if (hipMemcpyAsync(out4, c->d_panels, (size_t)n * 4 * sizeof(int), hipMemcpyDeviceToHost, c->stream) != hipSuccess) return -1;
	if (hipStreamSynchronize(c->stream) != hipSuccess) return -1;
	return n;
}

extern "C" int mpmc_memory_usage(mpmc_ctx *c, int64_t *total, int64_t *tensor) {
	if (!c) return MPMC_ERR_ARG;
	if (total) *total = c->bytes_total;
	if (tensor) *tensor = (c->solver_used == MPMC_SOLVER_COMPACT) ? (int64_t)(c->d_ab.cap * sizeof(double2)) : 0;
	return MPMC_OK;
}
