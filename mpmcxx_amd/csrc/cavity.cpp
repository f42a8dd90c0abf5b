// cavity.cpp -- the cavity-bias grid of uVT moves on the host side: System::cavity_update_grid with update_cavity_probability and
// update_cavity_volume (reference src/System.Cavity.cpp:15-188), the pick of an insertion point (src/System.MonteCarlo.cpp:742-764) and the
// ENSEMBLE_UVT branch of System::boltzmann_factor (:1358-1422).  The kernels are kernels_cavity.hip's.  Nothing here reads or writes what an
// evaluation or a trial move owns: the wrapped positions are made from the host mirror and uploaded into buffers of the grid's own, so an
// update may stand straight behind an accepted exchange trial whose upload is still pending, and it leaves cache_valid, the structure
// factors, pending dipoles and the trial state alone.  (part of libmpmc_energy.so; there is no CPU fallback for the update.)
#include "context.h"

using namespace mpmc;

// ---- host only, no device needed --------------------------------------------------------------------------------------------------------
extern "C" int mpmc_cavity_num_darts(double volume) {
	const double DARTSCALE = 0.1; // update_cavity_volume :124-132
	return (int)(volume * DARTSCALE);
}

extern "C" int mpmc_cavity_grid_point(const double basis[9], int grid_size, int i, int j, int k, double pos[3]) {
	if (!basis || !pos || grid_size <= 0 || i < 0 || j < 0 || k < 0 || i >= grid_size || j >= grid_size || k >= grid_size) return MPMC_ERR_ARG;
	const int idx[3] = {i, j, k};
	double comp[3];
	for (int q = 0; q < 3; q++) comp[q] = ((double)(idx[q] + 1)) / ((double)(grid_size + 1)); // :44-46
	for (int p = 0; p < 3; p++) {                                                              // :49-53
		pos[p] = 0;
		for (int q = 0; q < 3; q++) pos[p] += basis[3 * q + p] * comp[q];
	}
	for (int p = 0; p < 3; p++) // :56-58
		for (int q = 0; q < 3; q++) pos[p] -= 0.5 * basis[3 * q + p];
	return MPMC_OK;
}

// the smallest double T whose correctly rounded square root is >= radius: sqrt(r) < radius <=> r < T for every double r (sqrt is monotone)
extern "C" double mpmc_cavity_r2_threshold(double radius) {
	if (!(radius > 0.0) || !std::isfinite(radius)) return std::nan("");
	double t = radius * radius;
	if (!std::isfinite(t)) return std::nan("");
	while (t > 0.0 && std::sqrt(t) >= radius) t = std::nextafter(t, 0.0);
	while (std::sqrt(t) < radius) t = std::nextafter(t, INFINITY);
	return t;
}

// System::boltzmann_factor, case ENSEMBLE_UVT (same branch order, same expressions); N is observables->N as the reference reads it there
extern "C" int mpmc_uvt_boltzmann_factor(const mpmc_uvt_move *m, double *boltzmann_factor) {
	if (!m || !boltzmann_factor) return MPMC_ERR_ARG;
	constexpr double ATM2REDUCED = 0.0073389366; // src/constants.h
	const double delta_energy = m->final_energy - m->init_energy;
	const double temperature = m->temperature, fugacity = m->fugacity, N = m->N, volume = m->volume, cavity_volume = m->cavity_volume,
	             probability = m->avg_cavity_probability;
	const int sorbateCount = m->sorbate_count;
	if (m->biased_move) { // modified Metropolis function (:1368-1389)
		switch (m->movetype) {
		case MPMC_MOVETYPE_INSERT:
			*boltzmann_factor = (cavity_volume * probability * fugacity * ATM2REDUCED / (temperature * N)) * std::exp(-delta_energy / temperature) * (double)sorbateCount;
			return MPMC_OK;
		case MPMC_MOVETYPE_REMOVE:
			*boltzmann_factor = (temperature * (N + 1.0)) / (cavity_volume * probability * fugacity * ATM2REDUCED) * std::exp(-delta_energy / temperature) / (double)sorbateCount;
			return MPMC_OK;
		case MPMC_MOVETYPE_DISPLACE:
			*boltzmann_factor = std::exp(-delta_energy / temperature);
			return MPMC_OK;
		default:
			return MPMC_ERR_UNSUPPORTED;
		}
	}
	switch (m->movetype) { // :1391-1420
	case MPMC_MOVETYPE_INSERT:
		*boltzmann_factor = volume * fugacity * ATM2REDUCED / (temperature * (double)(N)) * std::exp(-delta_energy / temperature) * (double)(sorbateCount);
		return MPMC_OK;
	case MPMC_MOVETYPE_REMOVE:
		*boltzmann_factor = temperature * ((double)(N) + 1.0) / (volume * fugacity * ATM2REDUCED) * std::exp(-delta_energy / temperature) / (double)(sorbateCount);
		return MPMC_OK;
	case MPMC_MOVETYPE_DISPLACE:
		*boltzmann_factor = std::exp(-delta_energy / temperature);
		return MPMC_OK;
	default: // (spin flips need the rotational partition functions: quantum rotation is outside the energy path)
		return MPMC_ERR_UNSUPPORTED;
	}
}

// the ENSEMBLE_NPT branch (:1441-1457), operand for operand
extern "C" int mpmc_npt_boltzmann_factor(const mpmc_npt_move *m, double *boltzmann_factor) {
	if (!m || !boltzmann_factor) return MPMC_ERR_ARG;
	constexpr double ATM2REDUCED = 0.0073389366; // src/constants.h
	const double delta_energy = m->final_energy - m->init_energy;
	const double temperature = m->temperature, pressure = m->pressure, N = m->N, v_old = m->volume_old, v_new = m->volume_new;
	switch (m->movetype) {
	case MPMC_MOVETYPE_VOLUME:
		*boltzmann_factor = std::exp(-(delta_energy + pressure * ATM2REDUCED * (v_new - v_old) - (N + 1) * temperature * std::log(v_new / v_old)) / temperature);
		return MPMC_OK;
	case MPMC_MOVETYPE_DISPLACE:
		*boltzmann_factor = std::exp(-delta_energy / temperature);
		return MPMC_OK;
	default:
		return MPMC_ERR_UNSUPPORTED;
	}
}

// ---- the setting --------------------------------------------------------------------------------------------------------------------------
extern "C" int mpmc_set_cavity_grid(mpmc_ctx *c, int grid_size, double radius) {
	if (!c) return MPMC_ERR_ARG;
	if (c->trial.open) return fail(c, MPMC_ERR_ARG, "mpmc_set_cavity_grid: a trial move is open");
	if (grid_size != 0) {
		if (grid_size < 0 || !(radius > 0.0) || !std::isfinite(radius)) // SimulationControl.cpp:2157-2162
			return fail(c, MPMC_ERR_INVALID_SETTING, "mpmc_set_cavity_grid: cavity_bias needs a grid size and a sphere radius greater than zero");
		if (grid_size > MPMC_CAVITY_MAX_GRID)
			return fail(c, MPMC_ERR_INVALID_SETTING, "mpmc_set_cavity_grid: grid size " + std::to_string(grid_size) + " is above MPMC_CAVITY_MAX_GRID (" +
			                                             std::to_string(MPMC_CAVITY_MAX_GRID) + ", 2 M sphere centres)");
	}
	c->kept.cav_grid = grid_size;
	c->kept.cav_radius = grid_size ? radius : 0.0;
	c->cav_valid = false;
	return MPMC_OK;
}

// the last update describes the current grid setting, cell and atom list
static bool cavity_current(const mpmc_ctx *c) {
	return c->cav_valid && c->kept.cav_grid > 0 && c->cav_done_grid == c->kept.cav_grid && c->cav_done_radius == c->kept.cav_radius && c->cav_pos_gen == c->pos_gen &&
	       c->cav_static_gen == c->static_gen;
}

// the sphere centres of the current cell, on the host and on the device (made once per cell and grid size)
static int cavity_grid_ready(mpmc_ctx *c) {
	const int G = c->kept.cav_grid;
	const size_t points = (size_t)G * G * G;
	if (c->cav_grid_G == G && std::memcmp(c->cav_basis, c->box.b, sizeof(c->cav_basis)) == 0 && c->d_cav_grid.cap >= 3 * points) return MPMC_OK;
	c->cav_grid_G = 0;
	c->h_cav_grid.resize(3 * points);
	size_t at = 0;
	for (int i = 0; i < G; i++)
		for (int j = 0; j < G; j++)
			for (int k = 0; k < G; k++, at += 3) (void)mpmc_cavity_grid_point(c->box.b, G, i, j, k, &c->h_cav_grid[at]);
	int rc = c->d_cav_grid.reserve(c, 3 * points);
	if (rc != MPMC_OK) return rc;
	HIP_TRY(c, hipMemcpyAsync(c->d_cav_grid, c->h_cav_grid.data(), 3 * points * sizeof(double), hipMemcpyHostToDevice, c->stream));
	HIP_TRY(c, hipStreamSynchronize(c->stream)); // (pageable source; once per cell)
	std::memcpy(c->cav_basis, c->box.b, sizeof(c->cav_basis));
	c->cav_grid_G = G;
	return MPMC_OK;
}

extern "C" int mpmc_cavity_update(mpmc_ctx *c, int n_darts, const double *dart_frac, mpmc_cavity_result *out) {
	if (!c || !out || n_darts < 0 || (n_darts > 0 && !dart_frac)) return MPMC_ERR_ARG;
	if (c->kept.cav_grid <= 0) return fail(c, MPMC_ERR_ARG, "mpmc_cavity_update: the cavity grid is off (mpmc_set_cavity_grid)");
	if (!c->atoms_set || !c->box_set) return fail(c, MPMC_ERR_ARG, "mpmc_cavity_update: atoms and box must be set");
	if (c->h_mass.empty()) return fail(c, MPMC_ERR_ARG, "mpmc_cavity_update: mpmc_set_atoms was called without masses (the wrapped positions need the centres of mass)");
	if (c->trial.open) return fail(c, MPMC_ERR_ARG, "mpmc_cavity_update: a trial move is open (accept or reject it first)");
	// (every path that moves atoms -- mpmc_update_positions, mpmc_set_positions_device, the bead loops, accepted trials -- brings the host
	// mirror along before it returns: there is no state in which the latest positions live on the device alone)
	HIP_TRY(c, hipSetDevice(c->device));
	const int G = c->kept.cav_grid, n = c->n;
	const long long points = (long long)G * G * G;
	const size_t points_pad = (size_t)((points + 63) / 64) * 64;
	const int slices = cavity_atom_slices(points, n), dart_slices = cavity_dart_slices(points, n_darts);
	const size_t dart_waves = ((size_t)n_darts + 63) / 64;
	const double t2 = mpmc_cavity_r2_threshold(c->kept.cav_radius);
	int rc;
	if ((rc = cavity_grid_ready(c)) != MPMC_OK) return rc;
	const size_t n_in = 3 * ((size_t)n + (size_t)n_darts);
	if ((rc = c->d_cav_in.reserve(c, n_in, n_in + n_in / 4)) != MPMC_OK) return rc;
	if ((rc = c->h_cav_in.reserve(c, n_in, n_in + n_in / 4)) != MPMC_OK) return rc;
	if ((rc = c->d_cav_part.reserve(c, (size_t)slices * points_pad)) != MPMC_OK) return rc;
	if ((rc = c->d_cav_occ.reserve(c, points_pad)) != MPMC_OK) return rc;
	if ((rc = c->d_cav_wave.reserve(c, points_pad / 64)) != MPMC_OK) return rc;
	if ((rc = c->d_cav_open.reserve(c, points_pad)) != MPMC_OK) return rc;
	if ((rc = c->d_cav_mask.reserve(c, (size_t)dart_slices * dart_waves)) != MPMC_OK) return rc;
	if ((rc = c->d_cav_res.reserve(c, 2)) != MPMC_OK) return rc;
	if ((rc = c->h_cav_res.reserve(c, 2)) != MPMC_OK) return rc;
	c->cav_valid = false;

	// the reference's wrapped_pos of every atom, then the darts, in one copy (the pinned block is free: the last update waited for its stream)
	wrap_molecules(c, nullptr, nullptr, c->h_cav_in);
	if (n_darts > 0) std::memcpy(c->h_cav_in + 3 * (size_t)n, dart_frac, 3 * (size_t)n_darts * sizeof(double));
	HIP_TRY(c, hipMemcpyAsync(c->d_cav_in, c->h_cav_in, n_in * sizeof(double), hipMemcpyHostToDevice, c->stream));

	const bool prof = c->kept.prof;
	if (prof)
		for (hipEvent_t &e : c->cav_ev)
			if (!e) HIP_TRY(c, hipEventCreate(&e));
	if (prof) HIP_TRY(c, hipEventRecord(c->cav_ev[0], c->stream));
	launch_cavity_occupancy(c->stream, c->d_cav_grid, (int)points, c->d_cav_in, n, slices, t2, c->d_cav_part);
	if (prof) HIP_TRY(c, hipEventRecord(c->cav_ev[1], c->stream));
	launch_cavity_compact(c->stream, c->d_cav_part, slices, (int)points, c->d_cav_occ, c->d_cav_wave, c->d_cav_open, c->d_cav_res);
	if (prof) HIP_TRY(c, hipEventRecord(c->cav_ev[2], c->stream));
	launch_cavity_darts(c->stream, c->d_cav_grid, c->d_cav_open, c->d_cav_in + 3 * (size_t)n, n_darts, dart_slices, c->box.b, t2, c->d_cav_mask, c->d_cav_res);
	if (prof) HIP_TRY(c, hipEventRecord(c->cav_ev[3], c->stream));
	HIP_TRY(c, hipGetLastError());
	HIP_TRY(c, hipMemcpyAsync(c->h_cav_res, c->d_cav_res, 2 * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	if (prof)
		for (int k = 0; k < 3; k++) HIP_TRY(c, hipEventElapsedTime(&c->cav_ms[k], c->cav_ev[k], c->cav_ev[k + 1]));

	const long long open = c->h_cav_res[0], hits = c->h_cav_res[1];
	if (open < 0 || open > points || hits < 0 || hits > n_darts) return fail(c, MPMC_ERR_INTERNAL, "mpmc_cavity_update: the device returned counts outside their range");
	out->total_points = points;
	out->cavities_open = open;
	out->n_darts = n_darts;
	out->hits = hits;
	out->probability = ((double)open) / ((double)points);                  // update_cavity_probability :112
	const double fraction_hits = ((double)hits) / ((double)n_darts);      // update_cavity_volume :157-158 (0 darts: 0 / 0, as there)
	out->cavity_volume = fraction_hits * c->box.volume;
	c->cav_open = open;
	c->cav_open_cached = false;
	c->cav_done_grid = G;
	c->cav_done_radius = c->kept.cav_radius;
	c->cav_pos_gen = c->pos_gen;
	c->cav_static_gen = c->static_gen;
	c->cav_valid = true;
	return MPMC_OK;
}

// the open list of the last update on the host: one copy per update, at the first request
static int cavity_open_list(mpmc_ctx *c) {
	if (c->cav_open_cached) return MPMC_OK;
	c->h_cav_open.resize((size_t)c->cav_open);
	if (c->cav_open > 0) {
		HIP_TRY(c, hipSetDevice(c->device));
		HIP_TRY(c, hipMemcpyAsync(c->h_cav_open.data(), c->d_cav_open, (size_t)c->cav_open * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
		HIP_TRY(c, hipStreamSynchronize(c->stream));
	}
	c->cav_open_cached = true;
	return MPMC_OK;
}

extern "C" int mpmc_cavity_point(mpmc_ctx *c, int64_t open_rank, double pos[3]) {
	if (!c || !pos) return MPMC_ERR_ARG;
	if (!cavity_current(c)) return fail(c, MPMC_ERR_ARG, "mpmc_cavity_point: no mpmc_cavity_update since the grid, the cell or the atom list last changed");
	if (open_rank < 0 || open_rank >= c->cav_open)
		return fail(c, MPMC_ERR_ARG, "mpmc_cavity_point: rank " + std::to_string((long long)open_rank) + " outside the " + std::to_string((long long)c->cav_open) + " empty points");
	const int rc = cavity_open_list(c);
	if (rc != MPMC_OK) return rc;
	const size_t idx = (size_t)c->h_cav_open[(size_t)open_rank];
	for (int p = 0; p < 3; p++) pos[p] = c->h_cav_grid[3 * idx + p];
	return MPMC_OK;
}

extern "C" int mpmc_cavity_get(mpmc_ctx *c, int32_t *occupancy, double *grid_pos, int32_t *open_flat_index) {
	if (!c) return MPMC_ERR_ARG;
	if (!cavity_current(c)) return fail(c, MPMC_ERR_ARG, "mpmc_cavity_get: no mpmc_cavity_update since the grid, the cell or the atom list last changed");
	const size_t points = (size_t)c->cav_done_grid * c->cav_done_grid * c->cav_done_grid;
	if (occupancy) {
		HIP_TRY(c, hipSetDevice(c->device));
		HIP_TRY(c, hipMemcpyAsync(occupancy, c->d_cav_occ, points * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
		HIP_TRY(c, hipStreamSynchronize(c->stream));
	}
	if (grid_pos) std::memcpy(grid_pos, c->h_cav_grid.data(), 3 * points * sizeof(double));
	if (open_flat_index) {
		const int rc = cavity_open_list(c);
		if (rc != MPMC_OK) return rc;
		if (c->cav_open > 0) std::memcpy(open_flat_index, c->h_cav_open.data(), (size_t)c->cav_open * sizeof(int32_t));
	}
	return MPMC_OK;
}

// (measurement) device time of the three kernel groups of the last update made under mpmc_set_profiling: occupancy, compaction, darts
extern "C" int mpmc_debug_cavity_times(mpmc_ctx *c, double ms3[3]) {
	if (!c || !ms3) return MPMC_ERR_ARG;
	for (int k = 0; k < 3; k++) ms3[k] = (double)c->cav_ms[k];
	return MPMC_OK;
}
