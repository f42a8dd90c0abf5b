// kernels_cavity.hip -- the cavity-bias grid of uVT moves: System::cavity_update_grid (reference src/System.Cavity.cpp:15-188).
//
// In front of every move of a `cavity_bias on` run the reference bins every atom against a G x G x G grid of sphere centres, counts the
// spheres that hold no atom, and estimates their joint volume by throwing darts at them.  Three kernel groups, all on the context's stream:
//   k_cavity_occupancy        lanes own sphere centres (registers), a slice of the atom list streams through LDS at wave-uniform addresses;
//                             one int per (slice, centre)
//   k_cavity_compact_*        the slices summed into the occupancy, the empty centres counted per wave by ballot / popcount, one fixed-order
//                             scan across the waves, then each wave writes its empty centres' flat indices behind its prefix: the list comes
//                             out in the reference's enumeration order (i outermost, k innermost) whatever the launch does
//   k_cavity_darts (+ _sum)   lanes own darts, a slice of the empty centres streams through LDS; a wave leaves once every lane has a hit; one
//                             64-bit hit mask per (slice, wave), OR-ed over the slices and popcounted
// Arithmetic (csrc is compiled with -ffp-contract=off): r = ((dx dx) + dy dy) + dz dz with d = centre - atom, respectively dart - centre, as
// the reference writes them; "inside" is r < t2 with t2 the smallest double whose correctly rounded square root reaches the radius
// (mpmc_cavity_r2_threshold), which decides exactly as sqrt(r) < radius does.  No minimum image: the reference uses none.  Every result is an
// integer, so nothing depends on the order in which slices or waves finish.
#include "kernels.h"
#include "device_math.h"

namespace mpmc {

struct CavityBasis {
	double b[9]; // pbc.basis[q][p], row-major
};

// block = one wave = 64 sphere centres (blockIdx.x) x one slice of the atoms (blockIdx.y)
__global__ __launch_bounds__(64) void k_cavity_occupancy(const double *__restrict__ grid, int points, int points_pad, const double *__restrict__ atoms, int n,
                                                         int per_slice, double t2, int *__restrict__ part) {
	__shared__ double s_at[3 * kCavityChunk];
	const int lane = threadIdx.x;
	const int p = blockIdx.x * 64 + lane;
	const size_t pc = (size_t)(p < points ? p : points - 1); // (the lanes past the last centre repeat it; the compaction never reads their count)
	const double gx = grid[3 * pc], gy = grid[3 * pc + 1], gz = grid[3 * pc + 2];
	const int a0 = blockIdx.y * per_slice, a1 = min(n, a0 + per_slice);
	int cnt = 0;
	for (int base = a0; base < a1; base += kCavityChunk) {
		const int m = min(kCavityChunk, a1 - base);
		__syncthreads();
		for (int t = lane; t < 3 * m; t += 64) s_at[t] = atoms[3 * (size_t)base + t];
		__syncthreads();
#pragma unroll 4
		for (int a = 0; a < m; ++a) {
			const double dx = gx - s_at[3 * a], dy = gy - s_at[3 * a + 1], dz = gz - s_at[3 * a + 2];
			const double r = ((dx * dx) + dy * dy) + dz * dz;
			cnt += (r < t2) ? 1 : 0;
		}
	}
	part[(size_t)blockIdx.y * points_pad + p] = cnt;
}

// occupancy = sum of the slices; empty centres per wave
__global__ __launch_bounds__(64) void k_cavity_compact_count(const int *__restrict__ part, int slices, int points, int points_pad, int *__restrict__ occ,
                                                             int *__restrict__ wave_cnt) {
	const int p = blockIdx.x * 64 + threadIdx.x;
	int o = 0;
	for (int s = 0; s < slices; ++s) o += part[(size_t)s * points_pad + p];
	occ[p] = o;
	const unsigned long long empty = __ballot(p < points && o == 0);
	if (threadIdx.x == 0) wave_cnt[blockIdx.x] = __popcll(empty);
}

// ONE block: wave_cnt[w] becomes the number of empty centres in front of wave w; res[0] = cavities_open
__global__ __launch_bounds__(1024) void k_cavity_compact_scan(int *__restrict__ wave_cnt, int waves, long long *__restrict__ res) {
	__shared__ int s_tot[16];
	const int t = threadIdx.x, lane = t & 63, w = t >> 6;
	const int per = (waves + 1023) / 1024;
	const int i0 = min(waves, t * per), i1 = min(waves, i0 + per);
	int sum = 0;
	for (int i = i0; i < i1; ++i) sum += wave_cnt[i];
	int inc = sum;
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const int v = __shfl_up(inc, d, 64);
		if (lane >= d) inc += v;
	}
	if (lane == 63) s_tot[w] = inc;
	__syncthreads();
	int before = 0;
	for (int k = 0; k < w; ++k) before += s_tot[k];
	int run = before + inc - sum;
	for (int i = i0; i < i1; ++i) {
		const int c = wave_cnt[i];
		wave_cnt[i] = run;
		run += c;
	}
	if (t == 1023) res[0] = (long long)(before + inc);
}

// every wave writes the flat indices of its empty centres behind its prefix
__global__ __launch_bounds__(64) void k_cavity_compact_scatter(const int *__restrict__ occ, const int *__restrict__ wave_off, int points, int *__restrict__ open) {
	const int lane = threadIdx.x;
	const int p = blockIdx.x * 64 + lane;
	const bool empty = p < points && occ[p] == 0;
	const unsigned long long m = __ballot(empty);
	const int rank = __popcll(m & ((1ull << lane) - 1ull));
	if (empty) open[wave_off[blockIdx.x] + rank] = p;
}

// block = one wave = 64 darts (blockIdx.x) x one slice of the empty centres (blockIdx.y)
__global__ __launch_bounds__(64) void k_cavity_darts(const double *__restrict__ grid, const int *__restrict__ open, const long long *__restrict__ res,
                                                     const double *__restrict__ frac, int n_darts, int slices, CavityBasis bs, double t2,
                                                     unsigned long long *__restrict__ mask) {
	__shared__ double s_g[3 * kCavityChunk];
	const int lane = threadIdx.x;
	const int d = blockIdx.x * 64 + lane;
	const size_t dc = (size_t)(d < n_darts ? d : n_darts - 1);
	const double f[3] = {frac[3 * dc], frac[3 * dc + 1], frac[3 * dc + 2]};
	double pos[3];
	for (int p = 0; p < 3; ++p) { // (update_cavity_volume :142-148)
		pos[p] = 0;
		for (int q = 0; q < 3; ++q) pos[p] += bs.b[3 * q + p] * f[q];
	}
	const int n_open = (int)res[0];
	const int chunks = (n_open + kCavityChunk - 1) / kCavityChunk, per = (chunks + slices - 1) / slices;
	const int c0 = blockIdx.y * per, c1 = min(chunks, c0 + per);
	int hit = 0;
	bool done = false;
	for (int ch = c0; ch < c1 && !done; ++ch) {
		const int base = ch * kCavityChunk, m = min(kCavityChunk, n_open - base);
		__syncthreads();
		for (int t = lane; t < m; t += 64) {
			const size_t g = 3 * (size_t)open[base + t];
			s_g[3 * t] = grid[g], s_g[3 * t + 1] = grid[g + 1], s_g[3 * t + 2] = grid[g + 2];
		}
		__syncthreads();
		for (int a0 = 0; a0 < m && !done; a0 += 64) {
			const int a1 = min(m, a0 + 64);
#pragma unroll 4
			for (int a = a0; a < a1; ++a) {
				const double dx = pos[0] - s_g[3 * a], dy = pos[1] - s_g[3 * a + 1], dz = pos[2] - s_g[3 * a + 2];
				const double r = ((dx * dx) + dy * dy) + dz * dz;
				hit |= (r < t2) ? 1 : 0;
			}
			done = __ballot(!hit && d < n_darts) == 0ull; // wave-uniform: every dart of this wave is inside some empty sphere
		}
	}
	const unsigned long long mk = __ballot(hit && d < n_darts);
	if (lane == 0) mask[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = mk;
}

// ONE block: res[1] = darts with a hit in any slice
__global__ __launch_bounds__(256) void k_cavity_darts_sum(const unsigned long long *__restrict__ mask, int slices, int dart_waves, long long *__restrict__ res) {
	__shared__ int s_cnt[4];
	int cnt = 0;
	for (int b = threadIdx.x; b < dart_waves; b += 256) {
		unsigned long long m = 0ull;
		for (int s = 0; s < slices; ++s) m |= mask[(size_t)s * dart_waves + b];
		cnt += __popcll(m);
	}
	cnt = wave_sum_i(cnt);
	if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = cnt;
	__syncthreads();
	if (threadIdx.x == 0) res[1] = (long long)(((s_cnt[0] + s_cnt[1]) + s_cnt[2]) + s_cnt[3]);
}

void launch_cavity_occupancy(hipStream_t st, const double *grid, int points, const double *atoms, int n, int slices, double t2, int *part) {
	const int blocks = (points + 63) / 64;
	const int per_slice = (n + slices - 1) / slices;
	hipLaunchKernelGGL(k_cavity_occupancy, dim3(blocks, slices), dim3(64), 0, st, grid, points, blocks * 64, atoms, n, per_slice, t2, part);
}

void launch_cavity_compact(hipStream_t st, const int *part, int slices, int points, int *occ, int *wave_cnt, int *open, long long *res) {
	const int blocks = (points + 63) / 64;
	hipLaunchKernelGGL(k_cavity_compact_count, dim3(blocks), dim3(64), 0, st, part, slices, points, blocks * 64, occ, wave_cnt);
	hipLaunchKernelGGL(k_cavity_compact_scan, dim3(1), dim3(1024), 0, st, wave_cnt, blocks, res);
	hipLaunchKernelGGL(k_cavity_compact_scatter, dim3(blocks), dim3(64), 0, st, occ, wave_cnt, points, open);
}

void launch_cavity_darts(hipStream_t st, const double *grid, const int *open, const double *dart_frac, int n_darts, int slices, const double basis[9], double t2,
                         unsigned long long *mask, long long *res) {
	const int dart_waves = (n_darts + 63) / 64;
	if (n_darts > 0) {
		CavityBasis bs;
		for (int k = 0; k < 9; ++k) bs.b[k] = basis[k];
		hipLaunchKernelGGL(k_cavity_darts, dim3(dart_waves, slices), dim3(64), 0, st, grid, open, res, dart_frac, n_darts, slices, bs, t2, mask);
	}
	hipLaunchKernelGGL(k_cavity_darts_sum, dim3(1), dim3(256), 0, st, mask, slices, dart_waves, res);
}

} // namespace mpmc
