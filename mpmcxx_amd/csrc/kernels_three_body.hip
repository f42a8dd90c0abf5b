// kernels_three_body.hip -- the Axilrod-Teller triple-dipole dispersion, reference System::axilrod_teller (src/System.Energy.cpp:1653-1770).
//
//   E3 = sum over unordered triples {a, b, c} of distinct atoms, not all three in one molecule, no cutoff, frozen atoms included:
//        c9_abc (1 + 3 cos A cos B cos C) / (r_ab r_ac r_bc)^3
// Every pair vector is that pair's own minimum image (min_image_sq, pair_math.h; the three need not close a triangle).  With the vectors
// ab = x_a - x_b, ac = x_a - x_c, bc = x_b - x_c and d = r_ab^2 r_ac^2 r_bc^2 the angular factor is
//   1 + 3 cos A cos B cos C = (d - 3 P) / d,   P = (ab.ac) (ab.bc) (ac.bc)
// (the cosine at b is taken between -ab and bc: its sign enters P once, and every vector appears in two of the three dot products, so the
// orientation of a minimum image never matters).  The mixing rule c9_abc = 3 a_a a_b a_c / (u_a + u_b + u_c) (times the unit factor, applied
// once to the sum) uses per-atom a_i = 6.7483345 alpha_i and u_i = a_i^3 / c9_i, prepared on the host (context.cpp: three_body_coefficients);
// an atom whose term vanishes (alpha = 0, c9 = 0) carries a = 0, u = 1, so a triple costs one division and one square root:
//   e = (a_ab a_c) (d - 3 P) / ((u_ab + u_c) d^2 sqrt(d)).
//
// k_three_body walks unordered triples of the 64-atom tiles of the spatial order, I <= J <= K, one wave per tile triple: lanes own k, the
// (i, k) vector and r^2 stay in registers across the j loop, the (i, j) row of the j-tile (vector, r^2, a_i a_j, u_i + u_j, molecule) is
// computed once per i into LDS and read at a wave-uniform address, the (j, k) vector is recomputed per triple.  Equal tiles keep i < j < k.
// Workgroups take tile triples in a fixed stride and leave one fp64 partial each; k_sum_partials (trial_kernels.h) adds them in a fixed order,
// so repeated evaluations are bit-identical.
//
// k_three_body_delta: the change of E3 under a trial move of m atoms (slots mv_slot, new positions mv_new).  A triple with a moved atom is
// owned by its lowest-slot moved atom a, which pairs with every pair {b, c} of atoms that are neither a nor a moved atom of lower slot;
// every such triple is evaluated in its old and in its new geometry.  One wave per tile pair (B <= C), lanes own c, the (a, b) rows of
// the b-tile in LDS, the (a, c) vectors in registers, (b, c) recomputed: O(m N^2).
#include "kernels.h"
#include "device_math.h"
#include "trial_kernels.h"

namespace mpmc {

__device__ __forceinline__ double dot3(double ax, double ay, double az, double bx_, double by_, double bz_) {
	return ((ax * bx_) + ay * by_) + az * bz_;
}

// one triple's term without the unit factor (see the file header); P and d as defined there
__device__ __forceinline__ double tb_term(double aabc, double usum, double abx, double aby, double abz, double r2ab, double acx, double acy, double acz,
                                          double r2ac, double bcx, double bcy, double bcz, double r2bc) {
	const double p = (dot3(abx, aby, abz, acx, acy, acz) * dot3(abx, aby, abz, bcx, bcy, bcz)) * dot3(acx, acy, acz, bcx, bcy, bcz);
	const double d = (r2ab * r2ac) * r2bc;
	return (aabc * (d - 3.0 * p)) / (((usum * d) * d) * sqrt(d));
}

// tile triple number t -> (I <= J <= K): t = K(K+1)(K+2)/6 + J(J+1)/2 + I
__device__ __forceinline__ void tb_decode_triple(long long t, int &I, int &J, int &K) {
	auto tet = [](long long x) { return x * (x + 1) * (x + 2) / 6; };
	long long k = (long long)cbrt(6.0 * (double)t);
	while (k > 0 && tet(k) > t) --k;
	while (tet(k + 1) <= t) ++k;
	const long long r = t - tet(k);
	long long j = (long long)((sqrt(8.0 * (double)r + 1.0) - 1.0) * 0.5);
	while (j > 0 && j * (j + 1) / 2 > r) --j;
	while ((j + 1) * (j + 2) / 2 <= r) ++j;
	I = (int)(r - j * (j + 1) / 2);
	J = (int)j;
	K = (int)k;
}
// tile pair number p -> (B <= C): p = C(C+1)/2 + B
__device__ __forceinline__ void tb_decode_pair(int p, int &B, int &C) {
	long long c = (long long)((sqrt(8.0 * (double)p + 1.0) - 1.0) * 0.5);
	while (c > 0 && c * (c + 1) / 2 > p) --c;
	while ((c + 1) * (c + 2) / 2 <= p) ++c;
	B = (int)(p - c * (c + 1) / 2);
	C = (int)c;
}

template <bool ORTHO>
__global__ __launch_bounds__(64) void k_three_body(const double4 *__restrict__ xyzq, const int2 *__restrict__ mf, const double2 *__restrict__ au,
                                                   int n, int n_triples, Box bx, double *__restrict__ part) {
	__shared__ double s_x[kTile], s_y[kTile], s_z[kTile];                  // j-tile positions
	__shared__ double s_dx[kTile], s_dy[kTile], s_dz[kTile], s_r2[kTile]; // (i, j) row
	__shared__ double s_a[kTile], s_u[kTile];
	__shared__ int s_mol[kTile];
	const int l = threadIdx.x;
	double acc = 0.0;
	for (int t = blockIdx.x; t < n_triples; t += gridDim.x) {
		int I, J, K;
		tb_decode_triple(t, I, J, K);
		const int k = K * kTile + l, jl = J * kTile + l;
		const bool k_in = k < n;
		const double4 pk = xyzq[k];
		const int mol_k = mf[k].x;
		const double2 au_k = au[k];
		const double4 pj = xyzq[jl];
		const int mol_jl = mf[jl].x;
		const double2 au_jl = au[jl];
		const int ni = min(kTile, n - I * kTile), nj = min(kTile, n - J * kTile);
		__syncthreads(); // (the previous tile triple's readers are done)
		s_x[l] = pj.x, s_y[l] = pj.y, s_z[l] = pj.z;
		s_mol[l] = mol_jl;
		for (int ii = 0; ii < ni; ++ii) {
			const int i = I * kTile + ii;
			const double4 pi = xyzq[i];
			const int mol_i = mf[i].x;
			const double2 au_i = au[i];
			double ikx, iky, ikz, ijx, ijy, ijz;
			const double r2ik = min_image_sq<ORTHO>(bx, pi.x - pk.x, pi.y - pk.y, pi.z - pk.z, ikx, iky, ikz);
			const double r2ij = min_image_sq<ORTHO>(bx, pi.x - pj.x, pi.y - pj.y, pi.z - pj.z, ijx, ijy, ijz);
			__syncthreads();
			s_dx[l] = ijx, s_dy[l] = ijy, s_dz[l] = ijz, s_r2[l] = r2ij;
			s_a[l] = au_i.x * au_jl.x;
			s_u[l] = au_i.y + au_jl.y;
			__syncthreads();
			const bool k_i_same = (mol_k == mol_i);
			for (int jj = (I == J) ? ii + 1 : 0; jj < nj; ++jj) {
				double jkx, jky, jkz;
				const double r2jk = min_image_sq<ORTHO>(bx, s_x[jj] - pk.x, s_y[jj] - pk.y, s_z[jj] - pk.z, jkx, jky, jkz);
				const double e = tb_term(s_a[jj] * au_k.x, s_u[jj] + au_k.y, s_dx[jj], s_dy[jj], s_dz[jj], s_r2[jj], ikx, iky, ikz, r2ik, jkx, jky, jkz, r2jk);
				const bool ok = k_in && (J != K || l > jj) && !(k_i_same && s_mol[jj] == mol_i);
				acc += ok ? e : 0.0;
			}
		}
	}
	acc = wave_sum(acc);
	if (l == 0) part[blockIdx.x] = acc;
}

// trial moves.  moved_idx[slot] = index of the slot in the moved list, -1 for every other slot (k_mark_moved, trial_kernels.h)
template <bool ORTHO>
__global__ __launch_bounds__(64) void k_three_body_delta(const double4 *__restrict__ xyzq, const int2 *__restrict__ mf, const double2 *__restrict__ au,
                                                         int n, int n_tile_pairs, Box bx, const int *__restrict__ mv_slot,
                                                         const double4 *__restrict__ mv_new, int m, const int *__restrict__ moved_idx,
                                                         double *__restrict__ part) {
	__shared__ double s_ox[kTile], s_oy[kTile], s_oz[kTile], s_nx[kTile], s_ny[kTile], s_nz[kTile]; // b-tile, old / new positions
	__shared__ double s_a[kTile], s_u[kTile];
	__shared__ int s_mol[kTile], s_mv[kTile], s_ok[kTile];
	__shared__ double s_odx[kTile], s_ody[kTile], s_odz[kTile], s_or2[kTile]; // (a, b) rows, old geometry
	__shared__ double s_ndx[kTile], s_ndy[kTile], s_ndz[kTile], s_nr2[kTile]; // new geometry
	const int l = threadIdx.x;
	double acc = 0.0;
	for (int p = blockIdx.x; p < n_tile_pairs; p += gridDim.x) {
		int B, C;
		tb_decode_pair(p, B, C);
		const int c = C * kTile + l, bl = B * kTile + l;
		const bool c_in = c < n, b_in = bl < n;
		const double4 pco = xyzq[c];
		const int mv_c = c_in ? moved_idx[c] : -1;
		const double4 pcn = (mv_c >= 0) ? mv_new[mv_c] : pco;
		const int mol_c = mf[c].x;
		const double2 au_c = au[c];
		const double4 pbo = xyzq[bl];
		const int mv_b = b_in ? moved_idx[bl] : -1;
		const double4 pbn = (mv_b >= 0) ? mv_new[mv_b] : pbo;
		const int nb = min(kTile, n - B * kTile);
		__syncthreads();
		s_ox[l] = pbo.x, s_oy[l] = pbo.y, s_oz[l] = pbo.z;
		s_nx[l] = pbn.x, s_ny[l] = pbn.y, s_nz[l] = pbn.z;
		s_a[l] = au[bl].x;
		s_u[l] = au[bl].y;
		s_mol[l] = mf[bl].x;
		s_mv[l] = mv_b;
		for (int t = 0; t < m; ++t) {
			const int sa = mv_slot[t];
			const double4 pao = xyzq[sa], pan = mv_new[t];
			const int mol_a = mf[sa].x;
			const double2 au_a = au[sa];
			// partners of a: neither a nor a moved atom of lower slot
			const bool c_ok = c_in && (mv_c < 0 || c > sa);
			double acox, acoy, acoz, acnx, acny, acnz, abox, aboy, aboz, abnx, abny, abnz;
			const double r2aco = min_image_sq<ORTHO>(bx, pao.x - pco.x, pao.y - pco.y, pao.z - pco.z, acox, acoy, acoz);
			const double r2acn = min_image_sq<ORTHO>(bx, pan.x - pcn.x, pan.y - pcn.y, pan.z - pcn.z, acnx, acny, acnz);
			const double r2abo = min_image_sq<ORTHO>(bx, pao.x - pbo.x, pao.y - pbo.y, pao.z - pbo.z, abox, aboy, aboz);
			const double r2abn = min_image_sq<ORTHO>(bx, pan.x - pbn.x, pan.y - pbn.y, pan.z - pbn.z, abnx, abny, abnz);
			__syncthreads();
			s_odx[l] = abox, s_ody[l] = aboy, s_odz[l] = aboz, s_or2[l] = r2abo;
			s_ndx[l] = abnx, s_ndy[l] = abny, s_ndz[l] = abnz, s_nr2[l] = r2abn;
			s_ok[l] = b_in && (mv_b < 0 || bl > sa);
			__syncthreads();
			const double a_ac = au_a.x * au_c.x, u_ac = au_a.y + au_c.y;
			const bool c_a_same = (mol_c == mol_a);
			for (int bb = 0; bb < nb; ++bb) {
				if (!s_ok[bb]) continue; // (wave-uniform)
				double bcox, bcoy, bcoz, bcnx, bcny, bcnz;
				const double r2bco = min_image_sq<ORTHO>(bx, s_ox[bb] - pco.x, s_oy[bb] - pco.y, s_oz[bb] - pco.z, bcox, bcoy, bcoz);
				const double r2bcn = min_image_sq<ORTHO>(bx, s_nx[bb] - pcn.x, s_ny[bb] - pcn.y, s_nz[bb] - pcn.z, bcnx, bcny, bcnz);
				const double aabc = a_ac * s_a[bb], usum = u_ac + s_u[bb];
				const double e_old = tb_term(aabc, usum, s_odx[bb], s_ody[bb], s_odz[bb], s_or2[bb], acox, acoy, acoz, r2aco, bcox, bcoy, bcoz, r2bco);
				const double e_new = tb_term(aabc, usum, s_ndx[bb], s_ndy[bb], s_ndz[bb], s_nr2[bb], acnx, acny, acnz, r2acn, bcnx, bcny, bcnz, r2bcn);
				const bool ok = c_ok && (B != C || l > bb) && !(c_a_same && s_mol[bb] == mol_a);
				acc += ok ? (e_new - e_old) : 0.0;
			}
		}
	}
	acc = wave_sum(acc);
	if (l == 0) part[blockIdx.x] = acc;
}

long long three_body_tile_triples(int n_tiles) { return (long long)n_tiles * (n_tiles + 1) * (n_tiles + 2) / 6; }
int three_body_grid(long long work_items) { return (int)std::min<long long>(work_items, kThreeBodyBlocks); }

void launch_three_body(hipStream_t st, const AtomsDev &at, const double2 *au, const Box &bx, double scale, double *part, double *out) {
	const int nt3 = (int)three_body_tile_triples(at.n_pad / kTile); // (mpmc_set_axilrod_teller refuses boxes beyond INT_MAX tile triples)
	const int grid = three_body_grid(nt3);
	with_flag(bx.ortho, [&](auto O) { hipLaunchKernelGGL(k_three_body<O.value>, dim3(grid), dim3(kTile), 0, st, at.xyzq, at.mf, au, at.n, nt3, bx, part); });
	launch_sum_partials(st, part, 0, grid, 1, out, 1, scale);
}

void launch_three_body_delta(hipStream_t st, const AtomsDev &at, const double2 *au, const Box &bx, double scale, const int *mv_slot, const double4 *mv_new,
                             int m, int *moved_idx, double *part, double *out) {
	const int nt = at.n_pad / kTile;
	const int ntp = nt * (nt + 1) / 2;
	const int grid = three_body_grid(ntp);
	launch_mark_moved(st, moved_idx, mv_slot, m, 1);
	with_flag(bx.ortho, [&](auto O) {
		hipLaunchKernelGGL(k_three_body_delta<O.value>, dim3(grid), dim3(kTile), 0, st, at.xyzq, at.mf, au, at.n, ntp, bx, mv_slot, mv_new, m, moved_idx, part);
	});
	launch_sum_partials(st, part, 0, grid, 1, out, 1, scale, 0, 0.0, 0.0, moved_idx, mv_slot, m); // (clears the map)
}

} // namespace mpmc
