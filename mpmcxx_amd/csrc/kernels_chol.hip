// kernels_chol.hip -- the exact dipole solve of `polar_iterative off` (System::polar, src/System.Energy.cpp:2590-2607: thole_field,
// thole_bmatrix, thole_bmatrix_dipoles): A mu = E0 solved directly on the device.  A (thole_amatrix :2661-2781: 1/alpha on the diagonal,
// the exponentially damped dipole tensor off it, all pairs, minimum image, no cutoff) is symmetric and, for a physical model, positive
// definite, so it is factored as L L^T instead of the reference's pivoted LU with an explicit inverse.
//
// Layout: the unknowns are the 3 n_pol components of the POLARIZABLE atoms (alpha != 0) in slot order; atoms with alpha == 0 (diagonal
// 1e40 in the reference, dipoles of the order 1e-40 E) are left out and get mu = 0.  The matrix is row-major, ld = np = 3 n_pol rounded up
// to kCholPanel (padding: unit diagonal, zero off it); only the lower triangle is built, read and overwritten by L.
//
//   k_chol_index    slot list of the polarizable atoms (one workgroup, ballot prefix: ascending slot order)
//   k_chol_build    lower triangle of A, one thread per 3 x 3 block (the pair geometry exactly as k_dense_build computes it)
//   blocked right-looking Cholesky, two levels: block width kCholNB = 64, panel width kCholPanel = 192.  Per 64-column block:
//     k_chol_potrf   the 64 x 64 diagonal block, one workgroup, in LDS;
//     k_chol_trsm    the 64-row blocks under it: X L^T = B, one row per thread;
//     k_chol_update  C(i, j) -= P_i P_j^T on v_mfma_f64_16x16x4_f64, operand tiles staged in LDS: inside the panel after every block
//                    (rank 64, the panel's remaining columns only), behind the panel once (rank 192, the whole trailing matrix: this
//                    is where the n^3 / 3 flops are).
//   k_chol_fwd / k_chol_bwd   the two triangular solves for the one right-hand side, one launch per 64-row block
//   k_chol_rhs / k_chol_scatter / k_chol_finish   E0 in, mu out, residual + status + ef_induced
// Every sum has a fixed order: two evaluations of one configuration give the same bits.
// A non-positive pivot (A not positive definite: polarization catastrophe) is recorded in status[0] (1-based index of the unknown); every
// later kernel of the solve returns at once, the dipoles are zeroed.  Nothing faults.
#include "kernels.h"
#include "device_math.h"

namespace mpmc {

typedef double v4f64c __attribute__((ext_vector_type(4)));
constexpr int NB = kCholNB;
constexpr int LDT = NB + 1; // LDS row stride of a 64 x 64 tile

__global__ __launch_bounds__(1024) void k_chol_index(AtomsDev at, int *__restrict__ pol_list) {
	__shared__ int s_w[16];
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	int base = 0;
	for (int c0 = 0; c0 < at.n; c0 += 1024) {
		const int i = c0 + threadIdx.x;
		const bool f = (i < at.n) && (at.alpha[i] != 0.0) && !(at.mf[i].y & AF_PAD);
		const unsigned long long b = __ballot(f);
		const int pre = __popcll(b & ((1ull << lane) - 1ull));
		__syncthreads(); // (the sums of the chunk before are read)
		if (lane == 0) s_w[w] = __popcll(b);
		__syncthreads();
		int off = 0, total = 0;
		for (int k = 0; k < 16; ++k) {
			if (k < w) off += s_w[k];
			total += s_w[k];
		}
		if (f) pol_list[base + off + pre] = i;
		base += total;
	}
}

template <bool ORTHO>
__global__ __launch_bounds__(256) void k_chol_build(AtomsDev at, Box bx, double lambda, const int *__restrict__ pol_list, int n_pol, int na_pad,
                                                    double *__restrict__ m, int ld) {
	const int pj = blockIdx.x * 256 + threadIdx.x; // column atom (index into the list)
	const int pi = blockIdx.y;                     // row atom
	if (pj >= na_pad || pj > pi) return;
	double v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
	if (pi == pj) {
		const double d = (pi < n_pol) ? 1.0 / at.alpha[pol_list[pi]] : 1.0;
		v[0] = v[4] = v[8] = d;
	} else if (pi < n_pol) {
		const int si = pol_list[pi], sj = pol_list[pj];
		const int lo = min(si, sj), hi = max(si, sj);
		const double4 pl = at.xyzq[lo], ph = at.xyzq[hi];
		double d[3];
		const double r = min_image<ORTHO>(bx, pl.x - ph.x, pl.y - ph.y, pl.z - ph.z, d[0], d[1], d[2]);
		double ta, tb;
		thole_ab(r, lambda, ta, tb);
		for (int p = 0; p < 3; ++p)
			for (int q = 0; q < 3; ++q) v[3 * p + q] = ((p == q) ? ta : 0.0) - tb * d[p] * d[q];
	}
	double *blk = m + (3 * (size_t)pi) * ld + 3 * (size_t)pj;
	for (int p = 0; p < 3; ++p)
		for (int q = 0; q < 3; ++q) blk[(size_t)p * ld + q] = v[3 * p + q];
}

// the diagonal block at offset o: unblocked right-looking Cholesky in LDS (lower triangle in, L out)
__global__ __launch_bounds__(256) void k_chol_potrf(double *__restrict__ m, int ld, int o, int *__restrict__ status) {
	__shared__ double s[NB * LDT];
	if (status[0] != 0) return;
	for (int e = threadIdx.x; e < NB * NB; e += 256) {
		const int r = e >> 6, c = e & 63;
		s[r * LDT + c] = (c <= r) ? m[(size_t)(o + r) * ld + o + c] : 0.0;
	}
	__syncthreads();
	for (int j = 0; j < NB; ++j) {
		double d = s[j * LDT + j];
		if (!(d > 0.0)) { // not positive definite (or not a number): the first such pivot is the status; carry on with a finite block
			if (threadIdx.x == 0 && status[0] == 0) status[0] = o + j + 1;
			d = 1.0;
		}
		const double ljj = sqrt(d);
		__syncthreads();
		if (threadIdx.x < NB) {
			const int r = threadIdx.x;
			if (r == j) s[j * LDT + j] = ljj;
			else if (r > j) s[r * LDT + j] = s[r * LDT + j] / ljj;
		}
		__syncthreads();
		for (int e = threadIdx.x; e < NB * NB; e += 256) {
			const int r = e >> 6, c = e & 63;
			if (c > j && r >= c) s[r * LDT + c] -= s[r * LDT + j] * s[c * LDT + j];
		}
		__syncthreads();
	}
	for (int e = threadIdx.x; e < NB * NB; e += 256) {
		const int r = e >> 6, c = e & 63;
		if (c <= r) m[(size_t)(o + r) * ld + o + c] = s[r * LDT + c];
	}
}

// the 64-row blocks under the diagonal block at o: X L^T = B in place; workgroup = one block of rows, thread = one row
__global__ __launch_bounds__(64) void k_chol_trsm(double *__restrict__ m, int ld, int o, const int *__restrict__ status) {
	__shared__ double sl[NB * LDT], sx[NB * LDT];
	if (status[0] != 0) return;
	const int t = threadIdx.x;
	const size_t r0 = (size_t)o + (size_t)NB * (blockIdx.x + 1);
	for (int r = 0; r < NB; ++r) {
		sl[r * LDT + t] = (t <= r) ? m[(size_t)(o + r) * ld + o + t] : 0.0;
		sx[r * LDT + t] = m[(r0 + r) * ld + o + t];
	}
	__syncthreads();
	for (int c = 0; c < NB; ++c) {
		double acc = sx[t * LDT + c];
		for (int j = 0; j < c; ++j) acc -= sx[t * LDT + j] * sl[c * LDT + j];
		sx[t * LDT + c] = acc / sl[c * LDT + c];
	}
	__syncthreads();
	for (int r = 0; r < NB; ++r) m[(r0 + r) * ld + o + t] = sx[r * LDT + t];
}

// C(ib, jb) -= sum over the kw columns from k0 of M[ib rows][k] M[jb rows][k], for the 64 x 64 tiles jb in [jb0, jb0 + gridDim.x),
// ib in [jb0, jb0 + gridDim.y), ib >= jb.  Four waves; wave w owns rows 16 w .. 16 w + 15 of the tile and all 64 columns (four
// accumulators).  v_mfma_f64_16x16x4_f64: A operand lane l = A[row l & 15][k = l >> 4], B operand lane l = B[k = l >> 4][col l & 15],
// result register g of lane l = D[row (l >> 4) + 4 g][col l & 15].  With B = P_j^T both operands are read as P[row l & 15][k0 + (l >> 4)].
__global__ __launch_bounds__(256) void k_chol_update(double *__restrict__ m, int ld, int k0, int kw, int jb0, const int *__restrict__ status) {
	__shared__ double sa[NB * LDT], sb[NB * LDT];
	const int jb = jb0 + blockIdx.x, ib = jb0 + blockIdx.y;
	if (ib < jb) return;
	if (status[0] != 0) return;
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	const int l15 = lane & 15, l4 = lane >> 4;
	v4f64c acc[4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
	const double *pa = m + (size_t)ib * NB * ld, *pb = m + (size_t)jb * NB * ld;
	for (int kc = k0; kc < k0 + kw; kc += NB) {
		if (kc != k0) __syncthreads();
		for (int e = threadIdx.x; e < NB * NB; e += 256) {
			const int r = e >> 6, c = e & 63;
			sa[r * LDT + c] = pa[(size_t)r * ld + kc + c];
			sb[r * LDT + c] = pb[(size_t)r * ld + kc + c];
		}
		__syncthreads();
#pragma unroll 4
		for (int ks = 0; ks < NB / 4; ++ks) {
			const double a = sa[(16 * w + l15) * LDT + 4 * ks + l4];
#pragma unroll
			for (int t = 0; t < 4; ++t) {
				const double b = sb[(16 * t + l15) * LDT + 4 * ks + l4];
				acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[t], 0, 0, 0);
			}
		}
	}
	double *pc = m + ((size_t)ib * NB + 16 * w + l4) * ld + (size_t)jb * NB + l15;
#pragma unroll
	for (int t = 0; t < 4; ++t)
#pragma unroll
		for (int g = 0; g < 4; ++g) {
			double *q = pc + (size_t)(4 * g) * ld + 16 * t;
			*q = *q - acc[t][g];
		}
}

// forward substitution, block kb: every workgroup solves L_kk y_k = b_k for itself (same bits in each); workgroup 0 writes y_k, workgroup
// g > 0 takes L[kb + g][kb] y_k off its rows of b.  b_k itself is read only (y goes to its own vector: no workgroup races another's read).
__global__ __launch_bounds__(64) void k_chol_fwd(const double *__restrict__ m, int ld, int kb, double *__restrict__ b, double *__restrict__ y,
                                                 const int *__restrict__ status) {
	__shared__ double sl[NB * LDT], sy[NB];
	if (status[0] != 0) return;
	const int t = threadIdx.x, o = kb * NB;
	for (int r = 0; r < NB; ++r) sl[r * LDT + t] = (t <= r) ? m[(size_t)(o + r) * ld + o + t] : 0.0;
	sy[t] = b[o + t];
	__syncthreads();
	for (int c = 0; c < NB; ++c) {
		if (t == c) sy[c] = sy[c] / sl[c * LDT + c];
		__syncthreads();
		if (t > c) sy[t] -= sl[t * LDT + c] * sy[c];
		__syncthreads();
	}
	if (blockIdx.x == 0) {
		y[o + t] = sy[t];
		return;
	}
	const size_t r0 = (size_t)(kb + blockIdx.x) * NB;
	for (int r = 0; r < NB; ++r) sl[r * LDT + t] = m[(r0 + r) * ld + o + t];
	__syncthreads();
	double acc = 0.0;
	for (int c = 0; c < NB; ++c) acc += sl[t * LDT + c] * sy[c];
	b[r0 + t] -= acc;
}

// backward substitution, block kb: L_kk^T x_k = y_k in every workgroup; workgroup kb writes x_k, workgroup i < kb takes L[kb][i]^T x_k off y_i
__global__ __launch_bounds__(64) void k_chol_bwd(const double *__restrict__ m, int ld, int kb, double *__restrict__ y, double *__restrict__ x,
                                                 const int *__restrict__ status) {
	__shared__ double sl[NB * LDT], sx[NB];
	if (status[0] != 0) return;
	const int t = threadIdx.x, o = kb * NB;
	for (int r = 0; r < NB; ++r) sl[r * LDT + t] = (t <= r) ? m[(size_t)(o + r) * ld + o + t] : 0.0;
	sx[t] = y[o + t];
	__syncthreads();
	for (int c = NB - 1; c >= 0; --c) {
		if (t == c) sx[c] = sx[c] / sl[c * LDT + c];
		__syncthreads();
		if (t < c) sx[t] -= sl[c * LDT + t] * sx[c];
		__syncthreads();
	}
	const int i = blockIdx.x;
	if (i == kb) {
		x[o + t] = sx[t];
		return;
	}
	double acc = 0.0;
	for (int r = 0; r < NB; ++r) acc += m[(size_t)(o + r) * ld + (size_t)i * NB + t] * sx[r];
	y[(size_t)i * NB + t] -= acc;
}

__global__ __launch_bounds__(256) void k_chol_rhs(const int *__restrict__ pol_list, int n_pol, int np, const double *__restrict__ e_static,
                                                  double *__restrict__ b, int *__restrict__ status) {
	const int u = blockIdx.x * 256 + threadIdx.x;
	if (u == 0) status[0] = 0;
	if (u >= np) return;
	const int k = u / 3;
	b[u] = (k < n_pol) ? e_static[3 * (size_t)pol_list[k] + (u - 3 * k)] : 0.0;
}

// mu (zeroed in front of this launch) of the polarizable atoms; zeros stay when the factorisation failed
__global__ __launch_bounds__(256) void k_chol_scatter(const int *__restrict__ pol_list, int n_pol, const double *__restrict__ x, double *__restrict__ mu,
                                                      const int *__restrict__ status) {
	const int u = blockIdx.x * 256 + threadIdx.x;
	if (u >= 3 * n_pol || status[0] != 0) return;
	const int k = u / 3;
	mu[3 * (size_t)pol_list[k] + (u - 3 * k)] = x[u];
}

// residual of the solve from an independent product: e_induced holds -(A_off mu) of one matrix-free contraction (k_dipole_update), so
// r = E0 - A mu = E0 + e_induced - mu / alpha.  info = { status, max |r|, max |E0| } over the unknowns; afterwards e_induced is set to what
// the converged iteration leaves there: mu / alpha - E0 for polarizable atoms, 0 for the others (and for everybody after a failed solve).
__global__ __launch_bounds__(256) void k_chol_finish(AtomsDev at, const double *__restrict__ mu, const double *__restrict__ e_static,
                                                     double *__restrict__ e_induced, const int *__restrict__ status, double *__restrict__ info) {
	__shared__ double s_r[256], s_e[256];
	const int failed = status[0];
	double mr = 0.0, me = 0.0;
	for (int i = threadIdx.x; i < at.n_pad; i += 256) {
		const double al = at.alpha[i];
		const bool live = (i < at.n) && (al != 0.0) && !failed;
		for (int p = 0; p < 3; ++p) {
			const size_t q = 3 * (size_t)i + p;
			double out = 0.0;
			if (live) {
				const double e0 = e_static[q], ma = mu[q] / al;
				mr = fmax(mr, fabs((e0 + e_induced[q]) - ma));
				me = fmax(me, fabs(e0));
				out = ma - e0;
			}
			e_induced[q] = out;
		}
	}
	s_r[threadIdx.x] = mr;
	s_e[threadIdx.x] = me;
	__syncthreads();
	for (int s = 128; s > 0; s >>= 1) {
		if (threadIdx.x < s) {
			s_r[threadIdx.x] = fmax(s_r[threadIdx.x], s_r[threadIdx.x + s]);
			s_e[threadIdx.x] = fmax(s_e[threadIdx.x], s_e[threadIdx.x + s]);
		}
		__syncthreads();
	}
	if (threadIdx.x == 0) {
		info[0] = (double)failed;
		info[1] = s_r[0];
		info[2] = s_e[0];
	}
}

// ---- launchers -----------------------------------------------------------------------------------------------------------------
void launch_chol_build(hipStream_t st, const AtomsDev &at, const Box &bx, double polar_damp, int *pol_list, int n_pol, int np, double *m) {
	hipLaunchKernelGGL(k_chol_index, dim3(1), dim3(1024), 0, st, at, pol_list);
	const int na_pad = np / 3;
	dim3 grid((na_pad + 255) / 256, na_pad), block(256);
	if (bx.ortho) hipLaunchKernelGGL(k_chol_build<true>, grid, block, 0, st, at, bx, polar_damp, pol_list, n_pol, na_pad, m, np);
	else hipLaunchKernelGGL(k_chol_build<false>, grid, block, 0, st, at, bx, polar_damp, pol_list, n_pol, na_pad, m, np);
}

void launch_chol_factor(hipStream_t st, double *m, int np, int *status) {
	const int nb = np / NB, bpp = kCholPanel / NB; // blocks, blocks per panel
	for (int p0 = 0; p0 < nb; p0 += bpp) {
		const int pe = p0 + bpp; // (np is a multiple of the panel width)
		for (int kb = p0; kb < pe; ++kb) {
			hipLaunchKernelGGL(k_chol_potrf, dim3(1), dim3(256), 0, st, m, np, kb * NB, status);
			if (kb + 1 < nb) hipLaunchKernelGGL(k_chol_trsm, dim3(nb - kb - 1), dim3(64), 0, st, m, np, kb * NB, status);
			if (kb + 1 < pe) // the panel's remaining columns, all rows under them
				hipLaunchKernelGGL(k_chol_update, dim3(pe - kb - 1, nb - kb - 1), dim3(256), 0, st, m, np, kb * NB, NB, kb + 1, status);
		}
		if (pe < nb) hipLaunchKernelGGL(k_chol_update, dim3(nb - pe, nb - pe), dim3(256), 0, st, m, np, p0 * NB, kCholPanel, pe, status);
	}
}

void launch_chol_solve(hipStream_t st, const double *m, int np, double *v0, double *v1, const int *status) {
	const int nb = np / NB;
	for (int kb = 0; kb < nb; ++kb) hipLaunchKernelGGL(k_chol_fwd, dim3(nb - kb), dim3(64), 0, st, m, np, kb, v0, v1, status);
	for (int kb = nb - 1; kb >= 0; --kb) hipLaunchKernelGGL(k_chol_bwd, dim3(kb + 1), dim3(64), 0, st, m, np, kb, v1, v0, status);
}

void launch_chol_rhs(hipStream_t st, const int *pol_list, int n_pol, int np, const double *e_static, double *b, int *status) {
	hipLaunchKernelGGL(k_chol_rhs, dim3((np + 255) / 256), dim3(256), 0, st, pol_list, n_pol, np, e_static, b, status);
}

void launch_chol_scatter(hipStream_t st, const int *pol_list, int n_pol, const double *x, double *mu, const int *status) {
	hipLaunchKernelGGL(k_chol_scatter, dim3((3 * n_pol + 255) / 256), dim3(256), 0, st, pol_list, n_pol, x, mu, status);
}

void launch_chol_finish(hipStream_t st, const AtomsDev &at, const double *mu, const double *e_static, double *e_induced, const int *status,
                        double *info) {
	hipLaunchKernelGGL(k_chol_finish, dim3(1), dim3(256), 0, st, at, mu, e_static, e_induced, status, info);
}

} // namespace mpmc
