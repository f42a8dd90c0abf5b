// kernels_volume.hip -- the position half of a volume-change trial move: System::volume_change / volume_change_Gibbs (reference
// src/System.MonteCarlo.cpp:1235-1340).  Every molecule is shifted rigidly by com * s - com, com = Molecule::update_COM of the accepted
// positions (src/Molecule.cpp:259-281), in the reference's arithmetic: mass += m_i and cm[p] += m_i * pos_i[p] atom by atom in list order,
// cm[p] /= mass, delta[p] = cm[p] * s - cm[p], pos_i[p] += delta[p].  The build is -ffp-contract=off: the expressions below round as written.
#include "kernels.h"

namespace mpmc {

// One wave per molecule.  The sums of a molecule are SEQUENTIAL by contract (a frozen framework is one molecule of thousands of atoms, and
// its centre must have the bits of the host's loop), so the wave shares the part that can be shared: 64 lanes gather 64 atoms of the
// molecule at a time (slot_of, position, mass: three dependent loads per atom, the latency of the whole move) and form the products, then
// every lane adds the 64 values in atom order from lane broadcasts -- the index is wave-uniform, so the broadcast is a lane read, and all
// lanes end with the same four sums.  A one-atom molecule costs one chunk with one addition; 10 000 of them are 10 000 short waves, a few
// microseconds.  The second pass writes the shifted atoms, 64 per step, into the alternate position buffer: the atoms keep their slots.
constexpr int kVolumeBlock = 256; // four waves (four molecules) per workgroup

__global__ __launch_bounds__(kVolumeBlock) void k_volume_scale(const double4 *__restrict__ xyzq, const int *__restrict__ slot_of, const double *__restrict__ mass,
                                                              const int *__restrict__ mol_first, int n_mol, int n, int n_pad, double s,
                                                              double4 *__restrict__ out) {
	const int lane = threadIdx.x & 63;
	const int mol = blockIdx.x * (kVolumeBlock / 64) + (threadIdx.x >> 6);
	// the padding slots behind the last atom travel as they are (n_pad - n < 64: the first workgroup's first wave)
	if (blockIdx.x == 0 && threadIdx.x < n_pad - n) out[n + threadIdx.x] = xyzq[n + threadIdx.x];
	if (mol >= n_mol) return; // (whole waves leave: the broadcasts below are never divergent)
	const int i0 = mol_first[mol], i1 = mol_first[mol + 1];
	double msum = 0.0, cx = 0.0, cy = 0.0, cz = 0.0;
	for (int base = i0; base < i1; base += 64) {
		const int i = base + lane;
		double m = 0.0, px = 0.0, py = 0.0, pz = 0.0;
		if (i < i1) {
			const double4 r = xyzq[slot_of[i]];
			m = mass[i];
			px = m * r.x, py = m * r.y, pz = m * r.z;
		}
		const int cnt = min(64, i1 - base);
		for (int k = 0; k < cnt; k++) {
			msum += __shfl(m, k, 64);
			cx += __shfl(px, k, 64);
			cy += __shfl(py, k, 64);
			cz += __shfl(pz, k, 64);
		}
	}
	cx /= msum, cy /= msum, cz /= msum;
	const double dx = cx * s - cx, dy = cy * s - cy, dz = cz * s - cz;
	for (int i = i0 + lane; i < i1; i += 64) {
		const int k = slot_of[i];
		const double4 r = xyzq[k];
		out[k] = make_double4(r.x + dx, r.y + dy, r.z + dz, r.w);
	}
}

void launch_volume_scale(hipStream_t st, const double4 *xyzq, const int *slot_of, const double *mass, const int *mol_first, int n_mol, int n, int n_pad, double s,
                         double4 *out) {
	const int per = kVolumeBlock / 64, blocks = std::max(1, (n_mol + per - 1) / per);
	hipLaunchKernelGGL(k_volume_scale, dim3(blocks), dim3(kVolumeBlock), 0, st, xyzq, slot_of, mass, mol_first, n_mol, n, n_pad, s, out);
}

} // namespace mpmc
