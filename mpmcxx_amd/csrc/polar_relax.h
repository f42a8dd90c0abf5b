// polar_relax.h -- `polar_sor` / `polar_esor`: the weights and the blend of the relaxed dipole update (thole_iterative :3526-3536, new_dipoles
// :3181-3211).  Host and device: the weights are computed on the host (they depend on the iteration number alone) and travel as kernel
// arguments; the blend runs in the update kernels' relaxed instantiations.  tests/polar_relax_host.cpp checks both on the host.
#pragma once
#include <cmath>

#include "pair_math.h"

namespace mpmc {

enum : int { RELAX_NONE = 0, RELAX_SOR = 1, RELAX_ESOR = 2 }; // = MPMC_POLAR_RELAX_*

// mu = w_new new_mu + w_old old_mu
struct RelaxWeights {
	double w_new, w_old;
};

// `it`: the 1-based iteration of thole_iterative; ewald_full passes its 0-based pass counter + 1 (:3196-3204).  The reference's expressions:
// polar_gamma and (1.0 - polar_gamma); (1.0 - exp(-polar_gamma * it)) and exp(-polar_gamma * it), exp in double.
inline RelaxWeights relax_weights(int scheme, double gamma, int it) {
	RelaxWeights w{1.0, 0.0};
	if (scheme == RELAX_SOR) w = RelaxWeights{gamma, 1.0 - gamma};
	else if (scheme == RELAX_ESOR) w = RelaxWeights{1.0 - std::exp(-gamma * it), std::exp(-gamma * it)};
	return w;
}

MPMC_HD double relax_blend(double w_new, double w_old, double new_mu, double old_mu) { return w_new * new_mu + w_old * old_mu; }

} // namespace mpmc
