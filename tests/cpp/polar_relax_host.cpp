// The weights and the blend of `polar_sor` / `polar_esor` (mpmcxx_amd/csrc/polar_relax.h) on the host: the functions the update kernels'
// relaxed instantiations call.  Reads lines "scheme gamma it new_mu old_mu" from stdin and prints, per line, w_new, w_old and the blend at
// %.17g; tests/test_polar_relax.py compares them with the numpy restatement and runs this program once more under the address and
// undefined-behaviour sanitizers.
#include <cstdio>

#include "polar_relax.h"

int main() {
	int scheme, it;
	double gamma, nm, om;
	int lines = 0;
	while (std::scanf("%d %lf %d %lf %lf", &scheme, &gamma, &it, &nm, &om) == 5) {
		const mpmc::RelaxWeights w = mpmc::relax_weights(scheme, gamma, it);
		std::printf("%.17g %.17g %.17g\n", w.w_new, w.w_old, mpmc::relax_blend(w.w_new, w.w_old, nm, om));
		lines++;
	}
	return lines > 0 ? 0 : 1;
}
