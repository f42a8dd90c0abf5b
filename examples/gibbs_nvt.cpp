// examples/gibbs_nvt.cpp -- an `ensemble nvt_gibbs` input of the reference run end to end on the HIP path.
//   gibbs_nvt INPUT.in [STEPS] [--trials] [--time]
// --trials: every move runs as a device trial (GibbsSettings::device_trials) instead of a full evaluation of both boxes per step; the JSON
// then also carries the sums over both boxes of the library's exchange-trial and volume-trial counters.
// --time: the wall time of the step loop alone goes to stderr (tools/gibbs_bench.py); stdout is the same with and without it.
// Box 0 = pqr_input on device 0, box 1 = pqr_input_B (default: the same file) on device 1 when the node shows two GPUs.  Prints the
// trajectory as one JSON object: per step the move types, the two trial energies, the Boltzmann factors, what was accepted, N and
// volume of both boxes; then the final geometries (include/mpmc_gibbs_run.hpp).
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "mpmc_gibbs_run.hpp"

int main(int argc, char **argv) {
	if (argc < 2) {
		std::fprintf(stderr, "usage: %s INPUT.in [STEPS] [--trials] [--time]\n", argv[0]);
		return 2;
	}
	try {
		mpmc::GibbsSettings cfg = mpmc::read_gibbs_settings(argv[1]);
		int steps = -1;
		bool timed = false;
		for (int k = 2; k < argc; k++) {
			if (std::strcmp(argv[k], "--trials") == 0) cfg.device_trials = true;
			else if (std::strcmp(argv[k], "--time") == 0) timed = true;
			else steps = std::atoi(argv[k]);
		}
		mpmc::System a, b;
		const std::string pqr_a = mpmc::read_input(argv[1], a);
		(void)mpmc::read_input(argv[1], b);
		std::string pqr_b = cfg.pqr_input_B.empty() ? pqr_a : cfg.pqr_input_B;
		if (pqr_b[0] != '/') pqr_b = mpmc::io_detail::dirname_of(argv[1]) + "/" + pqr_b;
		mpmc::read_pqr(pqr_a, a);
		mpmc::read_pqr(pqr_b, b);
		a.update_pbc();
		b.update_pbc();
		a.eager_dipoles = b.eager_dipoles = false;
		int ndev = 0;
		if (mpmc_device_count(&ndev) != MPMC_OK || ndev < 1) throw (int)MPMC_ERR_NO_DEVICE;
		a.device = 0;
		b.device = 1 % ndev;
		double loop_seconds = 0;
		mpmc::run_gibbs_and_print(a, b, cfg, steps, &loop_seconds);
		if (timed) std::fprintf(stderr, "step loop: %.6f s\n", loop_seconds);
	} catch (int code) {
		std::printf("{\"error\": %d}\n", code);
		return 1;
	}
	return 0;
}
