// `polar_ewald_full` through include/mpmc_io.hpp and the drivers: prints what the reader made of the input file given as argv[1] (the
// facade's field, and whether MPMC_FLAG_POLAR_EWALD_FULL is still set: the reader keeps setting it, mpmc::System clears it when it hands the
// term to mpmc_set_polar_ewald_full), then one line per driver: the PI-NVT and Gibbs drivers refuse a System with the term (4004) before
// anything is evaluated.
#include <cstdio>

#include "mpmc_gibbs.hpp"
#include "mpmc_io.hpp"
#include "mpmc_pimc.hpp"
#include "mpmc_system.hpp"

static void one_atom(mpmc::System &s, int ewald_full) {
	mpmc::Atom a;
	a.epsilon = 3.1, a.sigma = 3.45;
	s.atoms.push_back(a);
	s.polar_ewald_full = ewald_full;
}

int main(int argc, char **argv) {
	if (argc > 1) {
		try {
			mpmc::System s;
			mpmc::read_input(argv[1], s);
			std::printf("read %d %d %d %llu\n", s.polar_ewald_full, s.polar_ewald_full_vector_kweight, (s.unsupported_flags & MPMC_FLAG_POLAR_EWALD_FULL) ? 1 : 0,
			            (unsigned long long)(s.unsupported_flags & ~(uint64_t)MPMC_FLAG_POLAR_EWALD_FULL));
		} catch (int e) {
			std::printf("read thrown %d\n", e);
		}
	}
	{
		mpmc::System images[4];
		mpmc::PathIntegralNVT<mpmc::System> pi;
		for (auto &s : images) one_atom(s, 1), pi.systems.push_back(&s);
		pi.cfg.PI_trial_chain_length = 1, pi.cfg.numsteps = 1, pi.cfg.corrtime = 1, pi.cfg.temperature = 77.0;
		int code = 0;
		try {
			pi.init();
		} catch (int e) {
			code = e;
		}
		std::printf("pimc %d\n", code);
		mpmc::System a, b;
		one_atom(a, 0), one_atom(b, 1);
		mpmc::GibbsBoxesT<mpmc::System> g(a, b);
		code = 0;
		try {
			g.energy();
		} catch (int e) {
			code = e;
		}
		std::printf("gibbs %d\n", code);
	}
	return 0;
}
