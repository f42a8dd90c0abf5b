// `polar_wolf` / `polar_palmo` through include/mpmc_io.hpp and the drivers: prints what the reader made of the input file given as argv[1]
// (polar_wolf, polar_palmo, polar_wolf_alpha, unsupported flags), then one line per driver: the PI-NVT and Gibbs drivers refuse a System
// with either option (4004) before anything is evaluated.
#include <cstdio>

#include "mpmc_gibbs.hpp"
#include "mpmc_io.hpp"
#include "mpmc_pimc.hpp"
#include "mpmc_system.hpp"

static void one_atom(mpmc::System &s, int wolf, int palmo) {
	mpmc::Atom a;
	a.epsilon = 3.1, a.sigma = 3.45;
	s.atoms.push_back(a);
	s.polar_wolf = wolf, s.polar_palmo = palmo;
}

int main(int argc, char **argv) {
	if (argc > 1) {
		try {
			mpmc::System s;
			mpmc::read_input(argv[1], s);
			std::printf("read %d %d %.17g %llu\n", s.polar_wolf, s.polar_palmo, s.polar_wolf_alpha, (unsigned long long)s.unsupported_flags);
		} catch (int e) {
			std::printf("read thrown %d\n", e);
		}
	}
	for (int which = 0; which < 2; which++) {
		mpmc::System images[4];
		mpmc::PathIntegralNVT<mpmc::System> pi;
		for (auto &s : images) one_atom(s, which == 0, which == 1), pi.systems.push_back(&s);
		pi.cfg.PI_trial_chain_length = 1, pi.cfg.numsteps = 1, pi.cfg.corrtime = 1, pi.cfg.temperature = 77.0;
		int code = 0;
		try {
			pi.init();
		} catch (int e) {
			code = e;
		}
		std::printf("pimc %d\n", code);
		mpmc::System a, b;
		one_atom(a, 0, 0), one_atom(b, which == 0, which == 1);
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
