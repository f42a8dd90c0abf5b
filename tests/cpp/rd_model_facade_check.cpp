// The rd model through include/mpmc_io.hpp and the drivers: prints what the reader made of the input file given as argv[1] (the facade's
// five fields, the form and rule they select, and the flag bits that are set: none for these keywords), then one line per driver: the
// PI-NVT and Gibbs drivers refuse a System with a non-default model (4004) before anything is evaluated.
#include <cstdio>

#include "mpmc_gibbs.hpp"
#include "mpmc_io.hpp"
#include "mpmc_pimc.hpp"
#include "mpmc_system.hpp"

static void one_atom(mpmc::System &s, int halgren, bool b147) {
	mpmc::Atom a;
	a.epsilon = 3.1, a.sigma = 3.45;
	s.atoms.push_back(a);
	s.halgren_mixing = halgren;
	s.using_lj_buffered_14_7 = b147;
}

int main(int argc, char **argv) {
	if (argc > 1) {
		try {
			mpmc::System s;
			mpmc::read_input(argv[1], s);
			std::printf("read %d %d %d %d %d form %d mix %d flags %llu\n", s.waldmanhagler, s.halgren_mixing, s.c6_mixing, s.using_lj_buffered_14_7 ? 1 : 0,
			            s.use_dreiding, s.rd_model_form(), s.rd_model_mixing(), (unsigned long long)s.unsupported_flags);
		} catch (int e) {
			std::printf("read thrown %d\n", e);
		}
	}
	{
		mpmc::System images[4];
		mpmc::PathIntegralNVT<mpmc::System> pi;
		for (auto &s : images) one_atom(s, 1, false), pi.systems.push_back(&s);
		pi.cfg.PI_trial_chain_length = 1, pi.cfg.numsteps = 1, pi.cfg.corrtime = 1, pi.cfg.temperature = 77.0;
		int code = 0;
		try {
			pi.init();
		} catch (int e) {
			code = e;
		}
		std::printf("pimc %d\n", code);
		mpmc::System a, b;
		one_atom(a, 0, false), one_atom(b, 0, true);
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
