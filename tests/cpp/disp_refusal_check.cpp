// The PI-NVT and Gibbs drivers refuse the disp-expansion term (4004) before anything is evaluated: prints one line per driver.
#include <cstdio>

#include "mpmc_gibbs.hpp"
#include "mpmc_pimc.hpp"
#include "mpmc_system.hpp"

static void one_atom(mpmc::System &s, bool disp) {
	mpmc::Atom a;
	a.epsilon = 3.1, a.sigma = 3.45, a.c6 = 64.3, a.c8 = 1623.0, a.c10 = 49060.0;
	s.atoms.push_back(a);
	s.using_disp_expansion = disp;
}

int main() {
	mpmc::System images[4];
	mpmc::PathIntegralNVT<mpmc::System> pi;
	for (auto &s : images) one_atom(s, true), pi.systems.push_back(&s);
	pi.cfg.PI_trial_chain_length = 1, pi.cfg.numsteps = 1, pi.cfg.corrtime = 1, pi.cfg.temperature = 77.0;
	int code = 0;
	try {
		pi.init();
	} catch (int e) {
		code = e;
	}
	std::printf("pimc %d\n", code);
	mpmc::System a, b;
	one_atom(a, false), one_atom(b, true);
	mpmc::GibbsBoxesT<mpmc::System> g(a, b);
	code = 0;
	try {
		g.energy();
	} catch (int e) {
		code = e;
	}
	std::printf("gibbs %d\n", code);
	return 0;
}
