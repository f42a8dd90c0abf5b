// Exchange trials through include/mpmc_system.hpp: a small box of charged Lennard-Jones dimers; one dimer is inserted (accepted), one
// removed (rejected), one removed (accepted).  After every accepted trial the facade's own list must be the library's: the next energy()
// uploads nothing, and a second System built from the edited list gives the same totals.  Prints one JSON line.
#include <cmath>
#include <cstdio>
#include <vector>

#include "mpmc_system.hpp"

static void fill(mpmc::System &s, int cells, double edge) {
	for (int p = 0; p < 3; p++)
		for (int q = 0; q < 3; q++) s.pbc.basis[p][q] = (p == q) ? cells * edge : 0.0;
	int mol = 0;
	for (int x = 0; x < cells; x++)
		for (int y = 0; y < cells; y++)
			for (int z = 0; z < cells; z++, mol++)
				for (int k = 0; k < 2; k++) {
					mpmc::Atom a;
					a.pos[0] = (x + 0.31) * edge + 0.55 * k, a.pos[1] = (y + 0.47) * edge + 0.1 * ((x + z) % 3), a.pos[2] = (z + 0.52) * edge - 0.2 * k;
					a.mass = 14.0, a.charge = k ? -0.4 : 0.4, a.epsilon = 36.0, a.sigma = 3.3;
					a.molecule = mol;
					s.atoms.push_back(a);
				}
	s.update_pbc();
}

static double fresh_energy(const mpmc::System &like) {
	mpmc::System t;
	for (int p = 0; p < 3; p++)
		for (int q = 0; q < 3; q++) t.pbc.basis[p][q] = like.pbc.basis[p][q];
	t.atoms = like.atoms;
	t.update_pbc();
	return t.energy();
}

int main() {
	try {
		mpmc::System s;
		fill(s, 4, 4.1);
		const double e0 = s.energy();
		std::vector<mpmc::Atom> mol(s.atoms.begin() + 10, s.atoms.begin() + 12);
		for (auto &a : mol) a.pos[0] += 2.05, a.pos[1] += 1.9, a.pos[2] += 2.2;
		const double e_in = s.energy_trial_insert(6, mol);
		const double n_trial = s.trial_result().N;
		s.accept_trial();
		const int n_in = (int)s.atoms.size();
		const double e_in_fresh = fresh_energy(s), e_in_again = s.energy();
		const double e_out = s.energy_trial_remove(20, 2);
		s.reject_trial();
		const double e_back = s.energy();
		s.energy_trial_remove_async(6, 2);
		const double e_gone = s.energy_trial_wait();
		s.accept_trial();
		int refused = 0;
		try {
			s.energy_trial_remove(3, 2); // straddles two molecules
		} catch (int code) {
			refused = code;
		}
		std::printf("{\"e0\": %.17g, \"e_in\": %.17g, \"e_in_fresh\": %.17g, \"e_in_again\": %.17g, \"e_out\": %.17g, \"e_back\": %.17g, \"e_gone\": %.17g, "
		            "\"e_final\": %.17g, \"n_in\": %d, \"n_final\": %d, \"N_trial\": %.17g, \"refused\": %d}\n",
		            e0, e_in, e_in_fresh, e_in_again, e_out, e_back, e_gone, s.energy(), n_in, (int)s.atoms.size(), n_trial, refused);
	} catch (int code) {
		std::printf("{\"error\": %d}\n", code);
		return 1;
	}
	return 0;
}
