// Volume trials through include/mpmc_system.hpp: a small box of charged Lennard-Jones dimers with unequal masses.  One volume trial is
// rejected (cell and list stay, the next energy() has the first one's bits), one accepted (pbc and `atoms` follow in the library's
// arithmetic: the next energy() uploads nothing and agrees with a second System built from the scaled list), one accepted through the
// two halves.  Prints one JSON line.
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
					a.mass = k ? 14.0 : 1.0, a.charge = k ? -0.4 : 0.4, a.epsilon = 36.0, a.sigma = 3.3;
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
		const double e0 = s.energy(), v0 = s.pbc.volume;
		const double e_rej = s.energy_trial_volume(1.04);
		const double v_trial = s.trial_volume();
		s.reject_trial();
		const double e_back = s.energy(), v_back = s.pbc.volume;
		const double e_acc = s.energy_trial_volume(0.97);
		s.accept_trial();
		const double v_acc = s.pbc.volume, e_acc_again = s.energy(), e_acc_fresh = fresh_energy(s);
		s.energy_trial_volume_async(1.02);
		const double e_two = s.energy_trial_wait();
		s.accept_trial();
		int refused = 0;
		try {
			s.energy_trial_volume(-1.0);
		} catch (int code) {
			refused = code;
		}
		std::printf("{\"e0\": %.17g, \"v0\": %.17g, \"e_rej\": %.17g, \"v_trial\": %.17g, \"e_back\": %.17g, \"v_back\": %.17g, \"e_acc\": %.17g, \"v_acc\": %.17g, "
		            "\"e_acc_again\": %.17g, \"e_acc_fresh\": %.17g, \"e_two\": %.17g, \"e_two_fresh\": %.17g, \"refused\": %d}\n",
		            e0, v0, e_rej, v_trial, e_back, v_back, e_acc, v_acc, e_acc_again, e_acc_fresh, e_two, fresh_energy(s), refused);
	} catch (int code) {
		std::printf("{\"error\": %d}\n", code);
		return 1;
	}
	return 0;
}
