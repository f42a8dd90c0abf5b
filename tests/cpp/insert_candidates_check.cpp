// Batched insertion candidates through include/mpmc_system.hpp: a small box of charged Lennard-Jones dimers and 70 poses of one more dimer.
// energy_insert_candidates must give, candidate by candidate and field by field, the mpmc_result of energy_trial_insert + reject_trial;
// the accepted energy is the same before and after; one candidate is then accepted through the single trial.  Prints one JSON line.
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
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

int main() {
	try {
		mpmc::System s;
		fill(s, 4, 4.1);
		const double e0 = s.energy();
		const int n_cand = 70;
		mpmc::Molecule species(s.atoms.begin() + 10, s.atoms.begin() + 12);
		std::vector<std::vector<std::array<double, 3>>> poses;
		unsigned long long state = 12345; // (a fixed linear congruential sequence: centres over [-1, 2) box lengths, wrapped images included)
		auto u = [&]() {
			state = state * 6364136223846793005ULL + 1442695040888963407ULL;
			return (double)(state >> 11) / 9007199254740992.0;
		};
		for (int c = 0; c < n_cand; c++) {
			const double L = 4 * 4.1, cx = (3 * u() - 1) * L, cy = (3 * u() - 1) * L, cz = (3 * u() - 1) * L, th = 6.283185307179586 * u();
			poses.push_back({{{cx, cy, cz}}, {{cx + 0.6 * std::cos(th), cy + 0.6 * std::sin(th), cz + 0.15}}});
		}
		const std::vector<mpmc_result> batch = s.energy_insert_candidates(species, poses);
		int mismatches = 0;
		for (int c = 0; c < n_cand; c++) {
			mpmc::Molecule mol = species;
			for (int i = 0; i < 2; i++)
				for (int p = 0; p < 3; p++) mol[i].pos[p] = poses[c][i][p];
			s.energy_trial_insert((int)s.atoms.size(), mol);
			const mpmc_result one = s.trial_result();
			s.reject_trial();
			if (std::memcmp(&one, &batch[c], sizeof(mpmc_result)) != 0) mismatches++;
		}
		const double e_after = s.energy();
		mpmc::Molecule mol = species;
		for (int i = 0; i < 2; i++)
			for (int p = 0; p < 3; p++) mol[i].pos[p] = poses[17][i][p];
		const double e_in = s.energy_trial_insert((int)s.atoms.size(), mol);
		s.accept_trial();
		const std::vector<mpmc_result> second = s.energy_insert_candidates(species, poses);
		int refused = 0;
		try {
			poses[3].pop_back();
			s.energy_insert_candidates(species, poses);
		} catch (int code) {
			refused = code;
		}
		std::printf("{\"n_batch\": %d, \"mismatches\": %d, \"e0\": %.17g, \"e_after\": %.17g, \"e_in\": %.17g, \"e_batch_17\": %.17g, \"n_in\": %d, "
		            "\"N_second\": %.17g, \"n_second\": %d, \"refused\": %d}\n",
		            (int)batch.size(), mismatches, e0, e_after, e_in, batch[17].energy, (int)s.atoms.size(), second[0].N, (int)second.size(), refused);
	} catch (int code) {
		std::printf("{\"error\": %d}\n", code);
		return 1;
	}
	return 0;
}
