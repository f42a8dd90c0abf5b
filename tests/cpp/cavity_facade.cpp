// The cavity-bias grid through include/mpmc_system.hpp: argv[1] is an input file (lj64.in), argv[2] the grid size, argv[3] the sphere radius.
// One System::cavity_update_grid with a default-seeded std::mt19937, then the insertion point of one more draw of the same generator.
// Prints one JSON line.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "mpmc_io.hpp"
#include "mpmc_system.hpp"

int main(int argc, char **argv) {
	if (argc < 4) return 2;
	try {
		mpmc::System s;
		mpmc::load_system(argv[1], s);
		s.cavity_bias = 1;
		s.cavity_grid_size = std::atoi(argv[2]);
		s.cavity_radius = std::atof(argv[3]);
		std::mt19937 rng; // (default seed, as the reference's System::mt_rand when nothing seeds it)
		s.cavity_update_grid(rng);
		std::uniform_real_distribution<double> dist{0, 1};
		const double u = dist(rng);
		double pos[3] = {0, 0, 0};
		s.cavity_insertion_point(u, pos);
		std::printf("{\"cavities_open\": %d, \"hits\": %lld, \"n_darts\": %lld, \"probability\": %.17g, \"cavity_volume\": %.17g, \"u\": %.17g, "
		            "\"point\": [%.17g, %.17g, %.17g]}\n",
		            s.cavities_open, (long long)s.cavity_result.hits, (long long)s.cavity_result.n_darts, s.cavity_bias_probability, s.cavity_volume, u, pos[0], pos[1],
		            pos[2]);
	} catch (int code) {
		std::printf("{\"error\": %d}\n", code);
		return 1;
	}
	return 0;
}
