// `polar_sor` / `polar_esor` / `polar_zodid` through include/mpmc_io.hpp: prints what the reader made of the input file given as argv[1]
// (the facade's three fields and the refusal bits that remain: none for these keywords, MPMC_FLAG_POLAR_GS_RANKED for `polar_gs_ranked`),
// or the code it threw (3000 for both schemes together and for zodid with polar_iterative off).
#include <cstdio>

#include "mpmc_io.hpp"
#include "mpmc_system.hpp"

int main(int argc, char **argv) {
	if (argc < 2) return 2;
	try {
		mpmc::System s;
		mpmc::read_input(argv[1], s);
		std::printf("read %d %d %d %.17g %llu\n", s.polar_sor, s.polar_esor, s.polar_zodid, s.polar_gamma, (unsigned long long)s.unsupported_flags);
	} catch (int e) {
		std::printf("read thrown %d\n", e);
	}
	return 0;
}
