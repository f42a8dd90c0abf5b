// `polar_gs_ranked` through include/mpmc_io.hpp: prints what the reader made of the input file given as argv[1] (the facade's fields
// polar_gs and polar_gs_ranked and the refusal bits: the reader keeps MPMC_FLAG_POLAR_GS_RANKED set, the facade clears it when it hands
// the field to mpmc_set_polar_gs_ranked).  With a second argument it then asks the facade for the energy and prints the code that threw:
// polar_gs and polar_gs_ranked together are refused with 3000 before anything reaches a device (only such inputs are given that way).
#include <cstdio>

#include "mpmc_io.hpp"
#include "mpmc_system.hpp"

int main(int argc, char **argv) {
	if (argc < 2) return 2;
	mpmc::System s;
	try {
		mpmc::load_system(argv[1], s);
		std::printf("read %d %d %llu\n", s.polar_gs, s.polar_gs_ranked, (unsigned long long)s.unsupported_flags);
	} catch (int e) {
		std::printf("read thrown %d\n", e);
		return 0;
	}
	if (argc < 3) return 0;
	try {
		std::printf("energy %.17g\n", s.energy());
	} catch (int e) {
		std::printf("energy thrown %d\n", e);
	}
	return 0;
}
