// `rd_crystal` through include/mpmc_io.hpp: prints what the reader made of the input file given as argv[1] -- the facade's two fields, and
// whether MPMC_FLAG_RD_CRYSTAL is still set (the reader keeps setting it; mpmc::System clears it when it hands the term to
// mpmc_set_rd_crystal).
#include <cstdio>

#include "mpmc_io.hpp"
#include "mpmc_system.hpp"

int main(int argc, char **argv) {
	if (argc < 2) return 2;
	try {
		mpmc::System s;
		mpmc::read_input(argv[1], s);
		std::printf("read %d %d %d %llu\n", s.rd_crystal, s.rd_crystal_order, (s.unsupported_flags & MPMC_FLAG_RD_CRYSTAL) ? 1 : 0,
		            (unsigned long long)s.unsupported_flags);
	} catch (int e) {
		std::printf("read thrown %d\n", e);
	}
	return 0;
}
