// cavity_autoreject through include/mpmc_io.hpp: prints what the reader made of the input file given as argv[1] -- the facade's four fields,
// the rules it would hand to mpmc_set_cavity_autoreject, and whether MPMC_FLAG_CAVITY_AUTOREJECT is still set (the reader keeps setting it;
// mpmc::System clears it when it hands the rules over).  Without an argument: the size of the info struct, for the ctypes mirror.
#include <cstdio>

#include "mpmc_io.hpp"
#include "mpmc_system.hpp"

int main(int argc, char **argv) {
	if (argc < 2) {
		std::printf("sizeof %zu\n", sizeof(struct mpmc_cavity_autoreject_info));
		return 0;
	}
	try {
		mpmc::System s;
		mpmc::read_input(argv[1], s);
		std::printf("read %d %d %.17g %.17g %d %d\n", s.cavity_autoreject, s.cavity_autoreject_absolute, s.cavity_autoreject_scale, s.cavity_autoreject_repulsion,
		            s.cavity_autoreject_rules(), (s.unsupported_flags & MPMC_FLAG_CAVITY_AUTOREJECT) ? 1 : 0);
	} catch (int e) {
		std::printf("read thrown %d\n", e);
	}
	return 0;
}
