// The rd model's MPMC_HD functions of csrc/pair_math.h (rd_mix, rd_pair_energy with its three forms) on the host: one line per point of a
// grid of (sigma_i, eps_i, sigma_j, eps_j, r), every form and rule, printed at %.17g for tests/test_rd_model.py to compare with its numpy
// restatement.  The grid holds sigma_j = 0, eps_j = 0 and, per pair, r at 0.4 sigma_ij and at its two neighbours.  Plain C++: no HIP, no
// library; the sanitizer build of this program is the sanitizer run of these functions.
//   line: form mix sigma_i eps_i sigma_j eps_j r  sigma_ij eps_ij energy
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../mpmcxx_amd/csrc/pair_math.h"

using namespace mpmc;

static RdAtom atom(double s, double e) { return RdAtom{s, s * s, s * s * s, (s * s * s) * (s * s * s), std::sqrt(e), e}; }

struct HostExp {
	double operator()(double x) const { return std::exp(x); }
};

template <int FORM, int MIX>
static void point(double si, double ei, double sj, double ej, double r) {
	const RdMixed m = rd_mix<MIX, FORM>(atom(si, ei), atom(sj, ej));
	const double e = rd_pair_energy<FORM>(m, r * r, 0, 0.0, 0.0, 0.0, HostExp{});
	std::printf("%d %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", FORM, MIX, si, ei, sj, ej, r, m.sigma, m.eps, e);
}

template <int FORM, int MIX>
static void grid() {
	const double sig[] = {3.405, 2.958, 2.28, 0.0}, eps[] = {119.8, 36.7, 10.22, 0.0};
	for (int a = 0; a < 3; a++)
		for (int b = 0; b < 4; b++)
			for (int c = 0; c < 4; c++) {
				const double si = sig[a], ei = eps[a], sj = sig[b], ej = eps[c];
				const RdMixed m = rd_mix<MIX, FORM>(atom(si, ei), atom(sj, ej));
				std::vector<double> rs = {0.9, 2.0, 3.0, 3.7, 5.0, 9.5, 12.0};
				if (m.sigma > 0.0) { // the DREIDING contact threshold, from both sides
					const double rc = 0.4 * m.sigma;
					rs.push_back(rc);
					rs.push_back(std::nextafter(rc, 0.0));
					rs.push_back(std::nextafter(rc, 1e9));
				}
				for (double r : rs) point<FORM, MIX>(si, ei, sj, ej, r);
			}
}

template <int FORM>
static void rules() {
	grid<FORM, RD_MIX_LB>();
	grid<FORM, RD_MIX_WALDMAN_HAGLER>();
	grid<FORM, RD_MIX_HALGREN>();
	grid<FORM, RD_MIX_C6>();
}

int main() {
	rules<RD_FORM_LJ>();
	rules<RD_FORM_BUFFERED_14_7>();
	rules<RD_FORM_DREIDING>();
	return 0;
}
