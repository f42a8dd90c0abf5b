// include/mpmc_system.hpp -- C++ host facade over the C ABI (include/mpmc_energy.h).
//
// The reference is compiled C++ whose energy path is a set of `System` member functions; this header gives host
// C++ code the same surface -- same member names, argument meaning, side effects and error behaviour -- so that a
// Monte Carlo accept/reject loop written against the reference's `System` reads the same against this one:
//
//   reference (src/System.h)                         here (namespace mpmc)
//   -----------------------------------------------  ---------------------------------------------------------
//   double System::energy()               :315        double System::energy()
//   lj / coulombic / coulombic_real / _reciprocal /   same names, same return values
//     _self / polar / thole_field         :346-402
//   observables_t *observables            :94-113     observables_t *observables (same field names)
//   nodestats->polarization_iterations    :151-185    nodestats->polarization_iterations
//   int iterator_failed                   :680        int iterator_failed
//   PeriodicBoundary pbc (+ update_pbc)               PeriodicBoundary pbc, update_pbc()
//   option fields rd_only, rd_lrc, polarization, polar_* , ewald_* (:510-831)   same names
//   errors: `throw <int>` (src/constants.h:108-147)   `throw <int>` with the same codes
//   SimulationControl::PI_calculate_potential()       PathIntegralEnsemble::PI_calculate_potential()
//     (src/SimulationControl.PathIntegral.cpp:752)
//
// Data model: flat vectors instead of Molecule -> Atom linked lists (the flattening is what the adapter of
// INTEGRATION.md does for the real reference objects).  Header-only; link with -lmpmc_energy.
#pragma once

#include <array>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <functional>
#include <random>
#include <string>
#include <vector>

#include "mpmc_energy.h"

namespace mpmc {

enum { DAMPING_OFF = 0, DAMPING_LINEAR = 1, DAMPING_EXPONENTIAL = 2 }; // reference constants.h:66-70

// reference src/PeriodicBoundary.h
class PeriodicBoundary {
public:
	double cutoff = 0, volume = 0;
	double basis[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
	double reciprocal_basis[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
	void update() { // PeriodicBoundary::update, src/PeriodicBoundary.cpp:31-35
		int rc = mpmc_pbc_compute(&basis[0][0], &reciprocal_basis[0][0], &volume, &cutoff);
		if (rc != MPMC_OK) throw (int)MPMC_ERR_BOX;
	}
};

// reference src/System.h:94-113
struct observables_t {
	double energy = 0, coulombic_energy = 0, rd_energy = 0, polarization_energy = 0, vdw_energy = 0, three_body_energy = 0,
	       dipole_rrms = 0, kinetic_energy = 0, temperature = 0, volume = 0, N = 0, NU = 0, spin_ratio = 0, frozen_mass = 0, total_mass = 0;
	double potential() const { return coulombic_energy + rd_energy + polarization_energy + vdw_energy + three_body_energy; }
};
struct nodestats_t {
	double polarization_iterations = 0;
};

// whether a System-like type switches the Axilrod-Teller term on (the drivers are templates; a type without the member never does)
template <class T>
auto uses_three_body(const T &s, int) -> decltype(bool(s.using_axilrod_teller)) { return s.using_axilrod_teller; }
template <class T>
bool uses_three_body(const T &, long) { return false; }
// the same for the disp-expansion term
template <class T>
auto uses_disp_expansion(const T &s, int) -> decltype(bool(s.using_disp_expansion)) { return s.using_disp_expansion; }
template <class T>
bool uses_disp_expansion(const T &, long) { return false; }
// the same for the Wolf static field and the Palmo-Krimm correction
template <class T>
auto uses_polar_wolf_or_palmo(const T &s, int) -> decltype(bool(s.polar_wolf || s.polar_palmo)) { return s.polar_wolf || s.polar_palmo; }
template <class T>
bool uses_polar_wolf_or_palmo(const T &, long) { return false; }
// the same for the fully periodic dipole solve
template <class T>
auto uses_polar_ewald_full(const T &s, int) -> decltype(bool(s.polar_ewald_full)) { return s.polar_ewald_full; }
template <class T>
bool uses_polar_ewald_full(const T &, long) { return false; }
// the same for a non-default rd model (another mixing rule, the buffered 14-7 or the DREIDING form)
template <class T>
auto uses_rd_model(const T &s, int) -> decltype(bool(s.rd_model_form() || s.rd_model_mixing())) { return s.rd_model_form() || s.rd_model_mixing(); }
template <class T>
bool uses_rd_model(const T &, long) { return false; }
template <class T>
auto uses_sg(const T &s, int) -> decltype(bool(s.use_sg)) { return s.use_sg != 0; }
template <class T>
bool uses_sg(const T &, long) { return false; }

// one row of the flattened atom list (reference src/Atom.h:21-56, the fields the path reads / writes)
struct Atom {
	double pos[3] = {0, 0, 0};
	double mass = 0, charge = 0, polarizability = 0, epsilon = 0, sigma = 0;
	double c6 = 0, c8 = 0, c10 = 0;
	double c9 = 0; // Axilrod-Teller coefficient (PQR column 20, src/System.cpp:721)
	int frozen = 0;
	int molecule = 0; // index of the owning molecule (consecutive atoms with equal index form one Molecule)
	int moltype = -1; // index into System::moltype_names (the molecule-type column of the PQR row; -1: not recorded)
	// written by energy():
	double mu[3] = {0, 0, 0}, ef_static[3] = {0, 0, 0}, ef_induced[3] = {0, 0, 0};
};

using Molecule = std::vector<Atom>; // the atoms of one molecule, in order (a species to insert)

class System {
public:
	// ---- options, reference names and defaults (src/System.h:510-831) ----
	int rd_only = 0, rd_lrc = 1;
	int polarization = 0, polar_iterative = 0, polar_ewald = 0, polar_max_iter = 10, polar_gs = 0, polar_rrms = 0;
	int damp_type = DAMPING_EXPONENTIAL;
	int ewald_kmax = 7;
	int wolf = 0, feynman_hibbs = 0, feynman_hibbs_order = 0;
	bool using_axilrod_teller = false; // three-body dispersion (mpmc_set_axilrod_teller), src/System.h:659
	int midzuno_kihara_approx = 0;     // its c9 from c6, src/System.h:655
	bool using_disp_expansion = false; // disp-expansion repulsion/dispersion in place of lj() (mpmc_set_disp_expansion), src/System.h:661
	int damp_dispersion = 0, extrapolate_disp_coeffs = 0, schmidt_ff = 0; // its switches, src/System.h:649-656
	int dipoles_on_demand = 0; // energy() / energy_async() stop at the Jacobi iterations the energy needs; fetch_dipoles() runs the rest (mpmc_set_dipoles_on_demand)
	int polar_wolf = 0, polar_palmo = 0; // Wolf static field (mpmc_set_polar_wolf), Palmo-Krimm correction (mpmc_set_polar_palmo), src/System.h:685-694
	int rd_crystal = 0, rd_crystal_order = 0; // lattice-summed Lennard-Jones (mpmc_set_rd_crystal), src/System.h:632-633
	// the rd model (mpmc_set_rd_model): mixing rules src/System.h: waldmanhagler, halgren_mixing, c6_mixing; forms use_dreiding, using_lj_buffered_14_7
	int waldmanhagler = 0, halgren_mixing = 0, c6_mixing = 0, use_dreiding = 0;
	bool using_lj_buffered_14_7 = false;
	// dreiding wins over lj_buffered_14_7 (the dispatch order of System::energy, src/System.Energy.cpp:113-127); lj_buffered_14_7 does not switch
	// Halgren mixing on; the branches of pair_exclusions come in the order Waldman-Hagler, Halgren, C6 (src/System.cpp:1072-1165)
	int rd_model_form() const { return use_dreiding ? MPMC_RD_FORM_DREIDING : using_lj_buffered_14_7 ? MPMC_RD_FORM_BUFFERED_14_7 : MPMC_RD_FORM_LJ; }
	int rd_model_mixing() const {
		return waldmanhagler ? MPMC_RD_MIX_WALDMAN_HAGLER : halgren_mixing ? MPMC_RD_MIX_HALGREN : c6_mixing ? MPMC_RD_MIX_C6 : MPMC_RD_MIX_LB;
	}
	int use_sg = 0;                      // the Silvera-Goldman H2 potential in place of lj(), no electrostatics and no polarization (mpmc_set_silvera_goldman), src/System.h: use_sg
	int polar_sor = 0, polar_esor = 0;   // relaxed dipole updates by polar_gamma (mpmc_set_polar_relax), src/System.h: polar_sor, polar_esor
	int polar_zodid = 0;                 // zeroth-order dipoles, mu = alpha E0 (mpmc_set_polar_relax)
	int polar_gs_ranked = 0;             // Gauss-Seidel sweeps in ranked order (mpmc_set_polar_gs_ranked), src/System.h: polar_gs_ranked
	int polar_ewald_full = 0;            // Ewald-summed induced field (mpmc_set_polar_ewald_full), src/System.h: polar_ewald_full
	int polar_ewald_full_vector_kweight = 0; // MPMC_PEF_VECTOR_KWEIGHT: the intended reciprocal-space weight (no keyword: the reference has none)
	// the cavity-bias grid of uVT moves (mpmc_set_cavity_grid), src/System.h: cavity_bias, cavity_grid_size, cavity_radius; what
	// cavity_update_grid() leaves behind: cavities_open, cavity_volume and (nodestats->) cavity_bias_probability
	int cavity_bias = 0, cavity_grid_size = 0;
	double cavity_radius = 0;
	int cavities_open = 0;
	double cavity_volume = 0, cavity_bias_probability = 0;
	mpmc_cavity_result cavity_result{}; // of the last cavity_update_grid (hits and dart count too)
	// contact rejection of uVT moves (mpmc_set_cavity_autoreject), src/System.h: cavity_autoreject, cavity_autoreject_absolute,
	// cavity_autoreject_scale, cavity_autoreject_repulsion.  With a rule on, energy() and the energy_trial* calls return what the reference's
	// energy() returns -- the absolute rule's MAXVALUE included --, the observables stay unpenalised by it
	int cavity_autoreject = 0, cavity_autoreject_absolute = 0;
	double cavity_autoreject_scale = 0, cavity_autoreject_repulsion = 0;
	int cavity_autoreject_rules() const { return (cavity_autoreject ? MPMC_AUTOREJECT_SIGMA : 0) | (cavity_autoreject_absolute ? MPMC_AUTOREJECT_ABSOLUTE : 0); }
	double polar_wolf_alpha = 0;         // its damping parameter in [0, 1] (`polar_wolf_alpha` / `polar_wolf_damp`), src/System.h:697
	double temperature = 0;
	double polar_precision = 0, polar_gamma = 1.0, polar_damp = 0;
	double ewald_alpha = 0.5, polar_ewald_alpha = 0.5;
	int ewald_alpha_set = 0, polar_ewald_alpha_set = 0;
	uint64_t unsupported_flags = 0; // MPMC_FLAG_*: reference switches outside the hot path that are ON
	int solver = MPMC_SOLVER_AUTO;
	int device = 0;
	// the reference's energy() leaves mu / ef_static / ef_induced in every Atom, but reads them only when it writes the dipole and
	// field files (src/System.Output.cpp:1132-1229): a Monte Carlo driver may switch the per-call copy-back off and call
	// update_dipoles() when it samples
	bool eager_dipoles = true;

	// ---- state ----
	PeriodicBoundary pbc;
	std::vector<Atom> atoms;
	std::vector<std::string> moltype_names; // molecule-type labels met by read_pqr, in order of first appearance (Atom::moltype indexes it)
	int natoms = 0;
	int iterator_failed = 0;
	double last_volume = 0;
	observables_t *observables = &obs_;
	nodestats_t *nodestats = &stats_;
	mpmc_result last_result{};

	System() = default;
	System(const System &) = delete;
	System &operator=(const System &) = delete;
	~System() {
		if (ctx_) mpmc_ctx_destroy(ctx_);
	}

	// System::update_pbc, src/System.cpp:859-876
	void update_pbc() {
		pbc.update();
		if (ewald_alpha_set != 1) ewald_alpha = 3.5 / pbc.cutoff;
		if (polar_ewald_alpha_set != 1) polar_ewald_alpha = 3.5 / pbc.cutoff;
		box_dirty_ = true;
	}
	int countNatoms() const { return (int)atoms.size(); }
	// System::countN, src/System.cpp:909-931: molecules that are not frozen.  The flag of a molecule is that of its LAST atom row:
	// the PQR reader overwrites molecule->frozen on every row (src/System.cpp:684); adiabatic / target molecules are refused by the readers
	unsigned int countN() {
		unsigned int count = 0;
		for (size_t i = 0; i < atoms.size(); i++)
			if ((i + 1 == atoms.size() || atoms[i + 1].molecule != atoms[i].molecule) && !atoms[i].frozen) count++;
		observables->N = count;
		return count;
	}
	// Molecule::update_COM for every molecule (src/Molecule.cpp:259-281): com [n_molecules][3], mass, movable flag
	void molecule_coms(std::vector<double> &com, std::vector<double> &mol_mass, std::vector<int32_t> &movable) const {
		com.clear();
		mol_mass.clear();
		movable.clear();
		for (size_t a0 = 0; a0 < atoms.size();) {
			size_t a1 = a0;
			double m = 0, c[3] = {0, 0, 0};
			for (; a1 < atoms.size() && atoms[a1].molecule == atoms[a0].molecule; a1++) {
				m += atoms[a1].mass;
				for (int d = 0; d < 3; d++) c[d] += atoms[a1].mass * atoms[a1].pos[d];
			}
			for (int d = 0; d < 3; d++) com.push_back(c[d] / m);
			mol_mass.push_back(m);
			movable.push_back(atoms[a1 - 1].frozen ? 0 : 1); // last row decides (src/System.cpp:684)
			a0 = a1;
		}
	}

	// call after changing atom parameters or the number of atoms (positions alone: move_atoms)
	void atoms_changed() { atoms_dirty_ = true; }
	// after a Monte Carlo move that displaced atoms [first, first+count)
	void move_atoms(int first, int count) {
		if (atoms_dirty_ || !ctx_) return; // a full upload is pending anyway
		std::vector<double> p(3 * (size_t)count);
		for (int k = 0; k < count; k++)
			for (int d = 0; d < 3; d++) p[3 * k + d] = atoms[first + k].pos[d];
		check(mpmc_update_positions(ctx_, first, count, p.data()), "mpmc_update_positions");
	}

	// ---- double System::energy(), src/System.Energy.cpp:19-171 ----
	double energy() {
		sync_state();
		mpmc_result r;
		check(mpmc_energy(ctx_, &r), "mpmc_energy");
		absorb(r);
		return returned(r);
	}
	void energy_async() {
		sync_state();
		check(mpmc_hint_in_flight(ctx_, in_flight_hint_), "mpmc_hint_in_flight");
		check(mpmc_energy_async(ctx_), "mpmc_energy_async");
	}
	// how many evaluations the caller keeps in flight together with this system's (a scheduling hint for energy_async: mpmc_hint_in_flight;
	// kept here because the context is created lazily)
	void hint_in_flight(int n) { in_flight_hint_ = n < 1 ? 1 : n; }
	double energy_wait() {
		mpmc_result r;
		check(mpmc_energy_wait(ctx_, &r), "mpmc_energy_wait");
		absorb(r);
		return returned(r);
	}

	// ---- trial moves: the role of the reference's per-pair recalculate_energy cache (src/System.cpp:1211-1224) ----
	// energy of the configuration in which atoms [first, first+count) sit at new_pos ([count][3]); then accept_trial()
	// (atoms[].pos are updated to the trial positions) or reject_trial().  Needs a prior energy() of the accepted state.
	double energy_trial(int first, int count, const double *new_pos) {
		sync_state();
		check(mpmc_trial_begin(ctx_, first, count, new_pos), "mpmc_trial_begin");
		mpmc_result r;
		int rc = mpmc_trial_energy(ctx_, &r);
		if (rc != MPMC_OK) {
			mpmc_trial_reject(ctx_);
			check(rc, "mpmc_trial_energy");
		}
		trial_first_ = first, trial_kind_ = 0;
		trial_pos_.assign(new_pos, new_pos + 3 * (size_t)count);
		trial_result_ = r;
		return returned(r);
	}
	// the same in two halves, so that a driver can put the trials of many Systems in flight before the first wait
	void energy_trial_async(int first, int count, const double *new_pos) {
		sync_state();
		check(mpmc_trial_begin(ctx_, first, count, new_pos), "mpmc_trial_begin");
		int rc = mpmc_trial_energy_async(ctx_);
		if (rc != MPMC_OK) {
			mpmc_trial_reject(ctx_);
			check(rc, "mpmc_trial_energy_async");
		}
		trial_first_ = first, trial_kind_ = 0;
		trial_pos_.assign(new_pos, new_pos + 3 * (size_t)count);
	}
	double energy_trial_wait() {
		mpmc_result r;
		int rc = mpmc_trial_energy_wait(ctx_, &r);
		if (rc != MPMC_OK) {
			mpmc_trial_reject(ctx_);
			check(rc, "mpmc_trial_energy_wait");
		}
		trial_result_ = r;
		return returned(r);
	}
	const mpmc_result &trial_result() const { return trial_result_; } // the trial configuration's totals (observables keep the accepted ones)
	// ---- volume trials: System::volume_change / volume_change_Gibbs as a trial (mpmc_trial_volume_begin) ----
	// energy of the configuration with every basis element times basis_scale_factor and every molecule shifted rigidly by com * s - com, then
	// accept_trial() -- which scales pbc.basis, calls update_pbc() and shifts `atoms` with the library's expressions, so that the host list
	// equals the device's bit for bit and the next energy() uploads nothing -- or reject_trial(), which leaves both alone.  Needs a prior
	// energy() of the accepted state, masses on the atoms, and a cell whose reciprocal, volume and cutoff are update_pbc()'s own.
	// trial_result() holds the trial configuration's totals; trial_volume() its cell volume.
	double energy_trial_volume(double basis_scale_factor) {
		energy_trial_volume_async(basis_scale_factor);
		return energy_trial_wait();
	}
	void energy_trial_volume_async(double basis_scale_factor) {
		check(mpmc_trial_volume_begin(ctx_, basis_scale_factor), "mpmc_trial_volume_begin");
		trial_kind_ = 2, trial_first_ = 0, trial_scale_ = basis_scale_factor;
		trial_pos_.clear();
		exchange_enqueue();
		check(mpmc_trial_volume_get(ctx_, nullptr, nullptr, &trial_volume_, nullptr, nullptr), "mpmc_trial_volume_get");
	}
	double trial_volume() const { return trial_volume_; }
	// (diagnostics) mpmc_debug_exchange_counts and mpmc_debug_volume_trial_counts of this System's context; zeros before the first evaluation
	void trial_counts(long long exchange3[3], long long volume4[4]) const {
		for (int k = 0; k < 3; k++) exchange3[k] = 0;
		for (int k = 0; k < 4; k++) volume4[k] = 0;
		if (!ctx_) return;
		(void)mpmc_debug_exchange_counts(ctx_, exchange3);
		(void)mpmc_debug_volume_trial_counts(ctx_, volume4);
	}
	void accept_trial() {
		check(mpmc_trial_accept(ctx_), "mpmc_trial_accept");
		if (trial_kind_ == 2) { // the cell and the list follow the library's, in its arithmetic: the context is not told again
			const double s = trial_scale_;
			trial_kind_ = 0;
			if (s != 1.0) {
				for (int p = 0; p < 3; p++)
					for (int q = 0; q < 3; q++) pbc.basis[p][q] *= s;
				update_pbc();
				for (size_t a0 = 0; a0 < atoms.size();) {
					size_t a1 = a0;
					double m = 0, c[3] = {0, 0, 0};
					for (; a1 < atoms.size() && atoms[a1].molecule == atoms[a0].molecule; a1++) {
						m += atoms[a1].mass;
						for (int d = 0; d < 3; d++) c[d] += atoms[a1].mass * atoms[a1].pos[d];
					}
					for (int d = 0; d < 3; d++) {
						c[d] /= m;
						const double delta = c[d] * s - c[d];
						for (size_t k = a0; k < a1; k++) atoms[k].pos[d] += delta;
					}
					a0 = a1;
				}
			}
			absorb(trial_result_);
			return;
		}
		if (trial_kind_ > 0) { // the list follows the library's: the context is not told again
			int id = 0;
			for (const Atom &a : atoms) id = a.molecule >= id ? a.molecule + 1 : id;
			for (Atom &a : trial_mol_) a.molecule = id;
			atoms.insert(atoms.begin() + trial_first_, trial_mol_.begin(), trial_mol_.end());
			if ((int)atoms.size() > capacity_) capacity_ = (int)atoms.size(); // (the library has grown its context itself)
		} else if (trial_kind_ < 0) {
			atoms.erase(atoms.begin() + trial_first_, atoms.begin() + trial_first_ + trial_count_);
		}
		if (trial_kind_) natoms = (int)atoms.size();
		trial_kind_ = 0;
		for (size_t k = 0; k < trial_pos_.size() / 3; k++)
			for (int d = 0; d < 3; d++) atoms[trial_first_ + k].pos[d] = trial_pos_[3 * k + d];
		absorb(trial_result_);
	}
	void reject_trial() {
		check(mpmc_trial_reject(ctx_), "mpmc_trial_reject");
		trial_kind_ = 0;
	}

	// ---- exchange trials: one molecule in or out (uVT insert / remove, Gibbs transfers; mpmc_trial_insert_begin / mpmc_trial_remove_begin) ----
	// energy of the composition with the atoms of `mol` (one new molecule; their `molecule` index is not read) in front of atom `at` (a
	// molecule boundary, or atoms.size(): appended) / without the whole molecule that occupies atoms [first, first+count); then
	// accept_trial() -- which edits `atoms` accordingly (an inserted molecule gets an index no other has), so that the next energy() finds
	// the list it knows and uploads nothing -- or reject_trial().  Needs a prior energy() of the accepted state.  trial_result() holds the
	// trial composition's totals, counts and N.  Contexts with the Axilrod-Teller or disp-expansion term refuse (change `atoms`, then
	// atoms_changed()).
	double energy_trial_insert(int at, const std::vector<Atom> &mol) {
		energy_trial_insert_async(at, mol);
		return energy_trial_wait();
	}
	double energy_trial_remove(int first, int count) {
		energy_trial_remove_async(first, count);
		return energy_trial_wait();
	}
	void energy_trial_insert_async(int at, const std::vector<Atom> &mol) {
		sync_state();
		const int m = (int)mol.size();
		std::vector<double> pos(3 * (size_t)m), q(m), al(m), ep(m), sg(m), ms(m);
		std::vector<int32_t> fr(m), dp(m);
		for (int i = 0; i < m; i++) {
			const Atom &a = mol[i];
			for (int p = 0; p < 3; p++) pos[3 * i + p] = a.pos[p];
			q[i] = a.charge, al[i] = a.polarizability, ep[i] = a.epsilon, sg[i] = a.sigma, ms[i] = a.mass;
			fr[i] = a.frozen;
			dp[i] = (a.c6 != 0.0 || a.c8 != 0.0 || a.c10 != 0.0) ? 1 : 0;
		}
		check(mpmc_trial_insert_begin(ctx_, at, m, pos.data(), q.data(), al.data(), ep.data(), sg.data(), fr.data(), dp.data(), ms.data()), "mpmc_trial_insert_begin");
		trial_kind_ = +1, trial_first_ = at, trial_mol_ = mol;
		trial_pos_.clear();
		exchange_enqueue();
	}
	void energy_trial_remove_async(int first, int count) {
		sync_state();
		check(mpmc_trial_remove_begin(ctx_, first, count), "mpmc_trial_remove_begin");
		trial_kind_ = -1, trial_first_ = first, trial_count_ = count;
		trial_pos_.clear();
		exchange_enqueue();
	}

	// ---- batched insertion candidates (mpmc_insert_candidates): many poses of one species against the accepted state, one wait ----
	// poses[c][i] is the position of atom i of `species` in candidate c (the species' own `pos` is not read).  Entry c of the result is the
	// mpmc_result energy_trial_insert(atoms.size(), species at pose c) + reject_trial() would leave in trial_result(), bit for bit.  No trial
	// is opened and nothing of the accepted state changes: the chosen candidate is then inserted with energy_trial_insert / accept_trial.
	// Needs a prior energy() of the accepted state; non-polarizable boxes with the plain rd term only (the library refuses the others).
	std::vector<mpmc_result> energy_insert_candidates(const Molecule &species, const std::vector<std::vector<std::array<double, 3>>> &poses) {
		sync_state();
		const int m = (int)species.size(), n_cand = (int)poses.size();
		std::vector<double> pos(3 * (size_t)m * (size_t)n_cand), q(m), al(m), ep(m), sg(m), ms(m);
		std::vector<int32_t> fr(m), dp(m);
		for (int i = 0; i < m; i++) {
			const Atom &a = species[i];
			q[i] = a.charge, al[i] = a.polarizability, ep[i] = a.epsilon, sg[i] = a.sigma, ms[i] = a.mass;
			fr[i] = a.frozen;
			dp[i] = (a.c6 != 0.0 || a.c8 != 0.0 || a.c10 != 0.0) ? 1 : 0;
		}
		for (int c = 0; c < n_cand; c++) {
			if ((int)poses[c].size() != m) {
				last_error_ = "energy_insert_candidates: a pose has another number of atoms than the species";
				throw (int)MPMC_ERR_ARG;
			}
			for (int i = 0; i < m; i++)
				for (int p = 0; p < 3; p++) pos[3 * ((size_t)c * m + i) + p] = poses[c][i][p];
		}
		std::vector<mpmc_result> out((size_t)(n_cand > 0 ? n_cand : 0));
		check(mpmc_insert_candidates(ctx_, m, n_cand, pos.data(), q.data(), al.data(), ep.data(), sg.data(), fr.data(), dp.data(), ms.data(), out.data()),
		      "mpmc_insert_candidates");
		return out;
	}
	// the contact counts of each candidate's trial composition in the last energy_insert_candidates (mpmc_insert_candidates_contacts)
	void insert_candidates_contacts(int n_cand, std::vector<int64_t> &n_replaced, std::vector<int64_t> &n_absolute) {
		n_replaced.assign((size_t)(n_cand > 0 ? n_cand : 0), 0);
		n_absolute.assign(n_replaced.size(), 0);
		check(mpmc_insert_candidates_contacts(ctx_, n_cand, n_replaced.data(), n_absolute.data()), "mpmc_insert_candidates_contacts");
	}
	// what energy_trial_insert would RETURN for each result of the last energy_insert_candidates: its energy (the sigma rule's penalty is in
	// it), plus MAXVALUE where the absolute rule finds a contact -- or where the accepted list already trips it through unmeasured frozen pairs
	std::vector<double> insert_candidates_returned(const std::vector<mpmc_result> &results) {
		std::vector<double> e(results.size());
		for (size_t k = 0; k < results.size(); k++) e[k] = results[k].energy;
		if (!autoreject_rules_) return e;
		std::vector<int64_t> nr, na;
		insert_candidates_contacts((int)results.size(), nr, na);
		struct mpmc_cavity_autoreject_info v;
		check(mpmc_cavity_autoreject_info(ctx_, &v), "mpmc_cavity_autoreject_info");
		for (size_t k = 0; k < results.size(); k++)
			if (na[k] > 0 || v.n_unmeasured_frozen > 0) e[k] += 1.0e40;
		return e;
	}

	// ---- System::cavity_update_grid, src/System.Cavity.cpp:15-188 (the reference calls it in front of every move of a cavity_bias run) ----
	// The darts of update_cavity_volume come from the caller's generator through the distribution System::get_rand uses: three uniforms per
	// dart, dart-major, each entered as -0.5 + u; (int)(0.1 volume) of them.
	template <class Rng>
	void cavity_update_grid(Rng &rng) {
		sync_state();
		std::uniform_real_distribution<double> dist{0, 1};
		const int n_darts = mpmc_cavity_num_darts(pbc.volume);
		std::vector<double> frac(3 * (size_t)(n_darts > 0 ? n_darts : 0));
		for (size_t t = 0; t < frac.size(); t++) frac[t] = -0.5 + dist(rng);
		check(mpmc_cavity_update(ctx_, n_darts > 0 ? n_darts : 0, frac.empty() ? nullptr : frac.data(), &cavity_result), "mpmc_cavity_update");
		cavities_open = (int)cavity_result.cavities_open;
		cavity_volume = cavity_result.cavity_volume;
		cavity_bias_probability = cavity_result.probability;
	}
	// the centre of mass of a biased insertion (System::make_move, src/System.MonteCarlo.cpp:742-764): u is the caller's get_rand()
	void cavity_insertion_point(double u, double pos[3]) {
		if (cavities_open <= 0) { // (the reference takes the unbiased branch then)
			last_error_ = "cavity_insertion_point: no empty cavity";
			throw (int)MPMC_ERR_INTERNAL;
		}
		const int random_index = (cavities_open - 1) - (int)std::rint(((double)((size_t)cavities_open - 1)) * u);
		check(mpmc_cavity_point(ctx_, random_index, pos), "mpmc_cavity_point");
	}

	// the contact counts behind the last result delivered, the absolute rule's penalty and the value the reference's energy() returns
	struct mpmc_cavity_autoreject_info cavity_autoreject_info() {
		sync_state();
		struct mpmc_cavity_autoreject_info v;
		check(mpmc_cavity_autoreject_info(ctx_, &v), "mpmc_cavity_autoreject_info");
		return v;
	}
	double lj() { return piece(mpmc_lj); }
	double coulombic() { return piece(mpmc_coulombic); }
	double coulombic_real() { return piece(mpmc_coulombic_real); }
	double coulombic_reciprocal() { return piece(mpmc_coulombic_reciprocal); }
	double coulombic_self() { return piece(mpmc_coulombic_self); }
	double polar() {
		double v = piece(mpmc_polar);
		fetch_dipoles();
		return v;
	}
	void thole_field() {
		sync_state();
		std::vector<double> e(3 * atoms.size());
		check(mpmc_thole_field(ctx_, e.data()), "mpmc_thole_field");
		for (size_t i = 0; i < atoms.size(); i++)
			for (int p = 0; p < 3; p++) atoms[i].ef_static[p] = e[3 * i + p];
	}
	// rows [row0, row0+nrows) of the dense 3N x 3N matrix of System::thole_amatrix (row-major nrows x 3N)
	std::vector<double> thole_amatrix(int row0, int nrows) {
		sync_state();
		std::vector<double> a((size_t)nrows * 3 * atoms.size());
		check(mpmc_thole_amatrix(ctx_, row0, nrows, a.data()), "mpmc_thole_amatrix");
		return a;
	}

	void update_dipoles() { // atoms[].mu / ef_static / ef_induced of the last evaluation
		if (polarization && !rd_only && !use_sg && ctx_) fetch_dipoles(); // (no polarization under sg: System::energy :46)
	}

	mpmc_ctx *context() {
		sync_state();
		return ctx_;
	}

private:
	observables_t obs_;
	nodestats_t stats_;
	mpmc_ctx *ctx_ = nullptr;
	int in_flight_hint_ = 1;
	int capacity_ = 0;
	bool atoms_dirty_ = true, box_dirty_ = true;
	bool three_body_on_ = false; // what the context's three-body setting is (sync_state)
	int three_body_mk_ = 0;
	bool disp_on_ = false; // what the context's disp-expansion setting is (sync_state)
	int disp_flags_ = 0;
	int polar_wolf_on_ = 0, polar_palmo_on_ = 0; // what the context's Wolf-field / Palmo settings are (sync_state)
	int on_demand_on_ = 0;                       // ... and its dipoles-on-demand switch
	int rd_crystal_on_ = 0, rd_crystal_order_ = 0; // ... and its rd_crystal setting
	int ewald_full_on_ = 0, ewald_full_flags_ = 0; // ... and its polar_ewald_full setting
	int rd_model_form_ = 0, rd_model_mixing_ = 0;  // ... and its rd model
	int sg_on_ = 0;                                // ... and its Silvera-Goldman switch
	int relax_scheme_ = 0, zodid_on_ = 0;          // ... and its polar_sor / polar_esor / polar_zodid setting
	int gs_ranked_on_ = 0;                         // ... and its polar_gs_ranked setting
	int cavity_grid_ = 0;                          // ... and its cavity grid (0: off)
	int autoreject_rules_ = 0;                     // ... and its cavity_autoreject setting
	double autoreject_scale_ = 0, autoreject_repulsion_ = 0;
	// what energy() returns: the observables' energy, plus the absolute rule's penalty when a rule is on (no device work: the info of the
	// result just delivered)
	double returned(const mpmc_result &r) {
		if (!autoreject_rules_) return r.energy;
		struct mpmc_cavity_autoreject_info v;
		check(mpmc_cavity_autoreject_info(ctx_, &v), "mpmc_cavity_autoreject_info");
		return v.returned_energy;
	}
	double cavity_radius_ = 0;
	double polar_wolf_alpha_ = 0;
	int trial_first_ = 0;
	int trial_kind_ = 0, trial_count_ = 0; // the open trial: 0 a displacement, +1 an insertion (trial_mol_), -1 a removal, 2 a volume change (trial_scale_)
	double trial_scale_ = 1.0, trial_volume_ = 0.0;
	std::vector<Atom> trial_mol_;
	void exchange_enqueue() {
		const int rc = mpmc_trial_energy_async(ctx_);
		if (rc != MPMC_OK) {
			mpmc_trial_reject(ctx_);
			trial_kind_ = 0;
			check(rc, "mpmc_trial_energy_async");
		}
	}
	std::vector<double> trial_pos_;
	mpmc_result trial_result_{};

	void check(int rc, const char *what) {
		if (rc == MPMC_OK) return;
		last_error_ = std::string(what) + ": " + (ctx_ ? mpmc_last_error(ctx_) : mpmc_last_error(nullptr));
		throw (rc > 0 ? rc : (int)MPMC_ERR_INTERNAL); // reference convention: throw <int>
	}

	void sync_state() {
		if (polar_gs && polar_gs_ranked) { // an input error of the reference (SimulationControl.cpp:2732), found before anything reaches the device
			last_error_ = "polar_gs and polar_gs_ranked are both on";
			throw 3000;
		}
		natoms = countNatoms();
		const int n = natoms;
		if (!ctx_ || capacity_ < n) {
			if (ctx_) mpmc_ctx_destroy(ctx_);
			ctx_ = nullptr;
			capacity_ = n + n / 4 + 64;
			check(mpmc_ctx_create(device, capacity_, &ctx_), "mpmc_ctx_create");
			atoms_dirty_ = box_dirty_ = true;
			polar_wolf_on_ = polar_palmo_on_ = on_demand_on_ = 0; // (a new context starts with all of them off)
			polar_wolf_alpha_ = 0;
			rd_crystal_on_ = rd_crystal_order_ = 0;
			ewald_full_on_ = ewald_full_flags_ = 0;
			rd_model_form_ = rd_model_mixing_ = 0;
			sg_on_ = 0;
			relax_scheme_ = zodid_on_ = 0;
			gs_ranked_on_ = 0;
			cavity_grid_ = 0;
			cavity_radius_ = 0;
			autoreject_rules_ = 0;
			autoreject_scale_ = autoreject_repulsion_ = 0;
		}
		if (box_dirty_) {
			// a cell whose reciprocal, volume and cutoff are PeriodicBoundary::update's own goes over as the basis alone: the library computes
			// the same bits from it, and only a cell without overrides can be scaled by a volume trial
			double R[9], vol = 0, cut = 0;
			const bool own = mpmc_pbc_compute(&pbc.basis[0][0], R, &vol, &cut) == MPMC_OK && std::memcmp(R, &pbc.reciprocal_basis[0][0], sizeof(R)) == 0 &&
			                 vol == pbc.volume && cut == pbc.cutoff;
			if (own) check(mpmc_set_box(ctx_, &pbc.basis[0][0], nullptr, 0.0, 0.0), "mpmc_set_box");
			else check(mpmc_set_box(ctx_, &pbc.basis[0][0], &pbc.reciprocal_basis[0][0], pbc.volume, pbc.cutoff), "mpmc_set_box");
			box_dirty_ = false;
		}
		mpmc_options o;
		mpmc_default_options(&o);
		o.rd_only = rd_only;
		o.rd_lrc = rd_lrc;
		o.polarization = polarization;
		o.polar_iterative = polar_iterative;
		o.polar_ewald = polar_ewald;
		o.polar_max_iter = polar_max_iter;
		o.polar_gs = polar_gs;
		o.polar_rrms = polar_rrms;
		o.damp_type = damp_type;
		o.ewald_kmax = ewald_kmax;
		o.solver = solver;
		o.wolf = wolf;
		o.feynman_hibbs = feynman_hibbs;
		o.feynman_hibbs_order = feynman_hibbs_order;
		o.temperature = temperature;
		o.polar_precision = polar_precision;
		o.polar_gamma = polar_gamma;
		o.polar_damp = polar_damp;
		// (an alpha that update_pbc() derived from the cutoff is left to the library, which derives the same bits from the same cutoff -- and
		// goes on doing so for the cell of a volume trial, as update_pbc() does after a volume change)
		o.ewald_alpha = (ewald_alpha_set != 1 && ewald_alpha == 3.5 / pbc.cutoff) ? 0.0 : ewald_alpha;
		o.polar_ewald_alpha = (polar_ewald_alpha_set != 1 && polar_ewald_alpha == 3.5 / pbc.cutoff) ? 0.0 : polar_ewald_alpha;
		// (polar_iterative off is the library's direct dipole solve: no flag; `rd_crystal on` goes to mpmc_set_rd_crystal below: the reader's
		// flag for the keyword is cleared here, a caller's flag without the field is still refused)
		// (`polar_ewald_full on` likewise, to mpmc_set_polar_ewald_full, `polar_gs_ranked on` to mpmc_set_polar_gs_ranked and
		// `cavity_autoreject on` / `cavity_autoreject_absolute on` to mpmc_set_cavity_autoreject)
		o.unsupported_flags = unsupported_flags & ~(uint64_t)((rd_crystal ? MPMC_FLAG_RD_CRYSTAL : 0) | (polar_ewald_full ? MPMC_FLAG_POLAR_EWALD_FULL : 0) |
		                                                      (polar_gs_ranked ? MPMC_FLAG_POLAR_GS_RANKED : 0) |
		                                                      (cavity_autoreject_rules() ? MPMC_FLAG_CAVITY_AUTOREJECT : 0));
		check(mpmc_set_options(ctx_, &o), "mpmc_set_options");
		if (atoms_dirty_) {
			std::vector<double> pos(3 * (size_t)n), q(n), al(n), ep(n), sg(n), ms(n);
			std::vector<int32_t> mol(n), fr(n), dp(n);
			for (int i = 0; i < n; i++) {
				const Atom &a = atoms[i];
				for (int p = 0; p < 3; p++) pos[3 * i + p] = a.pos[p];
				q[i] = a.charge;
				al[i] = a.polarizability;
				ep[i] = a.epsilon;
				sg[i] = a.sigma;
				ms[i] = a.mass;
				mol[i] = a.molecule;
				fr[i] = a.frozen;
				dp[i] = (a.c6 != 0.0 || a.c8 != 0.0 || a.c10 != 0.0) ? 1 : 0;
			}
			check(mpmc_set_atoms(ctx_, n, pos.data(), q.data(), al.data(), ep.data(), sg.data(), mol.data(), fr.data(), dp.data(), ms.data()),
			      "mpmc_set_atoms");
			atoms_dirty_ = false;
			three_body_on_ = false; // (the library discards the coefficients with the atom list)
			disp_on_ = false;
		}
		// the three-body term after every upload of the atoms, and whenever the switch changed
		if (using_axilrod_teller != three_body_on_ || (using_axilrod_teller && midzuno_kihara_approx != three_body_mk_)) {
			std::vector<double> c6(n), c9(n);
			for (int i = 0; i < n; i++) c6[i] = atoms[i].c6, c9[i] = atoms[i].c9;
			check(mpmc_set_axilrod_teller(ctx_, using_axilrod_teller ? 1 : 0, midzuno_kihara_approx, c6.data(), c9.data()), "mpmc_set_axilrod_teller");
			three_body_on_ = using_axilrod_teller;
			three_body_mk_ = midzuno_kihara_approx;
		}
		// the disp-expansion term likewise
		const int dflags = (damp_dispersion ? MPMC_DISP_DAMP : 0) | (extrapolate_disp_coeffs ? MPMC_DISP_EXTRAPOLATE_C10 : 0) | (schmidt_ff ? MPMC_DISP_SCHMIDT : 0);
		if (using_disp_expansion != disp_on_ || (using_disp_expansion && dflags != disp_flags_)) {
			std::vector<double> c6(n), c8(n), c10(n);
			for (int i = 0; i < n; i++) c6[i] = atoms[i].c6, c8[i] = atoms[i].c8, c10[i] = atoms[i].c10;
			check(mpmc_set_disp_expansion(ctx_, using_disp_expansion ? 1 : 0, dflags, c6.data(), c8.data(), c10.data()), "mpmc_set_disp_expansion");
			disp_on_ = using_disp_expansion;
			disp_flags_ = dflags;
		}
		// the Wolf static field and the Palmo-Krimm correction: switches of the context that outlive atom lists, set when they change
		if ((polar_wolf != 0) != (polar_wolf_on_ != 0) || (polar_wolf && polar_wolf_alpha != polar_wolf_alpha_)) {
			check(mpmc_set_polar_wolf(ctx_, polar_wolf ? 1 : 0, polar_wolf_alpha), "mpmc_set_polar_wolf");
			polar_wolf_on_ = polar_wolf ? 1 : 0;
			polar_wolf_alpha_ = polar_wolf_alpha;
		}
		if ((rd_crystal != 0) != (rd_crystal_on_ != 0) || (rd_crystal && rd_crystal_order != rd_crystal_order_)) {
			check(mpmc_set_rd_crystal(ctx_, rd_crystal ? 1 : 0, rd_crystal_order), "mpmc_set_rd_crystal");
			rd_crystal_on_ = rd_crystal ? 1 : 0;
			rd_crystal_order_ = rd_crystal_order;
		}
		if (rd_model_form() != rd_model_form_ || rd_model_mixing() != rd_model_mixing_) {
			check(mpmc_set_rd_model(ctx_, rd_model_form(), rd_model_mixing()), "mpmc_set_rd_model");
			rd_model_form_ = rd_model_form();
			rd_model_mixing_ = rd_model_mixing();
		}
		if ((use_sg != 0) != (sg_on_ != 0)) {
			check(mpmc_set_silvera_goldman(ctx_, use_sg ? 1 : 0), "mpmc_set_silvera_goldman");
			sg_on_ = use_sg ? 1 : 0;
		}
		const int pef_flags = polar_ewald_full_vector_kweight ? MPMC_PEF_VECTOR_KWEIGHT : 0;
		if ((polar_ewald_full != 0) != (ewald_full_on_ != 0) || (polar_ewald_full && pef_flags != ewald_full_flags_)) {
			check(mpmc_set_polar_ewald_full(ctx_, polar_ewald_full ? 1 : 0, pef_flags), "mpmc_set_polar_ewald_full");
			ewald_full_on_ = polar_ewald_full ? 1 : 0;
			ewald_full_flags_ = pef_flags;
		}
		if (polar_sor && polar_esor) { // (SimulationControl.cpp:2714-2730)
			last_error_ = "polar_sor and polar_esor are both on";
			throw (int)MPMC_ERR_INCOMPATIBLE;
		}
		const int relax_scheme = polar_sor ? MPMC_POLAR_RELAX_SOR : polar_esor ? MPMC_POLAR_RELAX_ESOR : MPMC_POLAR_RELAX_NONE;
		if (relax_scheme != relax_scheme_ || (polar_zodid != 0) != (zodid_on_ != 0)) {
			check(mpmc_set_polar_relax(ctx_, relax_scheme, polar_zodid ? 1 : 0), "mpmc_set_polar_relax");
			relax_scheme_ = relax_scheme;
			zodid_on_ = polar_zodid ? 1 : 0;
		}
		if ((polar_gs_ranked != 0) != (gs_ranked_on_ != 0)) {
			check(mpmc_set_polar_gs_ranked(ctx_, polar_gs_ranked ? 1 : 0), "mpmc_set_polar_gs_ranked");
			gs_ranked_on_ = polar_gs_ranked ? 1 : 0;
		}
		// (cavity_bias on with a grid size or radius that is not positive is refused by the library, SimulationControl.cpp:2157-2162)
		if (cavity_bias ? (cavity_grid_ == 0 || cavity_grid_size != cavity_grid_ || cavity_radius != cavity_radius_) : cavity_grid_ != 0) {
			if (cavity_bias && cavity_grid_size == 0) {
				last_error_ = "cavity_bias is on and cavity_grid_size is 0";
				throw (int)MPMC_ERR_INVALID_SETTING;
			}
			check(mpmc_set_cavity_grid(ctx_, cavity_bias ? cavity_grid_size : 0, cavity_radius), "mpmc_set_cavity_grid");
			cavity_grid_ = cavity_bias ? cavity_grid_size : 0;
			cavity_radius_ = cavity_radius;
		}
		// (a scale outside (0, 1] with a rule on is refused by the library, SimulationControl.cpp:2139-2154)
		const int ca_rules = cavity_autoreject_rules();
		if (ca_rules != autoreject_rules_ || (ca_rules && (cavity_autoreject_scale != autoreject_scale_ || cavity_autoreject_repulsion != autoreject_repulsion_))) {
			check(mpmc_set_cavity_autoreject(ctx_, ca_rules, cavity_autoreject_scale, cavity_autoreject_repulsion), "mpmc_set_cavity_autoreject");
			autoreject_rules_ = ca_rules;
			autoreject_scale_ = cavity_autoreject_scale;
			autoreject_repulsion_ = cavity_autoreject_repulsion;
		}
		if ((polar_palmo != 0) != (polar_palmo_on_ != 0)) {
			check(mpmc_set_polar_palmo(ctx_, polar_palmo ? 1 : 0), "mpmc_set_polar_palmo");
			polar_palmo_on_ = polar_palmo ? 1 : 0;
		}
		if ((dipoles_on_demand != 0) != (on_demand_on_ != 0)) {
			check(mpmc_set_dipoles_on_demand(ctx_, dipoles_on_demand ? 1 : 0), "mpmc_set_dipoles_on_demand");
			on_demand_on_ = dipoles_on_demand ? 1 : 0;
		}
	}

	void fetch_dipoles() {
		const size_t n = atoms.size();
		std::vector<double> mu(3 * n), e0(3 * n), ei(3 * n);
		check(mpmc_get_dipoles(ctx_, mu.data(), e0.data(), ei.data()), "mpmc_get_dipoles");
		for (size_t i = 0; i < n; i++)
			for (int p = 0; p < 3; p++) {
				atoms[i].mu[p] = mu[3 * i + p];
				atoms[i].ef_static[p] = e0[3 * i + p];
				atoms[i].ef_induced[p] = ei[3 * i + p];
			}
	}

	void absorb(const mpmc_result &r) {
		last_result = r;
		obs_.energy = r.energy;
		obs_.coulombic_energy = r.coulombic_energy;
		obs_.rd_energy = r.rd_energy;
		obs_.polarization_energy = r.polarization_energy;
		obs_.vdw_energy = r.vdw_energy;
		obs_.three_body_energy = r.three_body_energy;
		obs_.dipole_rrms = r.dipole_rrms;
		obs_.N = r.N;
		obs_.NU = r.NU;
		stats_.polarization_iterations = (double)r.polar_iterations;
		iterator_failed = r.iterator_failed;
		last_volume = pbc.volume;
		if (polarization && !rd_only && !use_sg && eager_dipoles) fetch_dipoles();
	}

	double piece(int (*fn)(mpmc_ctx *, double *)) {
		sync_state();
		double v = 0;
		check(fn(ctx_, &v), "component");
		return v;
	}

public:
	std::string last_error_;
};

// SimulationControl's multi-System part for ensemble pi_nvt (src/SimulationControl.h:60, PathIntegral.cpp:752-805).
// `systems` holds the beads owned by THIS process; `nSys` is the Trotter number P over all processes.
// The cross-process exchange of 4 doubles per bead (MPI_Allgather x4 in the reference) is delegated to
// `allgather`: it receives this process's per-bead values (n_local x stride, local order; stride = 4 for the
// potential, 3 * n_molecules for the centres of mass of the kinetic estimator) and must return all P x stride
// values in bead order.  With one process it may be left empty.
// (The reference keeps all P images on every MPI rank, so its kinetic estimator needs no exchange; with the beads
// sharded over ranks the ring of adjacent images crosses ranks and the centres of mass are gathered once per call.)
// one image's share of a loop that may run under OpenMP: the facade reports errors by throwing an int, and an exception must not
// leave a parallel region -- the first one is kept and thrown again behind the loop
template <class F>
inline void each_image_guarded(int &first_error, F &&body) {
	try {
		body();
	} catch (int e) {
#ifdef _OPENMP
#pragma omp critical(mpmc_image_error)
#endif
		if (!first_error) first_error = e;
	}
}

template <class SystemT>
class PathIntegralEnsembleT {
public:
	std::vector<SystemT *> systems;
	int nSys = 0;
	double temperature = 0;        // sys.temperature
	observables_t sys_observables; // the aggregate "sys.observables" of the reference
	std::function<std::vector<double>(const std::vector<double> &)> allgather;

	// one process per GPU: the exchange runs on RCCL inside libmpmc_energy.so (mpmc_pi_gather_beads: ONE ncclAllGather per call, the
	// reference's 4 x MPI_Allgather, PathIntegral.cpp:763-766).  `comm` comes from mpmc_comm_init_rank; nSys = P over all ranks.
	void use_comm(mpmc_comm *comm) {
		allgather = [this, comm](const std::vector<double> &mine) {
			const int n_local = (int)systems.size();
			int n_ranks = 1;
			(void)mpmc_comm_info(comm, &n_ranks, nullptr, nullptr);
			const int stride = n_local > 0 ? (int)(mine.size() / (size_t)n_local) : 0;
			std::vector<double> all((size_t)n_ranks * mine.size());
			const int rc = mpmc_pi_gather_beads(comm, mine.data(), n_local, stride, all.data());
			if (rc != MPMC_OK) throw rc;
			return all;
		};
	}

	// PI_calculate_potential for a TRIAL configuration in which atoms [first, first+count) of every image sit at new_pos[image]:
	// per-move delta energies behind the same aggregate (every image enqueued before the first wait); the Systems keep the accepted
	// configuration until accept_trial() / reject_trial()
	double PI_trial_potential(int first, int count, const std::vector<std::vector<double>> &new_pos) {
		const int n_local = (int)systems.size();
		int err_img = 0;
		// The images' enqueues are independent (one context, one stream each) and a trial is bound by the host's HIP calls, not by the GPU:
		// built with -fopenmp the images are enqueued by a few threads, as the reference's own bead loop is (PathIntegral.cpp:759-775);
		// without it this is the plain loop.  The waits and the sums below stay in image order: the result does not depend on threads.
#ifdef _OPENMP
#pragma omp parallel for schedule(static) num_threads(n_local < 4 ? n_local : 4) if (n_local > 1)
#endif
		for (int b = 0; b < n_local; b++) each_image_guarded(err_img, [&] { systems[b]->energy_trial_async(first, count, new_pos[b].data()); });
		if (err_img) throw err_img;
		std::vector<double> mine(4 * (size_t)n_local);
		for (int b = 0; b < n_local; b++) {
			systems[b]->energy_trial_wait();
			const mpmc_result &r = systems[b]->trial_result();
			mine[4 * b + 0] = r.rd_energy;
			mine[4 * b + 1] = r.coulombic_energy;
			mine[4 * b + 2] = r.polarization_energy;
			mine[4 * b + 3] = r.vdw_energy;
		}
		const std::vector<double> all = allgather ? allgather(mine) : mine;
		const int P = nSys ? nSys : n_local;
		double acc[4] = {0, 0, 0, 0};
		for (int s = 0; s < P; s++)
			for (int k = 0; k < 4; k++) acc[k] += all[4 * (size_t)s + k];
		for (int k = 0; k < 4; k++) acc[k] /= P;
		sys_observables.rd_energy = acc[0];
		sys_observables.coulombic_energy = acc[1];
		sys_observables.polarization_energy = acc[2];
		sys_observables.vdw_energy = acc[3];
		return acc[0] + acc[1] + acc[3] + acc[2];
	}

	// SimulationControl::PI_calculate_energy, PathIntegral.cpp:734-749
	double PI_calculate_energy() {
		const double kinetic = PI_calculate_kinetic();
		const double potential = PI_calculate_potential();
		sys_observables.energy = kinetic + potential;
		return sys_observables.energy;
	}

	// SimulationControl::PI_calculate_kinetic, PathIntegral.cpp:806-824
	double PI_calculate_kinetic() {
		const double N = (double)systems.at(0)->countN();
		const int P = nSys ? nSys : (int)systems.size();
		const double chain_mass_len2 = PI_chain_mass_length2_ENTIRE_SYSTEM();
		const double orient_mu_len2 = PI_orientational_mu_length2_ENTIRE_SYSTEM();
		sys_observables.N = N;
		sys_observables.kinetic_energy = mpmc_pi_kinetic(chain_mass_len2, orient_mu_len2, N, P, temperature);
		return sys_observables.kinetic_energy;
	}

	// SimulationControl::PI_chain_mass_length2_ENTIRE_SYSTEM, PathIntegral.cpp:851-896
	double PI_chain_mass_length2_ENTIRE_SYSTEM() {
		std::vector<double> com, mass;
		std::vector<int32_t> movable;
		const int nmol = gather_coms(com, mass, movable);
		const int P = nSys ? nSys : (int)systems.size();
		return mpmc_pi_chain_mass_length2(P, nmol, com.data(), mass.data(), movable.data());
	}
	// SimulationControl::PI_chain_mass_length2() for one chain, PathIntegral.cpp:897-965 (`molecule` plays the part of
	// checkpoint->molecule_altered: the index of the molecule whose bead chain was perturbed)
	double PI_chain_mass_length2(int molecule) {
		std::vector<double> com, mass;
		std::vector<int32_t> movable;
		const int nmol = gather_coms(com, mass, movable);
		if (molecule < 0 || molecule >= nmol) throw (int)MPMC_ERR_ARG;
		const int P = nSys ? nSys : (int)systems.size();
		std::vector<double> one(3 * (size_t)P);
		for (int s = 0; s < P; s++)
			for (int d = 0; d < 3; d++) one[3 * s + d] = com[3 * ((size_t)s * nmol + molecule) + d];
		return mpmc_pi_chain_mass_length2(P, 1, one.data(), &mass[molecule], nullptr);
	}
	double PI_orientational_mu_length2_ENTIRE_SYSTEM() { return 0.0; } // PathIntegral.cpp:970-972

private:
	int gather_coms(std::vector<double> &com, std::vector<double> &mass, std::vector<int32_t> &movable) {
		std::vector<double> mine, c, m0;
		std::vector<int32_t> mv;
		for (size_t b = 0; b < systems.size(); b++) {
			systems[b]->molecule_coms(c, b == 0 ? mass : m0, b == 0 ? movable : mv);
			mine.insert(mine.end(), c.begin(), c.end());
		}
		com = allgather ? allgather(mine) : mine;
		return (int)mass.size();
	}

public:

	double PI_calculate_potential() {
		const int n_local = (int)systems.size();
		int err_img = 0;
		// every bead enqueued on its own stream before the first wait (by a few threads when built with -fopenmp, see PI_trial_potential)
#ifdef _OPENMP
#pragma omp parallel for schedule(static) num_threads(n_local < 4 ? n_local : 4) if (n_local > 1)
#endif
		for (int b = 0; b < n_local; b++)
			each_image_guarded(err_img, [&] {
				systems[b]->hint_in_flight(n_local);
				systems[b]->energy_async();
			});
		if (err_img) throw err_img;
		std::vector<double> mine(4 * (size_t)n_local);
		for (int b = 0; b < n_local; b++) {
			systems[b]->energy_wait();
			const observables_t *o = systems[b]->observables;
			mine[4 * b + 0] = o->rd_energy;
			mine[4 * b + 1] = o->coulombic_energy;
			mine[4 * b + 2] = o->polarization_energy;
			mine[4 * b + 3] = o->vdw_energy;
		}
		const std::vector<double> all = allgather ? allgather(mine) : mine;
		const int P = nSys ? nSys : n_local;
		double acc[4] = {0, 0, 0, 0};
		for (int s = 0; s < P; s++) // ordered sum, :791-796
			for (int k = 0; k < 4; k++) acc[k] += all[4 * (size_t)s + k];
		for (int k = 0; k < 4; k++) acc[k] /= P; // :798-801
		sys_observables.rd_energy = acc[0];
		sys_observables.coulombic_energy = acc[1];
		sys_observables.polarization_energy = acc[2];
		sys_observables.vdw_energy = acc[3];
		return acc[0] + acc[1] + acc[3] + acc[2]; // :803-804
	}
};
using PathIntegralEnsemble = PathIntegralEnsembleT<System>;

} // namespace mpmc
