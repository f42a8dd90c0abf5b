/* include/mpmc_energy.h -- C ABI of the MI355X-native energy hot path (libmpmc_energy.so).
 *
 * This is the drop-in boundary for ONE path of b-tudor/mpmcxx: the per-move potential-energy
 * evaluation `double System::energy()` (reference src/System.h:315, src/System.Energy.cpp:19-171) and the
 * path-integral per-bead loop around it (src/SimulationControl.PathIntegral.cpp:752-805).
 * A reference-side adapter flattens the System's Molecule->Atom lists into the arrays below, calls
 * mpmc_energy(), and copies mpmc_result into System::observables.
 *
 * Conventions
 *  - plain C, no C++/torch types; all floating point is IEEE fp64; energies in Kelvin, lengths in Angstrom,
 *    charges in reduced units sqrt(K*A) (e * 408.7816, reference src/System.cpp:624).
 *  - every entry point returns MPMC_OK (0) or a negative/positive error code; mpmc_last_error() gives text.
 *    Codes reuse the reference's throw-int values where one exists (src/constants.h:108-147).
 *  - a context is the device-side state of ONE System (one box / one PI bead): its own HIP stream and
 *    device buffers.  Re-entrant per context (the reference calls energy() concurrently from P threads on P
 *    distinct Systems, PathIntegral.cpp:772-779); never call concurrently on the same context.
 *  - host pointers unless a name says _device.
 *  - there is NO CPU fallback: without a usable HIP device mpmc_ctx_create fails with MPMC_ERR_NO_DEVICE.
 */
#ifndef MPMC_ENERGY_H
#define MPMC_ENERGY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPMC_ABI_VERSION 6

/* ---- status codes -------------------------------------------------------------------------------------- */
#define MPMC_OK 0
#define MPMC_ERR_INTERNAL 101            /* reference internal_error (constants.h:110)                    */
#define MPMC_ERR_MEMORY 2000             /* memory_request_fail                                           */
#define MPMC_ERR_INVALID_SETTING 4000    /* invalid_setting                                               */
#define MPMC_ERR_INCOMPATIBLE 4002       /* incompatible_settings                                         */
#define MPMC_ERR_UNSUPPORTED 4004        /* unsupported_setting: physics outside the hot path */
#define MPMC_ERR_INVALID_DATUM 6001      /* invalid_datum (bad atom arrays)                               */
#define MPMC_ERR_BOX 6004                /* invalid_box_dimensions                                        */
#define MPMC_ERR_INVALID_MC_MOVE 20000   /* internal_err_invalid_mc_move: the two boxes of a coordinated move disagree (constants.h:147) */
#define MPMC_ERR_INVALID_MC_MOVE_KIND 102 /* invalid_monte_carlo_move (constants.h:110)                  */
#define MPMC_ERR_NO_DEVICE (-1)          /* no HIP device / HIP runtime failure at create                 */
#define MPMC_ERR_HIP (-2)                /* a HIP call failed (text in mpmc_last_error)                   */
#define MPMC_ERR_ARG (-3)                /* NULL / out-of-range argument                                  */
#define MPMC_ERR_COMM (-4)               /* RCCL missing or an RCCL call failed (text in mpmc_comm_last_error) */

/* ---- damping (reference enum constants.h:66-70) -------------------------------------------------------- */
#define MPMC_DAMPING_OFF 0
#define MPMC_DAMPING_LINEAR 1
#define MPMC_DAMPING_EXPONENTIAL 2

/* ---- how the Thole dipole iteration is executed on the device (not a reference option) ------------------ */
#define MPMC_SOLVER_AUTO 0         /* COMPACT when its store fits, else MATRIX_FREE                         */
#define MPMC_SOLVER_MATRIX_FREE 1  /* nothing stored: the damped tensors are rebuilt from the positions in every
                                    * iteration by the same symmetric kernel (7 % slower, 20x less memory)       */
#define MPMC_SOLVER_COMPACT 2      /* store (d1/r^3, 3 d2/r^5) per unordered pair, 16 B/pair (HBM-bound)      */
#define MPMC_SOLVER_DENSE 3        /* the reference's dense 3N x 3N A matrix in device memory, contraction on the
                                    * fp64 matrix cores; on request only (HBM-bound at 9x the bytes of COMPACT)  */

/* ---- out-of-scope reference switches: pass the ones that are ON so the library can refuse them ---------- */
#define MPMC_FLAG_WOLF (1ull << 0)          /* (now supported: mpmc_options.wolf; the bit stays for ABI stability) */
#define MPMC_FLAG_FEYNMAN_HIBBS (1ull << 1) /* (now supported: mpmc_options.feynman_hibbs) */
#define MPMC_FLAG_RD_CRYSTAL (1ull << 2)
#define MPMC_FLAG_SPECTRE (1ull << 3)
#define MPMC_FLAG_GWP (1ull << 4)
#define MPMC_FLAG_USE_SG (1ull << 5)
#define MPMC_FLAG_POLARVDW (1ull << 6)
#define MPMC_FLAG_POLAR_EWALD_FULL (1ull << 7)
#define MPMC_FLAG_POLAR_WOLF (1ull << 8)
#define MPMC_FLAG_POLAR_PALMO (1ull << 9)
#define MPMC_FLAG_POLAR_GS_RANKED (1ull << 10)
#define MPMC_FLAG_POLAR_SOR (1ull << 11)
#define MPMC_FLAG_POLAR_ZODID (1ull << 12)
#define MPMC_FLAG_NON_LB_MIXING (1ull << 13) /* cdvdw_* mixing; waldmanhagler / halgren_mixing / c6_mixing too when passed here -- still refused:
                                              * those three are switched on by mpmc_set_rd_model alone */
#define MPMC_FLAG_OTHER_RD (1ull << 14)      /* rd_anharmonic / cdvdw_exp_repulsion / disp_expansion_mbvdw; dreiding / lj_buffered_14_7 too when
                                              * passed here -- still refused: those two are switched on by mpmc_set_rd_model alone */
#define MPMC_FLAG_AXILROD_TELLER (1ull << 15) /* still refused here: the term is switched on by mpmc_set_axilrod_teller alone */
#define MPMC_FLAG_CAVITY_AUTOREJECT (1ull << 16)
#define MPMC_FLAG_POLAR_MATRIX_INVERSION (1ull << 17) /* polarization on with polar_iterative off (now supported: the direct solve
                                                       * below; the bit is accepted and ignored, polar_iterative == 0 selects the path) */

typedef struct mpmc_ctx mpmc_ctx; /* opaque: device buffers + stream of one System */

/* Options = the reference keywords that steer energy() (src/SimulationControl.cpp line in comment) */
typedef struct mpmc_options {
	int32_t rd_only;          /* :977  skip electrostatics + polarization                                   */
	int32_t rd_lrc;           /* :1003 LJ long-range correction (default on)                                */
	int32_t polarization;     /* :653                                                                       */
	int32_t polar_iterative;  /* :1240 on: Jacobi / Gauss-Seidel sweeps; off (the reference's default): the direct solve  */
	int32_t polar_ewald;      /* :718/:1210 static field by Ewald (recip_term + real_term) instead of nopbc */
	int32_t polar_max_iter;   /* :1303 fixed iteration count when polar_precision == 0                      */
	int32_t polar_gs;         /* :1256 Gauss-Seidel: in-place sweeps in atom order (serial over 64-atom tiles)  */
	int32_t polar_rrms;       /* :1320 compute per-atom dipole RRMS every iteration                         */
	int32_t damp_type;        /* :1308 must be MPMC_DAMPING_EXPONENTIAL when polarization is on             */
	int32_t ewald_kmax;       /* :1199 (default 7)                                                          */
	int32_t solver;           /* MPMC_SOLVER_*                                                              */
	int32_t wolf;             /* :994  Wolf electrostatics instead of Ewald in coulombic() (coulombic_wolf :1420-1462) */
	double polar_precision;   /* :1298 0 => fixed count; else stop when every |d mu| < precision*DEBYE2SKA  */
	double polar_gamma;       /* :1288 pre-scaling of the initial dipoles (default 1.0)                     */
	double polar_damp;        /* :1293 Thole exponential damping length parameter                           */
	double ewald_alpha;       /* :1192 <= 0 means "unset": 3.5 / cutoff (System.cpp:871-872)                 */
	double polar_ewald_alpha; /* :1218 <= 0 means "unset": 3.5 / cutoff (System.cpp:873-874)                 */
	uint64_t unsupported_flags; /* OR of MPMC_FLAG_* that are ON in the caller's System                     */
	int32_t feynman_hibbs;       /* :1042 Feynman-Hibbs corrections to lj() and coulombic_real() (:1100-1148, :1521-1557) */
	int32_t feynman_hibbs_order; /* :1067 2 or 4 (anything else: 2, SimulationControl.cpp:2497-2500)           */
	double temperature;          /* K; needed by Feynman-Hibbs (needs atom masses in mpmc_set_atoms)           */
} mpmc_options;

/* what energy() leaves in System::observables / nodestats (src/System.h:94-113,151-185) + parity diagnostics */
typedef struct mpmc_result {
	double energy;              /* observables->energy  = rd + coulombic + polarization + vdw + three_body  */
	double rd_energy;           /* observables->rd_energy            (lj(): pairs + pair LRC + self LRC)    */
	double coulombic_energy;    /* observables->coulombic_energy     (real + reciprocal + self)             */
	double polarization_energy; /* observables->polarization_energy  (-1/2 sum mu.E0)                       */
	double vdw_energy;          /* always 0 (polarvdw is out of scope)                                      */
	double three_body_energy;   /* observables->three_body_energy: Axilrod-Teller (mpmc_set_axilrod_teller), else 0 */
	double kinetic_energy;      /* always 0 (gwp out of scope)                                              */
	double es_real;             /* coulombic_real()                                                         */
	double es_recip;            /* coulombic_reciprocal()                                                   */
	double es_self;             /* coulombic_self()                                                         */
	double lj_pairs;            /* sum of pair->rd_energy                                                   */
	double lrc_pair;            /* sum of pair->lrc                                                         */
	double lrc_self;            /* sum of lj_lrc_self (disp-expansion: of disp_expansion_lrc_self)          */
	double dipole_rrms;         /* observables->dipole_rrms                                                 */
	double N;                   /* observables->N  (non-frozen molecules, countN System.cpp:909-931)        */
	double NU;                  /* observables->NU = N * energy                                             */
	int64_t n_pairs;            /* N(N-1)/2                                                                 */
	int64_t n_lj_in_cutoff;     /* pairs passing  rimg-1e-12 < rc && !rd_excluded && !frozen                */
	int64_t n_es_in_cutoff;     /* pairs passing  !frozen && !(rimg > rc || es_excluded)                    */
	int64_t n_intra;            /* same-molecule pairs                                                      */
	int64_t n_rd_excluded;
	int64_t n_es_excluded;
	int64_t n_frozen;           /* pairs with both atoms frozen                                             */
	int32_t polar_iterations;   /* nodestats->polarization_iterations                                       */
	int32_t iterator_failed;    /* System::iterator_failed (=> caller rejects the move)                      */
} mpmc_result;

/* accumulated device time of the kernels of one context, measured with HIP events on the context's stream
 * (only while profiling is enabled with mpmc_set_profiling).  Index with MPMC_K_*. */
#define MPMC_K_PAIR 0        /* LJ + real-space Coulomb pair kernel; the disp-expansion, rd_crystal and rd-model sums / trial differences too */
#define MPMC_K_RECIP 1       /* structure factors + reciprocal energy + atom terms  */
#define MPMC_K_FIELD 2       /* static field (recip + real, or nopbc)               */
#define MPMC_K_TENSOR 3      /* dense thole_amatrix rows (mpmc_thole_amatrix)        */
#define MPMC_K_DIPOLE_ITER 4 /* Jacobi contraction, stored tensors streamed (one launch per iteration; MATRIX_FREE: its kernel) */
#define MPMC_K_REDUCE 5      /* dipole update / final reductions / polarization energy */
#define MPMC_K_DIPOLE_FAR 6  /* unused since ABI 4 (the two-kernel form of the Jacobi contraction is gone); the slot stays for layout stability */
#define MPMC_K_THREE_BODY 6  /* the slot's use since: Axilrod-Teller sum / trial-move difference (0 for every context without the term) */
#define MPMC_K_CLASSES 7     /* tile bounding boxes, tile-pair classes, panel table of the Jacobi contraction     */
#define MPMC_K_COUNT 8
typedef struct mpmc_timings {
	double ms[MPMC_K_COUNT];      /* summed elapsed milliseconds                                           */
	int64_t launches[MPMC_K_COUNT]; /* number of timed launches                                            */
} mpmc_timings;

/* ---- library ---------------------------------------------------------------------------------------- */
int mpmc_abi_version(void);
int mpmc_device_count(int *count);
/* (ABI 6) for host programs that carry no HIP binding of their own (bench.py's ranks import neither torch nor hip-python): a fence over
 * everything this process has enqueued on `device`, and "<marketing name> (<gcnArchName>, <n> CUs)" for the job's log. */
int mpmc_device_synchronize(int device);
int mpmc_device_name(int device, char *name, int capacity);
const char *mpmc_last_error(const mpmc_ctx *ctx); /* ctx may be NULL: last create-time error of this thread */

/* ---- PeriodicBoundary::update (src/PeriodicBoundary.cpp:31-101): volume = det(basis), reciprocal = inverse,
 *      cutoff = half the shortest lattice vector (31^3 search).  Pure host helper. */
int mpmc_pbc_compute(const double basis[9], double reciprocal[9], double *volume, double *cutoff);

/* ---- context lifetime (one per System; replaces the per-System pair lists of src/System.Pairs.cpp:21) ---- */
/*      max_atoms is a capacity hint: mpmc_set_atoms with more atoms (insertions in the uVT / Gibbs ensembles) rebuilds the device
 *      buffers behind the same handle with 25 % headroom. */
int mpmc_ctx_create(int device, int max_atoms, mpmc_ctx **out);
int mpmc_ctx_destroy(mpmc_ctx *ctx);

/* System::update_pbc (src/System.cpp:859-876): basis = pbc.basis[q][p] row-major (rows are lattice vectors).
 * reciprocal/volume/cutoff may be NULL/0 to have the library compute them exactly like PeriodicBoundary. */
int mpmc_set_box(mpmc_ctx *ctx, const double basis[9], const double *reciprocal, double volume, double cutoff);
int mpmc_set_options(mpmc_ctx *ctx, const mpmc_options *opts);
void mpmc_default_options(mpmc_options *opts); /* reference defaults (src/System.h:21-24,510-831) */

/* Flattened atom list in atom_array order (src/System.cpp:881-904).  mol_id: equal ids = same Molecule.
 * frozen: Atom::frozen.  has_disp: nonzero iff any of c6,c8,c10 != 0 (only enters the rd_excluded test,
 * src/System.cpp:1050-1056); may be NULL.  mass may be NULL (only needed by mpmc_update_com). */
int mpmc_set_atoms(mpmc_ctx *ctx, int n, const double *pos /*[n][3]*/, const double *charge, const double *polarizability,
                   const double *epsilon, const double *sigma, const int32_t *mol_id, const int32_t *frozen,
                   const int32_t *has_disp, const double *mass);
/* after a Monte Carlo move: overwrite positions of atoms [first, first+count) */
int mpmc_update_positions(mpmc_ctx *ctx, int first, int count, const double *pos /*[count][3]*/);
/* same, positions already in device memory ([n][3] fp64, e.g. a torch tensor's data_ptr).  The library reads them on the context's own
 * stream, which is not ordered against the caller's streams: the data must be complete when this is called (synchronize the stream that
 * produced it first), and it is consumed before the call returns. */
int mpmc_set_positions_device(mpmc_ctx *ctx, const double *pos_device /*[n][3]*/);

/* ---- double System::energy() -------------------------------------------------------------------------- */
int mpmc_energy(mpmc_ctx *ctx, mpmc_result *out);
/* asynchronous pair: enqueue on the context's stream / wait + fetch (lets a caller overlap beads) */
int mpmc_energy_async(mpmc_ctx *ctx);
int mpmc_energy_wait(mpmc_ctx *ctx, mpmc_result *out);
/* (ABI 5) a scheduling hint for mpmc_energy_async: how many evaluations the caller keeps in flight together with this context's (the P
 * beads of PI_calculate_potential, PathIntegral.cpp:772-779).  With four or more the evaluation runs on ONE stream -- other evaluations
 * fill the device, and the side stream's fork and join only cost (+1 to 2 % evaluations/s with 8-32 in flight) --, alone it forks the
 * side stream for the reciprocal-space work (1.5 % faster).  Never changes a result; mpmc_energy() resets it to 1, the mpmc_pi_* loops set it
 * themselves. */
int mpmc_hint_in_flight(mpmc_ctx *ctx, int n_evaluations);

/* ---- polarization energy from half the Jacobi iterations; dipoles on demand ------------------------------------------------------------
 * A Jacobi solve with a fixed iteration count n = polar_max_iter (1 <= n <= 64) that starts from mu_0 = alpha E0 -- polar_iterative on,
 * polar_precision 0, polar_gamma 1, no polar_rrms, no polar_gs (`polar_palmo` acts under polar_gs only and changes nothing here); any solver -- takes its polarization energy from the
 * first ceil(n/2) iterations: with d_0 = mu_0 and d_k = mu_k - mu_(k-1) = (-alpha T)^k alpha E0 (T symmetric, alpha diagonal),
 *   E0 . mu_n = sum_{k=0..n} m_k,   m_2a = sum_i d_a,i . d_a,i / alpha_i,   m_2a+1 = sum_i d_a,i . d_a+1,i / alpha_i,
 * exact in exact arithmetic (polarization_energy differs from -1/2 sum mu_n . E0 in the last digits).  Every evaluation of such a context
 * computes its energy this way, so mpmc_energy and a bead of mpmc_pi_potential_local return the same bits.
 * The other n - ceil(n/2) iterations only produce mu_n, ef_induced and nothing an mpmc_result holds:
 *   - mpmc_energy, mpmc_energy_async, the component entry points and the trial moves run them at once, as before (eager);
 *   - mpmc_pi_potential_local, mpmc_pi_potential_local_host and mpmc_pi_allreduce leave them undone (on demand), and so do mpmc_energy /
 *     mpmc_energy_async of a context after mpmc_set_dipoles_on_demand(ctx, 1).  The setting survives like mpmc_set_polar_wolf's.
 * mpmc_get_dipoles (and the measurement entries that read the solve's state) first runs what is left, with the same kernels on the same
 * tables, and waits: mu, ef_induced and polar_iterations (= n in both modes) are bit-identical to an eager evaluation's.  The undone
 * iterations can no longer be run once their inputs are overwritten -- mpmc_set_atoms (capacity growth included), mpmc_update_positions,
 * mpmc_set_positions_device, a new cell or new options, a trial move, a measurement switch, or the next evaluation of any kind:
 * mpmc_get_dipoles then fails with MPMC_ERR_ARG and says so in mpmc_last_error; it never returns the dipoles of the half-way iteration.
 * Evaluate again (or switch to eager) to get them.  Contexts outside the conditions above behave exactly as before.
 * The debug key dipoles_on_demand = 0 (mpmc_debug_configure) makes every path eager, for A/B measurements. */
int mpmc_set_dipoles_on_demand(mpmc_ctx *ctx, int enabled);

/* ---- trial moves: the device-side counterpart of the reference's per-pair cache ----------------------------------------
 * The reference re-evaluates only the pairs whose displacement changed (Pair::recalculate_energy, src/System.cpp:1211-1224,
 * src/System.Energy.cpp:925,1484).  After a full mpmc_energy() of the accepted configuration:
 *   mpmc_trial_begin  : atoms [first, first+count) (original order; typically one molecule) get trial positions
 *   mpmc_trial_energy : energy of the trial configuration.  For count <= MPMC_TRIAL_MAX_ATOMS: O(count * N) pair terms (old
 *                       and new geometry of every pair that involves a moved atom) + O(K * count) structure-factor update,
 *                       added to the accepted totals.  Polarizable boxes without Wolf take the same delta path for the
 *                       pair energies and the real-space static field, rebuild the Thole tensors of the moved atoms' tiles
 *                       and solve the dipoles again (the solve is global).  A full evaluation of the trial configuration
 *                       runs instead for count > MPMC_TRIAL_MAX_ATOMS; for polarizable boxes under Wolf; with the tuning
 *                       switch polar_delta = 0; and, in a polarizable box, after a rejected full trial until the next
 *                       accepted trial or mpmc_energy().
 *   mpmc_trial_accept : the trial configuration becomes the accepted one / mpmc_trial_reject : it is discarded.
 * A full mpmc_energy() at any time re-bases the totals (the reference's flag_all_pairs, src/System.cpp:1284).
 * Trial positions equal to the accepted ones cost nothing: the trial totals are the accepted totals, no kernel runs. */
#define MPMC_TRIAL_MAX_ATOMS 256
int mpmc_trial_begin(mpmc_ctx *ctx, int first, int count, const double *new_pos /*[count][3]*/);
int mpmc_trial_energy(mpmc_ctx *ctx, mpmc_result *out);
/* the same in two halves (enqueue on the context's stream / wait): the P images of one path-integral move overlap on the device */
int mpmc_trial_energy_async(mpmc_ctx *ctx);
int mpmc_trial_energy_wait(mpmc_ctx *ctx, mpmc_result *out);
int mpmc_trial_accept(mpmc_ctx *ctx);
int mpmc_trial_reject(mpmc_ctx *ctx);

/* ---- exchange trials: insertion and removal of one molecule (uVT insert / remove, the particle transfers of the Gibbs ensemble) --------
 * The same five calls serve a trial that changes the composition: mpmc_trial_energy (or _async / _wait), then mpmc_trial_accept or
 * mpmc_trial_reject.  Preconditions as for mpmc_trial_begin: an accepted configuration (mpmc_energy), no open trial, finite positions
 * (MPMC_ERR_INVALID_DATUM otherwise).  A range that is not exactly one whole molecule, an at_index inside a molecule and the removal of the
 * last molecule are MPMC_ERR_ARG with a text in mpmc_last_error.
 *   The mpmc_result of the trial is that of the trial composition in every field (energies and their parts, N, NU and all counts).
 *   Boxes without polarization, with the default rd model and without rd_crystal, for count <= MPMC_TRIAL_MAX_ATOMS, take a delta path:
 * O(count * N) pair terms of the molecule with everybody else (each pair once, added or subtracted), the molecule's own pairs, the
 * structure factors plus or minus the molecule's phases, and the position-independent terms (es_self, lrc_pair, lrc_self, N) of the trial
 * composition.  Ewald or Wolf electrostatics, rd_only and the Feynman-Hibbs corrections are included.  Everything else (polarizable boxes,
 * rd_crystal, another rd model, longer molecules) evaluates the trial composition in full; mpmc_debug_last_trial_was_full tells.  A context
 * with Axilrod-Teller or disp-expansion coefficients refuses both calls with MPMC_ERR_UNSUPPORTED: those coefficients belong to one atom
 * list (mpmc_set_atoms, then the coefficients again).
 *   accept: the context's atom list is the new one (the molecule of an insertion gets a molecule id of its own; the context grows as under
 * mpmc_set_atoms), the accepted totals are the trial totals, and the next trial of either kind or mpmc_energy works on the new composition
 * -- on the delta path without a re-basing evaluation: the list is edited on the host, the spatial order is carried, and the next call
 * uploads it.  reject: nothing of a delta trial is left; after a full evaluation the accepted list is put back as a rejected displacement
 * of that branch puts the positions back. */
/* trial insertion of ONE molecule of `count` atoms in front of atom `at_index` of the current list (at_index == n: appended;
 * at_index must be a molecule boundary).  Arrays as in mpmc_set_atoms, `count` long; the new atoms form one new molecule. */
int mpmc_trial_insert_begin(mpmc_ctx *ctx, int at_index, int count, const double *pos, const double *charge, const double *polarizability,
                            const double *epsilon, const double *sigma, const int32_t *frozen, const int32_t *has_disp, const double *mass);
/* trial removal of the whole molecule that occupies atoms [first, first+count) */
int mpmc_trial_remove_begin(mpmc_ctx *ctx, int first, int count);

/* ---- volume trials: the volume change of NPT and of the Gibbs ensemble's volume exchange as a trial --------------------------------------
 * System::volume_change / volume_change_Gibbs with revert_volume_change as its rejection (src/System.MonteCarlo.cpp:1235-1340, 1690-1727).
 * The same five calls carry it: mpmc_trial_energy (or _async / _wait), then mpmc_trial_accept or mpmc_trial_reject.
 *   The move, in the reference's arithmetic: every basis element times basis_scale_factor; reciprocal, volume and cutoff from
 * mpmc_pbc_compute on the product; ewald_alpha and polar_ewald_alpha follow the new cutoff where the options leave them to the cell; every
 * molecule (frozen ones too) shifted rigidly by com * s - com, com its centre of mass of the ACCEPTED positions (mass += m_i, cm[p] += m_i *
 * pos_i[p] atom by atom in list order, cm[p] /= mass, as mpmc_update_com).  The positions are scaled on the device, on the context's stream,
 * into a second position buffer (MPMC_K_CLASSES); the atoms keep their slots, nothing is sorted or uploaded.
 *   The trial cell and positions get the full evaluation of whatever terms the context has on (mpmc_debug_last_trial_was_full answers 1);
 * every field of the mpmc_result is the trial configuration's.
 *   accept: cell, positions, the host mirrors behind mpmc_update_com / mpmc_cavity_update and the totals become the accepted ones with no
 * further evaluation; the host computes its mirrors with the same expressions, nothing is copied back.  The next displacement or exchange
 * trial is a delta on the new cell; a cavity grid is stale, as after mpmc_set_box; a later mpmc_set_box with the scaled basis is a no-op.
 *   reject: cell, k tables, structure factors, positions, position-independent terms and accepted totals are the accepted configuration's
 * again without an evaluation (the trial was evaluated into alternate buffers, which trade places back).  In a polarizable box the next
 * trial evaluates in full, as after any rejected full trial.
 *   basis_scale_factor == 1.0 is a trial that launches nothing.  MPMC_ERR_ARG with a text: no accepted configuration; a trial already
 * open; mpmc_set_atoms was called without masses; the accepted cell was set with a caller-supplied reciprocal, volume or cutoff (there is
 * no rule for scaling an override).  MPMC_ERR_INVALID_DATUM: basis_scale_factor not finite or <= 0; a molecule whose masses sum to 0.
 * mpmc_set_box, mpmc_set_options, mpmc_set_atoms and mpmc_update_positions close an open volume trial as a rejection before they act
 * (mpmc_set_box with the accepted cell and mpmc_set_options with unchanged options too: they are no-ops only while no volume trial is open); a
 * trial enqueued with mpmc_trial_energy_async and never waited for is drained first, as mpmc_trial_reject drains it.  What they leave is what
 * they leave without a trial: the accepted cell, tables and positions back in place, no accepted totals (call mpmc_energy), and
 * mpmc_trial_reject answers that no trial move is open.
 *   While a volume trial is open, every call that evaluates (mpmc_energy, mpmc_energy_async, the component calls mpmc_lj ... mpmc_polar,
 * mpmc_thole_field, the bead loops) is refused with MPMC_ERR_ARG and a text, and the trial stays open: the resident cell and positions
 * are the trial's, and a complete evaluation would re-base the accepted totals on them.  Accept or reject first.
 *   A context that outgrew its capacity (mpmc_set_atoms, an accepted insertion) keeps the cell as the caller gave it: a basis handed over
 * alone can still be scaled. */
int mpmc_trial_volume_begin(mpmc_ctx *ctx, double basis_scale_factor);
/* the open volume trial's cell and positions (any pointer may be NULL); valid from _begin until accept / reject */
int mpmc_trial_volume_get(mpmc_ctx *ctx, double basis[9], double reciprocal[9], double *volume, double *cutoff, double *pos /*[n][3]*/);
/* diagnostics: out4 = { volume trials evaluated, accepted, rejected, evaluations enqueued from inside mpmc_trial_reject for them } */
int mpmc_debug_volume_trial_counts(mpmc_ctx *ctx, long long out4[4]);
/* diagnostics: out3 = { exchange trials on the delta path, exchange trials evaluated in full, summations of the host sums over the whole list } */
int mpmc_debug_exchange_counts(mpmc_ctx *ctx, long long out3[3]);
/* diagnostics: the positions resident on the device, original atom order (the trial's while an evaluated volume trial is open); a blocking
 * copy.  MPMC_ERR_ARG while an upload of the atom list is pending. */
int mpmc_debug_device_positions(mpmc_ctx *ctx, double *pos /*[n][3]*/);
/* The ENSEMBLE_NPT branch of System::boltzmann_factor (:1441-1457) in the reference's operand order, host only:
 *   MPMC_MOVETYPE_VOLUME    exp(-(dE + pressure * ATM2REDUCED * (v_new - v_old) - (N + 1) * T * log(v_new / v_old)) / T), dE = final - init
 *   MPMC_MOVETYPE_DISPLACE  exp(-dE / T)
 * anything else: MPMC_ERR_UNSUPPORTED.  N = observables->N of the trial configuration, pressure in atm. */
typedef struct mpmc_npt_move {
	int32_t movetype, reserved;
	double temperature, pressure, N, init_energy, final_energy, volume_old, volume_new;
} mpmc_npt_move;
int mpmc_npt_boltzmann_factor(const mpmc_npt_move *move, double *boltzmann_factor);

/* ---- batched insertion candidates: many trial insertions of one molecule in one launch chain ---------------------------------------------
 * Widom test-particle insertion, orientational-bias / multiple-try insertion at one site and energy-biased site selection ask the same
 * question many times against an unchanged accepted configuration: what is the energy with this molecule at this pose?  out[c] is the
 * mpmc_result that mpmc_trial_insert_begin(ctx, n, count, pos + 3*count*c, ...) + mpmc_trial_energy + mpmc_trial_reject would give for
 * candidate c, in every field and bit for bit (at_index does not enter a delta-path result), for n_cand candidates behind ONE host wait.
 * The per-atom arrays are those of mpmc_trial_insert_begin, `count` long and shared by all candidates; only the positions differ.
 *   The call opens no trial and changes nothing an evaluation, a trial or a cavity update reads: accepted totals, structure factors and
 * atom list are as before, and the chosen candidate is then inserted with mpmc_trial_insert_begin / mpmc_trial_energy / mpmc_trial_accept,
 * whose result has the bits of out[c].  Preconditions and codes as for mpmc_trial_insert_begin, in the same order: no open trial
 * (MPMC_ERR_ARG), no Axilrod-Teller or disp-expansion coefficients (MPMC_ERR_UNSUPPORTED), an accepted configuration (MPMC_ERR_ARG), finite
 * positions in every candidate (MPMC_ERR_INVALID_DATUM).  MPMC_ERR_ARG also for count < 1, n_cand < 1, n_cand > MPMC_INSERT_MAX_CANDIDATES
 * and null pos or out.
 *   Only the delta path exists here: a polarizable box (polarization on and not rd_only), rd_crystal, a non-default rd model and
 * count > MPMC_TRIAL_MAX_ATOMS are MPMC_ERR_UNSUPPORTED with a text in mpmc_last_error -- a batch of full evaluations is the loop of single
 * trials.  Ewald and Wolf electrostatics, rd_only, the Feynman-Hibbs corrections, frozen and null-rd atoms and any cell are carried.
 *   Cost O(n_cand count N) pair terms + O(n_cand count K); device time is counted under MPMC_K_PAIR.  Scratch is bounded: large batches run
 * in internal chunks of 256 candidates (32 B x K of trial structure factors each), all buffers are allocated by the first call. */
#define MPMC_INSERT_MAX_CANDIDATES 65536
int mpmc_insert_candidates(mpmc_ctx *ctx, int count, int n_cand, const double *pos /*[n_cand][count][3]*/, const double *charge,
                           const double *polarizability, const double *epsilon, const double *sigma, const int32_t *frozen, const int32_t *has_disp,
                           const double *mass, mpmc_result *out /*[n_cand]*/);
/* diagnostics only, read-only: out2 = { calls of mpmc_insert_candidates that ran, candidates they evaluated } */
int mpmc_debug_insert_batch_counts(mpmc_ctx *ctx, long long *out2);

/* ---- the Axilrod-Teller triple-dipole dispersion, System::axilrod_teller (src/System.Energy.cpp:129-136, 1653-1770) --------------------
 * Sum over every unordered triple of distinct atoms that are not all in one molecule, no cutoff, frozen atoms included; each pair vector is
 * that pair's own minimum image.  Added to energy (and NU) as three_body_energy; the path-integral sums stay {rd, coulombic, polarization,
 * vdw} (PathIntegral.cpp:752-805), per_bead carries the field.  Cost O(N^3) per evaluation, O(m N^2) per trial move of m <= MPMC_TRIAL_MAX_ATOMS
 * atoms.  Per-atom coefficients in the caller's atom order, length n of the current atom list: c6 is read only with midzuno_kihara_approx
 * (c9_i = 3/4 alpha_i 6.7483345 c6_i), c9 only without it; either may then be NULL.  enabled = 0 switches the term off.  mpmc_set_atoms
 * discards the coefficients (the setting stays): an evaluation with the term on and no coefficients fails with MPMC_ERR_ARG.  Position
 * updates and accepted trials keep them. */
int mpmc_set_axilrod_teller(mpmc_ctx *ctx, int enabled, int midzuno_kihara_approx, const double *c6, const double *c9);
int mpmc_axilrod_teller(mpmc_ctx *ctx, double *out); /* System::axilrod_teller(), component entry like mpmc_lj */

/* ---- the dispersion-expansion repulsion/dispersion term, System::disp_expansion (src/System.Energy.cpp:1939-2080) ----------------------
 * `disp_expansion on`: replaces lj() in rd_energy.  The atoms' epsilon is the repulsion exponent alpha (1/A), sigma is r0 (A); c6, c8, c10
 * per atom in atomic units, in the caller's atom order, length n of the current atom list (c10 may be NULL: zeros).  Negative or non-finite
 * coefficients are refused with MPMC_ERR_INVALID_DATUM: unlike the reference, which would take sqrt of the product of two negative c's.
 * Every pair that is neither rd_excluded nor frozen contributes at its minimum-image distance, with no cutoff:
 *   315.775 exp(-alpha_ij (r - r0_ij)) - c6_ij / r^6 - c8_ij / r^8 - c10_ij / r^10   (Tang-Toennies damped under MPMC_DISP_DAMP)
 * With rd_lrc, lrc_pair holds disp_expansion_lrc summed over every non-frozen pair and lrc_self disp_expansion_lrc_self over every
 * non-frozen atom; lj_pairs holds the pair sum and rd_energy their total.  The counts keep their meaning.  Cost O(N^2) per evaluation,
 * O(m N) per trial move of m <= MPMC_TRIAL_MAX_ATOMS atoms.  enabled = 0 switches the term off.  mpmc_set_atoms discards the coefficients
 * (the setting stays): an evaluation with the term on and no coefficients fails with MPMC_ERR_ARG.  Position updates, accepted trials and
 * capacity growth keep them.  MPMC_FLAG_OTHER_RD (the keyword through mpmc_check_flags) is still refused. */
#define MPMC_DISP_DAMP 1            /* damp_dispersion: Tang-Toennies damping of the three dispersion terms  */
#define MPMC_DISP_EXTRAPOLATE_C10 2 /* extrapolate_disp_coeffs: c10_ij = 49/40 c8_ij^2 / c6_ij                */
#define MPMC_DISP_SCHMIDT 4         /* schmidt_ff: alpha_ij = (a_i + a_j) a_i a_j / (a_i^2 + a_j^2)            */
int mpmc_set_disp_expansion(mpmc_ctx *ctx, int enabled, int flags, const double *c6, const double *c8, const double *c10);
int mpmc_disp_expansion(mpmc_ctx *ctx, double *out); /* System::disp_expansion() (rd_energy of the term), component entry like mpmc_lj */

/* ---- `rd_crystal on`: the lattice-summed Lennard-Jones of System::lj (src/System.Energy.cpp:916-963, 1017-1022, 1152-1208) ----------------
 * With o = order and cut = 2 * cutoff * (o - 0.5) every unordered pair that is not frozen and whose minimum-image distance passes
 * rimg - 1e-12 < cut contributes the sum over the images n in [-(o-1), o-1]^3 at a = B n + (pos_i - pos_j), RAW positions as handed to
 * mpmc_set_atoms / mpmc_update_positions (not wrapped, not minimum image), of the terms with |a| <= cut:
 *   4 eps_ij (t12 - S6),  S6 = sum (|sigma_ij| / |a|)^6,  S12 likewise,  t12 = 0 for an attractive-only pair
 * (+ lj_fh_corr of the two sums at 1 / rimg under feynman_hibbs).  rd_excluded pairs (same molecule, null sigma / epsilon) are NOT skipped:
 * they only lose the image n = 0.  Every atom with sigma or epsilon != 0 adds 4 eps_i (t12 - t6) of half its own images n != 0 inside cut
 * (crystal_self); lrc_pair and lrc_self are taken at cut instead of the box cutoff.
 *   lj_pairs = the pair sum, rd_energy = ((lj_pairs + lrc_pair) + crystal_self) + lrc_self;  mpmc_lj returns this rd_energy.
 * The counts keep their meaning (box cutoff, !rd_excluded); electrostatics and polarization are untouched.  The image table, cut, the
 * corrections and crystal_self follow every mpmc_set_box.  The setting has the lifetime of mpmc_set_polar_wolf's: it survives
 * mpmc_set_atoms, mpmc_set_box, mpmc_set_options, position updates, accepted trials and capacity growth; enabled = 0 (order ignored)
 * restores the plain term.  order < 1 or > MPMC_RD_CRYSTAL_MAX_ORDER is refused with MPMC_ERR_INVALID_SETTING (SimulationControl.cpp:
 * 1688-1692).  Cost O(N^2 (2o-1)^3) per evaluation, O(m N (2o-1)^3) per trial move of m <= MPMC_TRIAL_MAX_ATOMS atoms; time is counted in
 * MPMC_K_PAIR.  System::disp_expansion ignores rd_crystal: a context with mpmc_set_disp_expansion on returns the disp-expansion result
 * unchanged, bit for bit, whatever this setting is.  MPMC_FLAG_RD_CRYSTAL in unsupported_flags is still refused: this call alone
 * switches the term on.  The sigma rule of mpmc_set_cavity_autoreject is refused together with this term (MPMC_ERR_UNSUPPORTED). */
#define MPMC_RD_CRYSTAL_MAX_ORDER 8 /* (2 * 8 - 1)^3 = 3375 images */
/* (a struct tag, not a typedef: the entry point below carries the same name) */
struct mpmc_rd_crystal_info {
	int32_t order;          /* of the last evaluation (complete, component or trial) with the term on; 0: none has run */
	int32_t n_images;       /* (2 order - 1)^3, the size of the image table                                             */
	double cutoff;          /* 2 * box cutoff * (order - 0.5)                                                           */
	int64_t n_image_terms;  /* image terms that passed |a| <= cutoff, over all contributing pairs                       */
	double crystal_self;    /* sum of rd_crystal_self over the atoms                                                    */
};
int mpmc_set_rd_crystal(mpmc_ctx *ctx, int enabled, int order);
int mpmc_rd_crystal_info(mpmc_ctx *ctx, struct mpmc_rd_crystal_info *out);

/* ---- the rd model: `waldmanhagler` / `halgren_mixing` / `c6_mixing` and `lj_buffered_14_7` / `dreiding` ------------------------------------
 * (mixing: System::pair_exclusions, src/System.cpp:1069-1177; forms: System::lj src/System.Energy.cpp:897-1032, lj_buffered_14_7 :1212-1248,
 * dreiding :2098-2215 with DREIDING_GAMMA = 12; dispatch :113-127, where dreiding comes before lj_buffered_14_7)
 * One setting per context: a potential form and a mixing rule for sigma_ij, eps_ij.  (LJ, LB) is the default: it runs none of this and
 * returns the bits of a context that never made the call.  Under any other model the pair sum inside the cutoff is
 *   LJ:        4 eps_ij (t12 - t6), t6 = (sigma_ij / rimg)^6, for pairs with rimg - 1e-12 < cutoff;  + lj_fh_corr with eps_ij under feynman_hibbs
 *   14-7:      eps_ij (1.07 / (rho + 0.07))^7 (1.12 / (rho^7 + 0.12) - 2), rho = rimg / sigma_ij, for pairs with !(rimg > cutoff)
 *   DREIDING:  eps_ij (termexp - 2 rho^-6), termexp = exp(12 (1 - rho)), or 1e40 (MAXVALUE) for rimg < 0.4 sigma_ij; !(rimg > cutoff)
 * over the pairs that are neither rd_excluded nor both frozen (the rules of the plain term), with
 *   LB:               sigma_ij = (s_i + s_j) / 2 (0 when either is 0),         eps_ij = sqrt(e_i e_j)
 *   Waldman-Hagler:   sigma_ij^6 = (s_i^6 + s_j^6) / 2 (0 when either is 0),  eps_ij = sqrt(e_i e_j) 2 s_i^3 s_j^3 / (s_i^6 + s_j^6)
 *   Halgren:          sigma_ij = (s_i^3 + s_j^3) / (s_i^2 + s_j^2),            eps_ij = 4 e_i e_j / (sqrt e_i + sqrt e_j)^2 (each 0 unless both > 0)
 *   C6:               sigma_ij = (s_i + s_j) / 2,                              eps_ij = 64 sqrt(e_i e_j) s_i^3 s_j^3 / (s_i + s_j)^6
 * A pair that is not excluded but whose sigma_ij or eps_ij is 0 (an atom with dispersion coefficients and no sigma) contributes exactly 0.
 * LJ form: lrc_pair = sum of lj_lrc_corr with the mixed parameters over every pair that is not frozen and has eps_ij != 0 and sigma_ij != 0
 * (intramolecular pairs too), lrc_self as ever; rd_energy = (lj_pairs + lrc_pair) + lrc_self.  14-7 and DREIDING have no long-range and no
 * Feynman-Hibbs correction whatever rd_lrc and feynman_hibbs say: lrc_pair = lrc_self = 0, rd_energy = lj_pairs; they ignore rd_crystal as
 * disp-expansion does (result unchanged to the bit).  mpmc_lj returns this rd_energy.  n_lj_in_cutoff keeps its meaning (the LJ test) under
 * every form; n_terms below counts by the form's own test (the two differ for rimg in (cutoff, cutoff + 1e-12) only).
 * Electrostatics, polarization and the Axilrod-Teller term are untouched.
 * sigma < 0 or epsilon < 0 on any atom is refused with MPMC_ERR_INVALID_DATUM at the evaluation (epsilon < 0 already by mpmc_set_atoms):
 * the reference's Waldman-Hagler branch leaves eps_ij unassigned for such atoms, its Halgren branch zeroes it and its C6 branch averages
 * signed values; no force field uses any of these.  Refused at the evaluation, with a message: MPMC_ERR_INCOMPATIBLE together with
 * mpmc_set_disp_expansion (the reference never reaches the disp-expansion mixing behind these rules); MPMC_ERR_UNSUPPORTED for the LJ form
 * with a non-LB rule together with mpmc_set_rd_crystal.  The sigma rule of mpmc_set_cavity_autoreject tests the model's sigma_ij.
 * The setting has the lifetime of mpmc_set_polar_wolf's: it survives mpmc_set_atoms, mpmc_set_box, mpmc_set_options, position updates,
 * accepted trials and capacity growth; it is refused while an evaluation or a trial move is open.  An unknown form or rule is refused
 * with MPMC_ERR_INVALID_SETTING.  MPMC_FLAG_NON_LB_MIXING and MPMC_FLAG_OTHER_RD in unsupported_flags are still refused: this call alone
 * switches the term on.  Cost O(N^2) per evaluation (tile pairs wholly beyond the cutoff are skipped in orthorhombic cells), O(m N) per
 * trial move of m <= MPMC_TRIAL_MAX_ATOMS atoms; time is counted in MPMC_K_PAIR. */
#define MPMC_RD_FORM_LJ 0
#define MPMC_RD_FORM_BUFFERED_14_7 1
#define MPMC_RD_FORM_DREIDING 2
#define MPMC_RD_MIX_LB 0
#define MPMC_RD_MIX_WALDMAN_HAGLER 1
#define MPMC_RD_MIX_HALGREN 2
#define MPMC_RD_MIX_C6 3
/* (a struct tag, not a typedef: the entry point below carries the same name) */
struct mpmc_rd_model_info {
	int32_t form, mixing;          /* of the last evaluation (complete, component or trial) with a non-default model; 0, 0: none has run */
	int64_t n_terms;               /* pairs that contributed: not excluded, not frozen, inside the form's own distance test               */
	int64_t n_tile_pairs;          /* 64 x 64 tile pairs of the table ...                                                                  */
	int64_t n_tile_pairs_skipped;  /* ... and how many of them lay wholly beyond the cutoff and were not walked (0 in triclinic cells)    */
};
int mpmc_set_rd_model(mpmc_ctx *ctx, int form, int mixing);
int mpmc_rd_model_info(mpmc_ctx *ctx, struct mpmc_rd_model_info *out);

/* ---- `sg`: the Silvera-Goldman molecular hydrogen potential ------------------------------------------------------------------------------
 * (System::sg src/System.Energy.cpp:1763-1867, dispatch :115-116; the constants of :1763-1770)
 * enabled != 0: System::energy() of a system with `sg on`.  rd_energy = lj_pairs = sg(), the sum over EVERY pair i < j of the atom list
 * with rimg < cutoff (strict: a pair at exactly the cutoff is out) of (V [+ V_FH]) * 3.15774655e5 K, with x = rimg / 0.529177249 and
 *   V = exp(ALPHA - BETA x - GAMMA x^2) - (C6 / x^6 + C8 / x^8 + C10 / x^10 - C9 / x^9) f(x),  f = exp(-(RM / x - 1)^2) for x < RM, else 1.
 * sg() tests neither the exclusions nor the frozen flags: pairs inside one molecule count, atoms with sigma = 0 or epsilon = 0 count, and
 * sigma, epsilon and the charge play no part.  Under feynman_hibbs V_FH is the expression of :1831-1845 as the reference writes it
 * (110 C10 / x^10 in the second derivative; derivatives in bohr under a prefactor in Angstrom^2; the mass of the molecule of the atom that
 * comes FIRST in the caller's atom list, not a reduced mass -- so with two species the value depends on the order of the list, as in the
 * reference); feynman_hibbs_order plays no part.  Masses and a positive temperature are required as for the Lennard-Jones corrections.
 *   With the term on there are no electrostatics and no polarization whatever the options say (:46): es_*, coulombic_energy,
 * polarization_energy, n_es_in_cutoff and polar_iterations are 0, no static field and no dipole solve run, and every entry point that reads
 * dipoles or fields behaves as on a box with polarization off.  lrc_pair = lrc_self = 0 whatever rd_lrc says, and mpmc_set_rd_crystal is
 * ignored (result unchanged to the bit).  No Lennard-Jones pass runs: n_lj_in_cutoff is 0; n_terms below counts the pairs kept.  The
 * Axilrod-Teller term is still added when on; the absolute rule of mpmc_set_cavity_autoreject works as it is.  mpmc_lj returns this rd_energy.
 *   Refused at the evaluation, with a message: MPMC_ERR_INCOMPATIBLE together with a non-default mpmc_set_rd_model or with
 * mpmc_set_disp_expansion; MPMC_ERR_UNSUPPORTED with the sigma rule of mpmc_set_cavity_autoreject (it lives inside lj()) and for a list with
 * two or more frozen atoms (the reference never measures a pair of two frozen atoms here: its value is inf - inf, not finite).
 *   Trial moves: a displacement of m <= MPMC_TRIAL_MAX_ATOMS atoms is the O(m N) delta with n_terms carried as a difference; longer moves,
 * insertions and removals evaluate the trial in full; mpmc_insert_candidates is refused with MPMC_ERR_UNSUPPORTED.
 *   The setting has the lifetime of mpmc_set_rd_model's: it survives mpmc_set_atoms, mpmc_set_box, mpmc_set_options, position updates,
 * accepted trials and capacity growth; it is refused while an evaluation or a trial move is open; it drops the accepted totals; enabled = 0
 * returns the bits of a context that never made the call.  MPMC_FLAG_USE_SG in unsupported_flags is still refused: this call alone
 * switches the term on.  Cost O(N^2) per evaluation; time is counted in MPMC_K_PAIR. */
/* (a struct tag, not a typedef: the entry point below carries the same name) */
struct mpmc_silvera_goldman_info {
	int32_t enabled;        /* the setting                                                                                          */
	int32_t feynman_hibbs;  /* of the last evaluation (complete, component or trial) with the term: V_FH was added                  */
	int64_t n_terms;        /* ... its pairs with rimg < cutoff; 0: none has run                                                    */
	double cutoff;          /* ... and its cutoff (Angstrom)                                                                        */
};
int mpmc_set_silvera_goldman(mpmc_ctx *ctx, int enabled);
int mpmc_silvera_goldman_info(mpmc_ctx *ctx, struct mpmc_silvera_goldman_info *out);

/* ---- `cavity_autoreject`, `cavity_autoreject_absolute`, `cavity_autoreject_scale`: contact rejection of uVT moves ---------------------------
 * (System::lj src/System.Energy.cpp:1001-1004, lj_buffered_14_7 :1237-1239, dreiding :2182-2185; System::cavity_absolute_check
 * src/System.Cavity.cpp:211-228, called at :167; validation SimulationControl.cpp:2139-2154)
 *   MPMC_AUTOREJECT_SIGMA     a pair the rd function admits (neither rd_excluded nor frozen, inside the form's own distance test: rimg - 1e-12 <
 *                             cutoff for LJ, !(rimg > cutoff) for 14-7 and DREIDING) with rimg < scale * sigma_ij gets MAXVALUE = 1e40 as its
 *                             rd_energy.  sigma_ij is the mixed sigma of the context's rd model (|sigma_ij| for the LJ form).  With n_replaced
 *                             such pairs:  lj_pairs = S + n_replaced * 1e40, computed on the host in this order, S the sum the pair kernels
 *                             deliver, untouched; rd_energy, energy and NU follow; mpmc_lj returns this rd_energy.  A replaced pair's own
 *                             energy stays in S, where the reference replaces it: that differs from the reference by less than 1e-9 relative
 *                             unless rimg < sigma_ij / 300 (4 eps (sigma / r)^12 reaches 1e31 there).  Overlapping atoms (rimg = 0) give a
 *                             non-finite S as they do without the rule; every driver rejects a non-finite energy.  n_lj_in_cutoff and the
 *                             other counts are unchanged; electrostatics and polarization are untouched to the bit.
 *   MPMC_AUTOREJECT_ABSOLUTE  every measured pair of atoms of different molecules -- excluded, null, beyond the cutoff -- with rimg < scale
 *                             (Angstrom) is an absolute contact.  System::pairs measures a pair `if (!frozen || polarization)` (System.cpp:985):
 *                             with mpmc_options.polarization off a pair of two frozen atoms of different molecules keeps rimg = 0 and trips the
 *                             test in every call (n_unmeasured_frozen, counted on the host from the atom list; 0 with polarization on).  On a
 *                             hit energy() RETURNS its value plus MAXVALUE; observables->energy, rd_energy and NU stay unpenalised, and so does
 *                             mpmc_result, which mirrors the observables: the penalty is absolute_penalty / returned_energy of the info struct.
 *                             PI_calculate_potential reads the observables, so the path-integral entry points carry no absolute penalty.
 * rules = 0 switches both off: no kernel of this feature is launched, and every result has the bits and the launch counts of a context
 * that never made the call.  rules != 0 with scale outside (0, 1] or non-finite, or unknown rule bits: MPMC_ERR_INVALID_SETTING.  repulsion
 * (`cavity_autoreject_repulsion`) is read under mpmc_set_disp_expansion alone, as in the reference (below).  The setting has the lifetime
 * and the refusal rules of
 * mpmc_set_rd_model: it survives mpmc_set_atoms, mpmc_set_box, mpmc_set_options, position updates, accepted trials and capacity growth, and
 * is refused while an evaluation or a trial move is open.  MPMC_FLAG_CAVITY_AUTOREJECT in unsupported_flags is still refused: this call alone
 * switches the behaviour on.
 *   The counts come from one more pair walk behind the evaluation's kernels (MPMC_K_PAIR), both rules in one walk, posted with the result:
 * no path gains a host wait.  In orthorhombic cells only the tile pairs whose bounding boxes come closer than dmax = scale * max sigma_ij
 * (sigma rule) or scale (absolute rule) are walked (tile_pairs_walked / tile_pairs_skipped); the debug key contact_skip = 0 walks all.
 *   Trial moves: a displacement of up to MPMC_TRIAL_MAX_ATOMS atoms on the delta path adds the (new - old) counts of the moved atoms' pairs
 * to the accepted counts, O(m N); accept commits the trial counts, reject drops them.  Every branch that evaluates the trial configuration
 * in full runs the full walk.  An insertion on the delta path adds the molecule's contacts with the residents, a removal subtracts them
 * (a sibling launch of the exchange kernel, molecule against resident tile, in front of the finish that posts), and the unmeasured frozen
 * pairs of the trial composition follow from the host's counts: exchange trials stay O(m N) under the setting.
 *   mpmc_insert_candidates: out[c] is what the single insertion trial delivers, bit for bit (the sigma rule's penalty included), and
 * mpmc_insert_candidates_contacts returns the last batch's counts per candidate -- n_replaced and n_absolute of candidate c's trial
 * composition, the values mpmc_cavity_autoreject_info gives behind that single trial (zeros for a rule that is off or a batch made with
 * the setting off).  Either array may be NULL.  MPMC_ERR_ARG when no batch has run on this context or n_cand differs from the last
 * batch's.  The counts travel behind the batch's one wait.  n_unmeasured_frozen of a candidate's composition does not depend on the pose:
 * it is the single trial's.
 *   Under mpmc_set_disp_expansion the sigma rule is System::disp_expansion's (:1958, 1983-1989): every pair that is neither rd_excluded nor
 * frozen, with no cutoff, sigma_ij = r0_ij as mixed; and with repulsion != 0 a pair is replaced as well when its repulsion
 * 315.775 exp(-alpha_ij (rimg - r0_ij)) > repulsion (the exponential is the device's: a pair within an ulp of the threshold may fall on the
 * other side than in the reference).  The repulsion test has no distance bound here: every tile pair is walked.  mpmc_disp_expansion returns
 * the penalised rd_energy.
 *   Refused at the evaluation with MPMC_ERR_UNSUPPORTED and a text: the sigma rule together with mpmc_set_rd_crystal (the reference tests
 * intramolecular pairs there, which rejects every multi-site molecule: no input means that).
 * mpmc_cavity_autoreject_info: of the last result delivered (evaluation, component call or trial). */
#define MPMC_AUTOREJECT_SIGMA 1
#define MPMC_AUTOREJECT_ABSOLUTE 2
/* (a struct tag, not a typedef: the entry point below carries the same name) */
struct mpmc_cavity_autoreject_info {
	int32_t rules;                /* MPMC_AUTOREJECT_* of the context                                                            */
	int32_t reserved;
	double scale, repulsion;      /* cavity_autoreject_scale, cavity_autoreject_repulsion                                        */
	int64_t n_replaced;           /* pairs whose rd_energy is MAXVALUE (sigma rule)                                              */
	int64_t n_absolute;           /* measured pairs of different molecules with rimg < scale (absolute rule)                     */
	int64_t n_unmeasured_frozen;  /* frozen-frozen pairs of different molecules, unmeasured (absolute rule, polarization off)    */
	double absolute_penalty;      /* MAXVALUE if n_absolute + n_unmeasured_frozen > 0, else 0                                     */
	double returned_energy;       /* result.energy + absolute_penalty: what System::energy() returns                             */
	int64_t tile_pairs_walked;    /* of the last full contact walk: tile pairs walked ...                                        */
	int64_t tile_pairs_skipped;   /* ... and tile pairs whose bounding boxes lie further apart than dmax                         */
};
int mpmc_set_cavity_autoreject(mpmc_ctx *ctx, int rules /* OR of MPMC_AUTOREJECT_*, 0 = off */, double scale, double repulsion);
int mpmc_cavity_autoreject_info(mpmc_ctx *ctx, struct mpmc_cavity_autoreject_info *out);
int mpmc_insert_candidates_contacts(mpmc_ctx *ctx, int n_cand, int64_t *n_replaced /*[n_cand]*/, int64_t *n_absolute /*[n_cand]*/);

/* ---- public component entry points of the reference (src/System.h:346-402), for parity tests ----------- */
int mpmc_lj(mpmc_ctx *ctx, double *out);                  /* System::lj() (rd_crystal: its lattice sum; a non-default rd model: its rd_energy) */
int mpmc_coulombic(mpmc_ctx *ctx, double *out);           /* System::coulombic()            */
int mpmc_coulombic_real(mpmc_ctx *ctx, double *out);      /* System::coulombic_real()       */
int mpmc_coulombic_reciprocal(mpmc_ctx *ctx, double *out);/* System::coulombic_reciprocal() */
int mpmc_coulombic_self(mpmc_ctx *ctx, double *out);      /* System::coulombic_self()       */
int mpmc_polar(mpmc_ctx *ctx, double *out);               /* System::polar()                */
int mpmc_thole_field(mpmc_ctx *ctx, double *ef_static /*[n][3] host, may be NULL*/); /* System::thole_field() */
/* System::thole_amatrix(): fills rows [row0, row0+nrows) of the dense 3N x 3N matrix into `a` (host, row-major
 * nrows x 3N).  Diagonal 1/alpha (1e40 when alpha == 0), off-diagonal blocks as src/System.Energy.cpp:2744-2764. */
int mpmc_thole_amatrix(mpmc_ctx *ctx, int row0, int nrows, double *a);

/* ---- `polar_iterative off`: the dipoles by a direct solve (System::polar :2590-2607: thole_field, thole_bmatrix, thole_bmatrix_dipoles) --
 * With polarization on, rd_only off and polar_iterative == 0 an evaluation computes the static field as always, solves A mu = E0 on the
 * device and returns polarization_energy = -1/2 sum mu . E0.  A is the matrix of thole_amatrix restricted to the polarizable atoms (atoms
 * with alpha == 0 get mu = 0 exactly; the reference's 1e40 diagonal gives them dipoles of the order 1e-40 E).  A is symmetric and positive
 * definite for a physical model: it is factored as L L^T (blocked Cholesky, trailing update on the fp64 matrix cores) where the reference
 * inverts it by pivoted LU.  polar_iterations, dipole_rrms and iterator_failed stay 0 as in the reference; polar_max_iter, polar_precision,
 * polar_gamma, polar_gs, polar_rrms and solver are ignored.
 * Deliberate difference: when A is NOT positive definite (polarization catastrophe) the reference returns the unphysical LU answer; here the
 * evaluation completes with iterator_failed = 1 (every driver rejects such a configuration), dipoles and polarization_energy 0, and
 * mpmc_polar_direct_info names the pivot.
 * Trial moves of such a context run a FULL evaluation of the trial configuration (as polarizable Wolf boxes do): the solve is global.
 * mpmc_get_dipoles: ef_induced = mu / alpha - ef_static for polarizable atoms, 0 for the others (the reference leaves stale values there
 * on this path).
 * Memory: (3 n_pol rounded up to 192)^2 doubles for the factor (the lower triangle is used; the square is allocated); a factor that does
 * not fit the free device memory fails the evaluation with MPMC_ERR_MEMORY and a text that names the size.  Time: the factorisation and
 * the solves are counted in MPMC_K_DIPOLE_ITER, the build of A in MPMC_K_TENSOR. */
typedef struct mpmc_direct_info {
	int64_t n_unknowns;   /* 3 n_pol of the last direct solve of this context (0: none has run)                            */
	int64_t status;       /* 0, or the 1-based index (among the unknowns, device order) of the first non-positive pivot       */
	double residual;      /* max |E0 - A mu| / max |E0| over the unknowns, A mu from an independent matrix-free product       */
	int64_t factor_bytes; /* device memory held by the factor (counted in mpmc_memory_usage's total)                          */
} mpmc_direct_info;
int mpmc_polar_direct_info(mpmc_ctx *ctx, mpmc_direct_info *out);

/* ---- `polar_wolf`: the static field as a Wolf sum, System::thole_field_wolf (src/System.Energy.cpp:3337-3396) -----------------------------
 * With polarization on and rd_only off the setting replaces the static field whenever mpmc_options.polar_ewald is off (polar_ewald wins
 * when both are set, thole_field :3289-3294); the iterative solvers and the direct solve read the new field.  The pairs are those of
 * thole_field_nopbc (different molecules, not both frozen, r - 1e-12 < R, r != 0, R the cutoff of the box); such a pair adds
 * q_j f(r) d / r to atom i and -q_i f(r) d / r to atom j with
 *   a > 0:  f(r) = erfc(a r) / r^2 + 2 a / sqrt(pi) exp(-a^2 r^2) / r - [the same at r = R]          a = 0:  f(r) = 1 / r^2 - 1 / R^2
 * f vanishes at r = R and follows every change of the box.  polar_wolf_alpha outside [0, 1] or non-finite is refused with
 * MPMC_ERR_INVALID_SETTING (SimulationControl.cpp:2652-2660).  Both setters follow the lifetime of mpmc_set_axilrod_teller's switch: the
 * setting survives mpmc_set_atoms, mpmc_set_box, mpmc_set_options, position updates, accepted trials and capacity growth; enabled = 0
 * restores the behaviour of a context that never called them, to the bit.  MPMC_FLAG_POLAR_WOLF and MPMC_FLAG_POLAR_PALMO (the keywords
 * through mpmc_check_flags / mpmc_set_options) are still refused.  Trial moves of up to MPMC_TRIAL_MAX_ATOMS atoms keep the O(m N) path
 * unless mpmc_options.wolf is on.  Time: MPMC_K_FIELD.
 * Not supported, and refused by the input readers: `polar_wolf_full`, which changes every block of thole_amatrix (:2735-2757), and
 * `polar_wolf_alpha_lookup`, a table indexed by (int)(r * 1000): a different function of r that would need the reference's rounding of r
 * for every pair.
 *
 * ---- `polar_palmo`: the Palmo-Krimm correction (palmo_contraction :3602-3627, thole_iterative :3517-3519, polar() :2610-2618) ------------
 * With polar_iterative on, one more contraction runs behind the solver's last iteration, with the final dipoles: F_i = -sum_{j != i}
 * A_ij mu_j.  With E_ind,i = mu_i / alpha_i - E0_i, the induced field that iteration used (what mpmc_get_dipoles reports),
 *   ef_induced_change_i = F_i - E_ind,i for polarizable atoms, 0 for the others,
 *   polarization_energy = -1/2 sum mu . E0 - 1/2 sum mu . ef_induced_change;  energy and NU follow.
 * Under Gauss-Seidel sweeps (polar_gs) the contraction runs (MPMC_K_DIPOLE_ITER, its reduce in MPMC_K_REDUCE).  Under Jacobi iterations the
 * reference contracts the dipoles the last iteration read, so it subtracts from the induced field that very field, and under the direct
 * solve ef_induced_change is never written: there its correction is zero to the last bit, no contraction runs here and the correction
 * reported is exactly 0.  It is 0 too when iterator_failed is set (:3483-3488).
 * mpmc_polar_palmo_info: the correction of the last evaluation with a dipole solve (already part of its polarization_energy) and the
 * per-atom change, [n][3] in the caller's atom order. */
int mpmc_set_polar_wolf(mpmc_ctx *ctx, int enabled, double polar_wolf_alpha);
int mpmc_set_polar_palmo(mpmc_ctx *ctx, int enabled);
int mpmc_polar_palmo_info(mpmc_ctx *ctx, double *energy_correction, double *ef_induced_change /*[n][3], may be NULL*/);

/* ---- `polar_ewald_full`: the induced field as an Ewald sum too, System::ewald_full (src/System.Energy.cpp:2785-2830, 2944-3143) -----------
 * The one fully periodic dipole solve of the reference, which System::polar() tries before every other.  With polarization on and
 * rd_only off the setting replaces the whole solve; mpmc_polar and mpmc_thole_field follow it.  a = polar_ewald_alpha (unset: 3.5 /
 * cutoff), l = polar_damp, V the cell volume, R the cutoff of the box.
 *   static field  E0 = recip_term + real_term: the field of `polar_ewald on`, whatever polar_ewald says.  polar_ewald, polar_iterative,
 *                 polar_gs, polar_gamma, polar_rrms, mpmc_set_polar_wolf and mpmc_options.solver change nothing under the term.
 *   start         mu = alpha E0 (no polar_gamma)
 *   one pass      E_ind = real + reciprocal + correction, then mu = alpha (E0 + E_ind):
 *     real        every unordered pair with alpha_i != 0 and alpha_j != 0 that is not dropped by rimg > R (r = R is kept; frozen-frozen and
 *                 same-molecule pairs contribute), d the minimum-image vector, r = rimg, e = erfc(a r), g = exp(-a^2 r^2), t = l r:
 *                   s1 = e + 2 a r g / sqrt(pi) - (1 + t + t^2/2) exp(-t)
 *                   s2 = e + 2 a r g / sqrt(pi) + 4/3 a^3 r^3 g / sqrt(pi) - (1 + t + t^2/2 + t^3/6) exp(-t)
 *                   T = 3 d d^T s2 / r^5 - I s1 / r^3;   E_ind,i += T mu_j,  E_ind,j += T mu_i
 *     reciprocal  over the hemisphere of k vectors of recip_term: Pc = sum_j (k . mu_j) cos(k . r_j), Ps likewise with sin, over all atoms;
 *                 E_ind,i[p] += w_p (-sin(k . r_i) Ps - cos(k . r_i) Pc) for every atom, non-polarizable ones included.  The reference
 *                 overwrites its weight in a loop over p (:3015-3016), so w_p = (8 pi / V) exp(-k^2 / 4 a^2) / k^2 * k_z for all three
 *                 components: that is what it computes and what this library returns by default.  MPMC_PEF_VECTOR_KWEIGHT puts k_p in the
 *                 place of k_z, the weight the formula intends (ion216_polar: -785.44 K instead of -808.05 K).
 *     correction  E_ind,i += -4 pi / (3 V) sum_j mu_j + 4 a^3 / (3 sqrt(pi)) mu_i for every atom
 *   pass count    polar_precision == 0: polar_max_iter + 1 passes; otherwise until no component of the change of mu has a square above
 *                 (polar_precision * DEBYE2SKA)^2; after 128 passes the solve stops with iterator_failed = 1 and keeps its dipoles.
 *   results       polarization_energy = -1/2 sum mu . E0; polar_iterations and dipole_rrms are 0 (the reference never writes them on this
 *                 path); mpmc_get_dipoles returns the dipoles after the last update and the induced field of the last pass, which is
 *                 non-zero on non-polarizable atoms.
 * The setting has the lifetime of mpmc_set_polar_wolf's; enabled = 0 restores the context's behaviour to the bit.  Unknown flag bits are
 * refused with MPMC_ERR_INVALID_SETTING.  MPMC_FLAG_POLAR_EWALD_FULL in unsupported_flags is still refused: this call alone switches
 * the term on.  An evaluation with mpmc_set_polar_palmo on as well fails with MPMC_ERR_UNSUPPORTED (ewald_palmo_contraction, :3243-3267,
 * is not part of the library).  Every evaluation runs all its passes at once: the energy-from-moments form and mpmc_set_dipoles_on_demand
 * do not apply, and trial moves evaluate the trial configuration in full.  The pair factors (-s1 / r^3, 3 s2 / r^5) are stored once per
 * evaluation, 16 bytes per pair of the 64 x 64 tile-pair table, and streamed once per pass; a store or phase table that does not fit
 * the free device memory fails the evaluation with MPMC_ERR_MEMORY and a text that names the size.  Time: the store and the phases in
 * MPMC_K_TENSOR, the real-space contraction and the dipole structure factors in MPMC_K_DIPOLE_ITER, the update in MPMC_K_REDUCE.
 * mpmc_polar_ewald_full_info: of the last evaluation with the term on. */
#define MPMC_PEF_VECTOR_KWEIGHT 1 /* w_p uses k_p (the intended physics) instead of the reference's k_z for every p */
int mpmc_set_polar_ewald_full(mpmc_ctx *ctx, int enabled, int flags);
typedef struct mpmc_ewald_full_info {
	int32_t passes;       /* passes run                                                     */
	int32_t n_k;          /* k vectors of the reciprocal-space sum                          */
	int64_t n_real_pairs; /* pairs that pass the real-space predicate                       */
	int64_t store_bytes;  /* device bytes of the pair-factor store                          */
} mpmc_ewald_full_info;
int mpmc_polar_ewald_full_info(mpmc_ctx *ctx, mpmc_ewald_full_info *out);

/* ---- `polar_sor`, `polar_esor`, `polar_zodid`: relaxed dipole updates and zeroth-order dipoles (src/System.Energy.cpp:3450-3560, 3181-3211) ---
 * scheme (gamma = mpmc_options.polar_gamma; `it` = 1, 2, ... the iteration; new_mu = alpha (E0 + E_ind) the unrelaxed update):
 *   MPMC_POLAR_RELAX_SOR    mu = gamma new_mu + (1 - gamma) old_mu
 *   MPMC_POLAR_RELAX_ESOR   mu = (1 - exp(-gamma it)) new_mu + exp(-gamma it) old_mu
 * Under a scheme the start is mu_0 = alpha E0 without the polar_gamma factor (init_dipoles :3555).
 *   Jacobi iterations and Gauss-Seidel sweeps (thole_iterative): dipole_rrms and the precision test compare the UNRELAXED new_mu with
 *     old_mu; the blend is what the next iteration reads, and it is applied behind the last iteration too, so the energy and the dipoles
 *     returned are blended ones.  ef_induced is the last contraction's field.  Under sweeps new_mu is the swept vector; mpmc_set_polar_palmo
 *     contracts the swept, unblended dipoles and takes its energy term with the blended ones.  At 128 iterations of a precision-terminated
 *     solve the dipoles are alpha E0 and iterator_failed is set, as without a scheme.  SOR with gamma = 1 is the plain solve.
 *   mpmc_set_polar_ewald_full: the weight of pass k = 0, 1, ... is that of it = k + 1, new_mu itself is overwritten with the blend, and the
 *     precision test sees the blended value (new_dipoles :3196-3204); the start never carries polar_gamma.
 *   polar_iterative off: the scheme is never read.
 * zodid: "zeroth-order" dipoles, mu = alpha E0 (times polar_gamma when no scheme is on), no A matrix and no iteration: polar_iterations and
 *   dipole_rrms are 0, ef_induced is 0, the Palmo-Krimm term is 0, polarization_energy = -1/2 sum mu . E0.  No tensor store, panel table or
 *   dense matrix is built; a trial move of up to MPMC_TRIAL_MAX_ATOMS atoms is O(m N) end to end.  Under mpmc_set_polar_ewald_full zodid
 *   changes nothing.  With polarization on and polar_iterative off the evaluation fails with MPMC_ERR_INCOMPATIBLE (SimulationControl.cpp:2634).
 * polar_gamma < 0 with a scheme on fails the evaluation with MPMC_ERR_INVALID_SETTING (SimulationControl.cpp:2714-2730); an unknown scheme
 * is refused by the setter with the same code.  The energy-from-moments form and mpmc_set_dipoles_on_demand do not apply under a scheme or
 * zodid: every evaluation runs all its iterations.  The setting has the lifetime of mpmc_set_polar_wolf's and is refused while an
 * evaluation or a trial move is open; (MPMC_POLAR_RELAX_NONE, 0) restores the behaviour of a context that never called it, to the bit.
 * MPMC_FLAG_POLAR_SOR and MPMC_FLAG_POLAR_ZODID in unsupported_flags are still refused: this call alone switches the behaviour on.
 * mpmc_polar_relax_info: of the last evaluation with a dipole solve. */
#define MPMC_POLAR_RELAX_NONE 0
#define MPMC_POLAR_RELAX_SOR 1
#define MPMC_POLAR_RELAX_ESOR 2
int mpmc_set_polar_relax(mpmc_ctx *ctx, int scheme, int zodid);
typedef struct mpmc_relax_info {
	int32_t scheme;        /* MPMC_POLAR_RELAX_* of the context                                                             */
	int32_t zodid;         /* the context's zodid switch                                                                    */
	int32_t acted;         /* 1: a relaxed update or the zeroth-order shortcut ran in that evaluation                       */
	int32_t store_filled;  /* 1: that evaluation filled a tensor store (compact, dense or the ewald_full pair factors)      */
	int64_t contractions;  /* A . mu contractions it ran: iterations, sweeps or passes, + 1 for Palmo-Krimm; 0 under zodid  */
	double last_weight;    /* w_new of the last update (1 when none was relaxed)                                            */
} mpmc_relax_info;
int mpmc_polar_relax_info(mpmc_ctx *ctx, mpmc_relax_info *out);

/* ---- `polar_gs_ranked`: Gauss-Seidel sweeps in ranked order (src/System.cpp:1001-1029, src/System.Energy.cpp:3450-3543, 3631-3656) --------
 * The last member of the iterative family.  The sweeps are those of mpmc_options.polar_gs; what changes is their order from the second
 * iteration on.
 *   rank pass     once per evaluation, on the resident positions.  rmin = the smallest minimum-image distance rimg over all pairs of atoms
 *                 with polarizability != 0 (same-molecule and frozen pairs count; MAXVALUE = 1e40 when there is no such pair), the
 *                 reference's double to the bit.  rank_metric[i] = the number of such pairs that contain i and have r <= rmin * 1.5, where
 *                 r = sqrt(((dx dx) + dy dy) + dz dz) is the UNWRAPPED distance pair->r, not rimg: in a periodic box a pair that is close
 *                 only through an image does not count.  That is what the reference computes and what this library returns.  Atoms
 *                 that are not polarizable keep rank 0.
 *   order         update_ranking is a bubble sort run after every iteration that is followed by another: iteration 1 sweeps in atom
 *                 order, iterations 2, 3, ... in the stable descending order of rank_metric (ties in atom order).  With polar_max_iter 1,
 *                 or a precision met in iteration 1, no ranked sweep runs and the result is that of polar_gs to the bit.
 *   unchanged     the start vector, dipole_rrms, the precision test, the failure at 128 iterations, the polar_sor / polar_esor blend
 *                 (mpmc_set_polar_relax) and mpmc_set_polar_palmo behind the sweeps.
 * The setting acts with polarization on, rd_only off and polar_iterative on; it has no effect under polar_iterative off, zodid or
 * mpmc_set_polar_ewald_full (acted = 0, results as without it, to the bit).  An evaluation with mpmc_options.polar_gs on as well fails
 * with MPMC_ERR_INVALID_SETTING (SimulationControl.cpp:2732).  Where it acts the atoms keep the caller's order on the device and the
 * solver is matrix-free, as under polar_gs; the energy-from-moments form and mpmc_set_dipoles_on_demand do not apply, and trial moves
 * evaluate the trial configuration in full.  The setting has the lifetime of mpmc_set_polar_relax's (kept across atoms, cell, accepted
 * trials and capacity growth; refused while an evaluation or a trial move is open); enabled = 0 restores the context's behaviour to the
 * bit.  MPMC_FLAG_POLAR_GS_RANKED in unsupported_flags is still refused: this call alone switches the behaviour on.  Time: the rank
 * pass, the order, the gathers and the view's tile classes in MPMC_K_CLASSES, the view's in-tile blocks in MPMC_K_TENSOR.
 * mpmc_polar_gs_ranked_info: of the last evaluation with a dipole solve.  mpmc_polar_gs_ranked_get: rank_metric and the sweep order
 * (order[p] = the atom swept p-th from iteration 2 on) of the last evaluation, in the caller's atom order, either pointer may be NULL;
 * MPMC_ERR_ARG when no evaluation in which the setting acted has been made since the atoms, the cell or the setting last changed. */
int mpmc_set_polar_gs_ranked(mpmc_ctx *ctx, int enabled);
typedef struct mpmc_gs_ranked_info {
	int32_t enabled;        /* the context's switch                                                      */
	int32_t acted;          /* 1: that evaluation made the rank pass and swept under the setting         */
	double rmin;            /* smallest image distance between polarizable atoms (1e40: none)            */
	int32_t max_rank;       /* largest rank_metric                                                       */
	int32_t n_moved;        /* places of the sweep order that differ from the identity                   */
	int32_t ranked_sweeps;  /* sweeps of that evaluation that ran in ranked order                        */
	int32_t reserved;
} mpmc_gs_ranked_info;
int mpmc_polar_gs_ranked_info(mpmc_ctx *ctx, mpmc_gs_ranked_info *out);
int mpmc_polar_gs_ranked_get(mpmc_ctx *ctx, int32_t *rank_metric /*[n]*/, int32_t *order /*[n]*/);

/* per-atom results written back by energy() in the reference (src/Atom.h:41-47); any pointer may be NULL.  After an on-demand evaluation
 * (mpmc_set_dipoles_on_demand above) the remaining Jacobi iterations run here first; MPMC_ERR_ARG when they no longer can. */
int mpmc_get_dipoles(mpmc_ctx *ctx, double *mu, double *ef_static, double *ef_induced /* each [n][3] */);
/* pairs() tail: update_com + wrap_all (src/System.cpp:1347-1425).  Host-side O(N); needs mass in set_atoms.
 * com / wrapped_com: [n_molecules][3]; wrapped_pos: [n][3]; any may be NULL. */
int mpmc_update_com(mpmc_ctx *ctx, double *com, double *wrapped_com, double *wrapped_pos, int *n_molecules);

/* ---- SimulationControl::PI_calculate_potential (PathIntegral.cpp:752-805) ------------------------------ */
/* Evaluates energy() on the n_local beads owned by this process (all enqueued before any wait, one stream per
 * bead) and returns the UN-normalised ordered sums {rd, coulombic, polarization, vdw} over those beads in
 * sums4.  per_bead (may be NULL) receives n_local mpmc_result.  The cross-rank combine (4 fp64 all-reduce over
 * RCCL / MPI_Allgather in the reference, :763-766) is the caller's; mpmc_pi_finish divides by P. */
int mpmc_pi_potential_local(mpmc_ctx **beads, int n_local, double sums4[4], mpmc_result *per_bead, int *any_iterator_failed);
/* The same, with every bead's coordinates handed over in HOST memory (pos[b]: n x 3 doubles in the caller's atom order -- what the
 * reference's bead loop holds, PathIntegral.cpp:759-775): bead b's upload is followed at once by its enqueue, so the uploads overlap
 * the evaluations of the beads in front of them instead of standing in front of the whole step. */
int mpmc_pi_potential_local_host(mpmc_ctx **beads, int n_local, const double *const *pos, double sums4[4], mpmc_result *per_bead,
                                 int *any_iterator_failed);
/* systems that shared each launch of the dipole iterations in this context's last evaluation: always 1 since ABI 4 (every bead runs
 * on its own streams; the lockstep form of rounds 1-2 was measured slower and removed).  Kept so that ABI 3 callers still link. */
int mpmc_last_batch_size(mpmc_ctx *ctx);
/* obs = sums / P ; returns V = rd + coulombic + vdw + polarization (:786-804) */
double mpmc_pi_finish(const double sums4_global[4], int P, double obs4[4]);

/* ---- the cross-GPU exchange of PI_calculate_potential on RCCL over xGMI ------------------------------------------
 * Reference: MPI_Allgather x 4 of one double per rank, then the ordered sum s = 0..P-1 (PathIntegral.cpp:763-766, :786-801).
 * Here: ONE ncclAllGather of `stride` fp64 per bead, then the same ordered sum on the host (bit-identical on every rank).
 * Bead s lives on rank s % n_ranks, local slot s / n_ranks.  RCCL is opened with dlopen at first use (mpmc_rccl_library_path);
 * without it these calls fail with MPMC_ERR_COMM and nothing else in the library is affected.
 *   one process per GPU : rank 0 calls mpmc_comm_unique_id, the host program carries the 128 bytes to the other ranks
 *                         (MPI_Bcast, a file, the torch.distributed store), every rank calls mpmc_comm_init_rank;
 *   one process, G GPUs : mpmc_comm_init_all / mpmc_pi_allreduce. */
typedef struct mpmc_comm mpmc_comm;
#define MPMC_COMM_ID_BYTES 128
int mpmc_rccl_version(int *version); /* ncclGetVersion: e.g. 22707 */
/* (ABI 6) the file the RCCL entry points were resolved from and why that copy, e.g. "/opt/rocm/lib/librccl.so.1 (next to the bound
 * libamdhip64)"; "" when RCCL could not be opened.  Order: $MPMC_RCCL_LIB, a librccl.so.1 the host program already mapped (shared, not
 * duplicated), the copy next to the HIP runtime this library is bound to, the loader's search path; always RTLD_LOCAL. */
const char *mpmc_rccl_library_path(void);
int mpmc_comm_unique_id(char id[MPMC_COMM_ID_BYTES]);
int mpmc_comm_init_rank(mpmc_comm **out, int n_ranks, int rank, const char id[MPMC_COMM_ID_BYTES], int device);
int mpmc_comm_init_all(mpmc_comm **out, int n_devices, const int *devices /* NULL: 0..n_devices-1 */);
int mpmc_comm_destroy(mpmc_comm *comm);
int mpmc_comm_info(const mpmc_comm *comm, int *n_ranks, int *rank, int *n_local_devices);
const char *mpmc_comm_last_error(const mpmc_comm *comm); /* comm may be NULL: last error of this thread */
/* all[r][0..count) = rank r's local[0..count)   (communicators of mpmc_comm_init_rank) */
int mpmc_comm_allgather_f64(mpmc_comm *comm, const double *local, int64_t count, double *all /*[n_ranks][count]*/);
/* local[n_local][stride] in local-slot order  ->  all[P][stride] in BEAD order, P = n_local * n_ranks.  stride 4 = the
 * {rd, coulombic, polarization, vdw} of PI_calculate_potential; 3 * n_molecules = the centres of mass of the kinetic estimator. */
int mpmc_pi_gather_beads(mpmc_comm *comm, const double *local, int n_local, int stride, double *all);
/* One process driving several GPUs: beads[b] may live on any device (the usual placement is b mod G).  Evaluates energy() on every
 * bead -- one host thread per device, all of a device's beads enqueued before the first wait -- gathers the per-bead values over a
 * process-wide ncclCommInitAll communicator of the devices involved, and returns the UN-normalised ordered sums over beads 0..n-1
 * (identical on every device: an all-reduce with a fixed summation order).  mpmc_pi_finish divides by P. */
int mpmc_pi_allreduce(mpmc_ctx **beads, int n_beads, double sums4[4], mpmc_result *per_bead, int *any_iterator_failed);
/* (ABI 5) what mpmc_pi_allreduce uses for these beads: the number of distinct devices they live on and the size of the process-wide
 * communicator of those devices (0 before the first mpmc_pi_allreduce on them) -- a host program's proof that RCCL saw G ranks. */
int mpmc_pi_allreduce_info(mpmc_ctx **beads, int n_beads, int *n_devices, int *comm_n_ranks);

/* ---- Gibbs ensemble: the two boxes of SimulationControl::Gibbs_mc -------------------------------------------------------
 * Reference: final_energy[0] = systems[0]->energy(); final_energy[1] = systems[1]->energy(); (src/SimulationControl.Gibbs.cpp:179-180),
 * then boltzmann_factor_NVT_Gibbs (:358-522).  The boxes are independent evaluations: box 0 -> device 0, box 1 -> device 1 of the node
 * (mpmc_ctx_create's device argument); mpmc_gibbs_energy enqueues both before it waits for either. */
int mpmc_gibbs_energy(mpmc_ctx *box_a, mpmc_ctx *box_b, mpmc_result *out_a, mpmc_result *out_b);
/* move types as the reference enumerates them (src/constants.h:87-95) */
#define MPMC_MOVETYPE_INSERT 0
#define MPMC_MOVETYPE_REMOVE 1
#define MPMC_MOVETYPE_DISPLACE 2
#define MPMC_MOVETYPE_ADIABATIC 3
#define MPMC_MOVETYPE_SPINFLIP 4
#define MPMC_MOVETYPE_VOLUME 5
#define MPMC_MOVETYPE_PERTURB_BEADS 6
typedef struct mpmc_gibbs_move {
	int32_t movetype[2];       /* sys[i]->checkpoint->movetype                                                  */
	double temperature;        /* sys[0]->temperature                                                           */
	double init_energy[2];     /* energies of the accepted configuration                                        */
	double final_energy[2];    /* systems[i]->energy() after the move (may be non-finite: bad contact)          */
	double N[2], volume[2];    /* sys[i]->observables->N / ->volume AFTER the move                              */
	double checkpoint_volume_0; /* sys[0]->checkpoint->observables->volume (the volume the move started from)   */
} mpmc_gibbs_move;
/* boltzmann_factor[i] = sys[i]->nodestats->boltzmann_factor; energy[i] (may be NULL) receives MAXVALUE where the reference overwrites
 * observables->energy on a bad contact.  Entries the reference leaves untouched are left untouched.  Returns MPMC_OK, or the
 * reference's throw codes 20000 / 102, or MPMC_ERR_UNSUPPORTED for spin-flip moves (quantum rotation is outside the path). */
int mpmc_gibbs_boltzmann_factor(const mpmc_gibbs_move *move, double boltzmann_factor[2], double energy[2]);

/* ---- `cavity_bias on`: the cavity grid of uVT moves, System::cavity_update_grid (src/System.Cavity.cpp:15-188) ---------------------------
 * In front of every move (System::make_move, src/System.MonteCarlo.cpp:731-735) the reference bins every atom against a G x G x G grid of
 * sphere centres, counts the spheres that hold no atom (cavities_open, cavity_bias_probability) and estimates their joint volume with
 * (int)(0.1 V) darts (update_cavity_volume).  A biased insertion then puts the molecule's centre of mass on one empty centre (:742-764) and
 * the acceptance factor carries cavity_volume * cavity_bias_probability (:1368-1389).  Here the binning, the count, the ordered list of empty
 * centres and the darts run on the device; the random stream stays the driver's.
 *   mpmc_set_cavity_grid   grid_size = 0 switches the grid off.  On: grid_size < 0, radius <= 0 or non-finite, or grid_size above
 *                          MPMC_CAVITY_MAX_GRID is MPMC_ERR_INVALID_SETTING (SimulationControl.cpp:2157-2162).  The setting has the lifetime of
 *                          mpmc_set_polar_wolf's (it survives mpmc_set_atoms, mpmc_set_box, mpmc_set_options and capacity growth).  A context
 *                          that never switches the grid on allocates nothing for it, launches nothing more and returns the same bits.
 *   mpmc_cavity_update     works on the accepted atom list (it needs masses: the atoms enter at the reference's wrapped_pos, what
 *                          mpmc_update_com returns: the position minus the lattice shift of the molecule's centre of mass, frozen molecules
 *                          unshifted).  dart_frac: the caller's `-0.5 + get_rand()` triples in draw order, n_darts of them (the reference throws
 *                          mpmc_cavity_num_darts(volume)); n_darts = 0 is allowed, dart_frac may then be NULL and cavity_volume is 0.0 / 0.0 *
 *                          volume, NaN, as in the reference.  Refused with MPMC_ERR_ARG and a text: the grid is off, no box or atoms, no
 *                          masses, a trial move open.  It may follow an accepted exchange trial directly; it changes nothing an evaluation
 *                          or a trial reads.
 *   arithmetic             sphere centre (i, j, k): comp[q] = (idx_q + 1) / (G + 1); v[p] = sum_q basis[q][p] comp[q], then minus
 *                          0.5 basis[q][p] for q = 0, 1, 2.  dart: pos[p] = sum_q basis[q][p] dart_frac[q].  r = sum_p d_p d_p with d = centre -
 *                          atom, respectively dart - centre; inside means sqrt(r) < radius, strict, decided on r itself against
 *                          mpmc_cavity_r2_threshold(radius).  No minimum image.  Products and sums are not fused.  occupancy = atoms inside
 *                          (a count); cavities_open = centres with none; probability = open / G^3; a dart hits when it lies inside some
 *                          empty sphere; cavity_volume = (hits / n_darts) * volume.  All counts are exact; the doubles are the reference's bits.
 *   mpmc_cavity_point      the open_rank-th empty centre in the reference's enumeration order (i outermost, k innermost): cavities_array[
 *                          random_index] of make_move.  MPMC_ERR_ARG when the rank is out of range, or when no update has been made since
 *                          the grid setting, the cell or the atom list (positions included) last changed.
 *   mpmc_cavity_get        occupancy [G^3], centres [G^3][3] and the flat indices (i G + j) G + k of the empty centres, ascending
 *                          [cavities_open]; any pointer may be NULL.  Same validity rule.
 * Host only, no device needed (like mpmc_pbc_compute): mpmc_cavity_num_darts = (int)(volume * 0.1); mpmc_cavity_grid_point;
 * mpmc_cavity_r2_threshold = the smallest double whose correctly rounded square root is >= radius (NaN for radius <= 0 or non-finite);
 * mpmc_uvt_boltzmann_factor = the ENSEMBLE_UVT branch of System::boltzmann_factor (:1358-1422) for INSERT / REMOVE / DISPLACE in the reference's
 * operand order, the biased form when biased_move != 0, with ATM2REDUCED = 0.0073389366; fugacity is the value the reference would pick
 * (pressure, fugacities[0] or fugacities[sorbateInsert]), N = observables->N as the reference reads it there, avg_cavity_probability the
 * driver's running average.  Any other move type: MPMC_ERR_UNSUPPORTED.
 * Not part of the library: a uVT driver and the fugacity equations of state.  (cavity_autoreject: mpmc_set_cavity_autoreject.) */
#define MPMC_CAVITY_MAX_GRID 128 /* 128^3 = 2 M sphere centres */
int mpmc_set_cavity_grid(mpmc_ctx *ctx, int grid_size, double radius);
typedef struct mpmc_cavity_result {
	int64_t total_points, cavities_open, n_darts, hits;
	double probability, cavity_volume;
} mpmc_cavity_result;
int mpmc_cavity_update(mpmc_ctx *ctx, int n_darts, const double *dart_frac /* [n_darts][3] */, mpmc_cavity_result *out);
int mpmc_cavity_point(mpmc_ctx *ctx, int64_t open_rank, double pos[3]);
int mpmc_cavity_get(mpmc_ctx *ctx, int32_t *occupancy /* [G^3] */, double *grid_pos /* [G^3][3] */, int32_t *open_flat_index /* [cavities_open] */);
int mpmc_cavity_num_darts(double volume);
int mpmc_cavity_grid_point(const double basis[9], int grid_size, int i, int j, int k, double pos[3]);
double mpmc_cavity_r2_threshold(double radius);
typedef struct mpmc_uvt_move {
	int32_t movetype, biased_move, sorbate_count; /* checkpoint->movetype (MPMC_MOVETYPE_*), checkpoint->biased_move, sorbateCount */
	double temperature, fugacity, volume, N, init_energy, final_energy, cavity_volume, avg_cavity_probability;
} mpmc_uvt_move;
int mpmc_uvt_boltzmann_factor(const mpmc_uvt_move *move, double *boltzmann_factor);
/* (measurement) device milliseconds of the last mpmc_cavity_update made under mpmc_set_profiling: { occupancy, compaction, darts } */
int mpmc_debug_cavity_times(mpmc_ctx *ctx, double ms3[3]);

/* ---- SimulationControl::PI_calculate_kinetic (PathIntegral.cpp:806-824) and its chain measure (:851-965) ----
 * Host-side O(P * n_molecules); no device work.  com: centres of mass [P][n_molecules][3] of the P images of every
 * molecule (Molecule::update_COM, src/Molecule.cpp:259-281; mpmc_update_com returns one bead's block),
 * mol_mass[n_molecules] = Molecule::mass of image 0, movable[m] != 0 iff image 0 of molecule m is neither frozen,
 * adiabatic nor target (:881).  Returns sum_m M_m * AMU2KG * 1e-20 * sum_i |com_i - com_{(i+1)%P}|^2  [kg m^2]. */
double mpmc_pi_chain_mass_length2(int P, int n_molecules, const double *com, const double *mol_mass, const int32_t *movable);
/* K [Kelvin] = (1/kB) * (0.5*3*N*kB*T*P - 0.5*omega2*chain_mass_len2), omega2 = P / (beta^2 hBar2)  (Tuckerman 12.5.12);
 * N = System::countN() of image 0. */
double mpmc_pi_kinetic(double chain_mass_len2, double orient_mu_len2, double N, int P, double temperature);

/* ---- measurement ------------------------------------------------------------------------------------- */
int mpmc_set_profiling(mpmc_ctx *ctx, int enabled); /* HIP-event timing of each kernel class on ctx's stream */
int mpmc_get_timings(mpmc_ctx *ctx, mpmc_timings *out, int reset);
int mpmc_synchronize(mpmc_ctx *ctx);
/* bytes of device memory held by the context and by its Thole tensor store */
int mpmc_memory_usage(mpmc_ctx *ctx, int64_t *total_bytes, int64_t *tensor_store_bytes);

/* tile-pair statistics of the LAST evaluation (64 x 64 atom tiles; orthorhombic cells are classified by the
 * minimum-image distance between tile bounding boxes): out4 = { tile pairs, pairs whose Thole tensors are stored and
 * streamed (64 KiB each), pairs beyond the damping range (bare dipole tensor recomputed), pairs wholly beyond the cutoff } */
int mpmc_get_tile_stats(mpmc_ctx *ctx, int64_t out4[4]);

/* ---- diagnostics (no effect on results) -------------------------------------------------------------------
 * How this context's host-side waits ended since it was created: out4 = { polls of the pinned result block that saw the device's post,
 * polls that ran out of their budget (the wait then synchronised the stream), stream synchronisations, yields taken inside long polls }.
 * Short evaluations and trial moves are polled for (a few microseconds earlier than the driver's completion path); a host with fewer
 * free cores than polling threads shows up here as timeouts and yields. */
int mpmc_debug_wait_counters(mpmc_ctx *ctx, long long out4[4]);
/* The sort of `polar_gs_ranked` on keys of the caller's: order[p] = the atom at place p of the stable descending order of keys[0 .. n),
 * n the atoms of the context.  The rank pass itself cannot produce a key above about 60 (atoms no closer than rmin within 1.5 rmin of
 * one of them); the sort takes any values.  It overwrites what mpmc_polar_gs_ranked_get hands out. */
int mpmc_debug_gs_rank_order(mpmc_ctx *ctx, const int32_t *keys /*[n]*/, int32_t *order /*[n]*/);
/* The tile-pair classes of the ranked view that the last evaluation under `polar_gs_ranked` swept (rebuilt from the atoms in sweep order):
 * out6 = { tile pairs, off-diagonal tile pairs, of those: far, beyond the cutoff, with one periodic image index for the whole tile pair
 * in some dimension, with such an image that is not the zero image }.  Read-only. */
int mpmc_debug_gs_ranked_pair_stats(mpmc_ctx *ctx, int64_t out6[6]);
/* Measurement / A-B switch, key = value (keys: csrc/context.cpp, struct mpmc_tuning).  ctx == NULL: the default of contexts created
 * afterwards in this process.  The library reads no environment variable for any of these. */
int mpmc_debug_configure(mpmc_ctx *ctx, const char *key, double value);

#ifdef __cplusplus
}
#endif
#endif /* MPMC_ENERGY_H */
