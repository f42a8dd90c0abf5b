// evaluate.cpp -- one energy evaluation: k tables, work buffers, the enqueue of every kernel of double System::energy(), result assembly, component entry points
// (part of libmpmc_energy.so; shared state and helpers: context.h.  There is no CPU fallback anywhere in this library.)
#include "context.h"


using namespace mpmc;

// ---- k-vector tables (hemisphere enumeration of coulombic_reciprocal :1577-1590 / recip_term :2849-2865) --------
static int build_k_tables(mpmc_ctx *c) {
	const int kmax = c->opts.ewald_kmax;
	const double alpha = c->ewald_alpha, ea = c->polar_ewald_alpha;
	// the set of l-vectors depends on kmax alone: count it, make room (device tables and ONE persistent pinned staging block), fill the
	// staging block in place and copy asynchronously -- a volume move rebuilds these tables every time, and four blocking copies from
	// pageable vectors plus a stream synchronisation cost more than the reciprocal-space kernels they feed
	auto each_lvec = [kmax](auto &&visit) { // the hemisphere of integer l-vectors inside the sphere of radius kmax, in the reference's order
		int l[3];
		for (l[0] = 0; l[0] <= kmax; l[0]++)
			for (l[1] = (!l[0] ? 0 : -kmax); l[1] <= kmax; l[1]++)
				for (l[2] = ((!l[0] && !l[1]) ? 1 : -kmax); l[2] <= kmax; l[2]++)
					if (l[0] * l[0] + l[1] * l[1] + l[2] * l[2] <= kmax * kmax) visit(l);
	};
	int K = 0, rc;
	each_lvec([&K](const int *) { K++; });
	if ((size_t)K > c->d_lvec.cap) c->lvec_kmax = -1; // (a fresh d_lvec holds zeros)
	if ((rc = c->d_kvec.reserve(c, (size_t)K)) != MPMC_OK) return rc;
	if ((rc = c->d_kw.reserve(c, (size_t)K)) != MPMC_OK) return rc;
	if ((rc = c->d_lvec.reserve(c, (size_t)K)) != MPMC_OK) return rc;
	if ((rc = c->d_w_en.reserve(c, (size_t)K)) != MPMC_OK) return rc;
	if ((rc = c->d_sf.reserve(c, (size_t)K)) != MPMC_OK) return rc;
	if (K > 0) {
		if (c->kstage_in_flight) { // (one rebuild per evaluation at most, and evaluations are waited for: normally long done)
			HIP_TRY(c, hipEventSynchronize(c->ev_kstage));
			c->kstage_in_flight = false;
		}
		if ((rc = c->h_kstage.reserve(c, (size_t)K * (2 * sizeof(double4) + sizeof(double) + sizeof(int4)))) != MPMC_OK) return rc;
		if (!c->ev_kstage) HIP_TRY(c, hipEventCreateWithFlags(&c->ev_kstage, hipEventDisableTiming));
		// (the 16-byte types first: behind an odd number of doubles an int4 array would be misaligned -- found by tools/host_asan.sh)
		double4 *kvec = reinterpret_cast<double4 *>(c->h_kstage.p), *kw = kvec + K;
		int4 *lvec = reinterpret_cast<int4 *>(kw + K);
		double *wen = reinterpret_cast<double *>(lvec + K);
		int n = 0;
		each_lvec([&](const int *l) {
			double k[3];
			for (int p = 0; p < 3; p++) {
				k[p] = 0;
				for (int q = 0; q < 3; q++) k[p] += 2.0 * kPi * c->box.r[3 * p + q] * l[q];
			}
			const double k2 = k[0] * k[0] + k[1] * k[1] + k[2] * k[2];
			kvec[n] = make_double4(k[0], k[1], k[2], k2);
			lvec[n] = make_int4(l[0], l[1], l[2], 0);
			wen[n] = std::exp(-k2 / (4.0 * alpha * alpha)) / k2;
			const double g = std::exp(-k2 / (4.0 * ea * ea));
			kw[n] = make_double4(k[0] / k2 * g, k[1] / k2 * g, k[2] / k2 * g, 0.0);
			n++;
		});
		HIP_TRY(c, hipMemcpyAsync(c->d_kvec, kvec, K * sizeof(double4), hipMemcpyHostToDevice, c->stream));
		HIP_TRY(c, hipMemcpyAsync(c->d_kw, kw, K * sizeof(double4), hipMemcpyHostToDevice, c->stream));
		HIP_TRY(c, hipMemcpyAsync(c->d_w_en, wen, K * sizeof(double), hipMemcpyHostToDevice, c->stream));
		if (c->lvec_kmax != kmax) {
			HIP_TRY(c, hipMemcpyAsync(c->d_lvec, lvec, K * sizeof(int4), hipMemcpyHostToDevice, c->stream));
			c->lvec_kmax = kmax;
		}
		HIP_TRY(c, hipEventRecord(c->ev_kstage, c->stream));
		c->kstage_in_flight = true;
	}
	c->K = K;
	return MPMC_OK;
}

constexpr int kDenseChunks = 16; // row chunks (= partial slots) of the dense matrix-vector product
constexpr int kOneStreamMinInflight = 4; // evaluations in flight from which on an evaluation keeps to one stream
constexpr int kCheckEvery = 4;         // precision-terminated Jacobi solve: host reads the device-side verdict once per this many iterations
constexpr int kSingleLaunchTiles = 32; // <= 2048 atoms (528 tile pairs): LJ-only evaluations run as ONE launch

static int ensure_polar_buffers(mpmc_ctx *c) {
	const size_t np = (size_t)c->max_pad;
	int rc;
	if ((rc = c->d_e_static.reserve(c, 3 * np)) != MPMC_OK) return rc;
	if ((rc = c->d_mu[0].reserve(c, 3 * np)) != MPMC_OK) return rc;
	if ((rc = c->d_mu[1].reserve(c, 3 * np)) != MPMC_OK) return rc;
	if ((rc = c->d_e_induced.reserve(c, 3 * np)) != MPMC_OK) return rc;
	if ((rc = c->d_rrms.reserve(c, np)) != MPMC_OK) return rc;
	if ((rc = c->d_e_recip_part.reserve(c, recip_slices_capacity(np))) != MPMC_OK) return rc;
	if ((rc = c->d_e_real.reserve(c, 3 * np)) != MPMC_OK) return rc;
	if ((rc = c->d_e_real_trial.reserve(c, 3 * np)) != MPMC_OK) return rc;
	if ((rc = c->d_gs_ul.reserve(c, 6 * np)) != MPMC_OK) return rc; // Gauss-Seidel sweeps: fields of the tiles above / below
	if ((rc = c->d_palmo_f.reserve(c, 3 * np)) != MPMC_OK) return rc;
	if ((rc = c->d_palmo_change.reserve(c, 3 * np)) != MPMC_OK) return rc;
	if (polar_moments_apply(c) && (rc = reserve_dk_ring(c)) != MPMC_OK) return rc;
	// per-atom partial slots: one per source tile (symmetric kernels) -- also covers the n_split <= n_tiles slots of the matrix-free
	// row kernel -- and never fewer than the kDenseChunks row chunks the dense matrix-vector product writes (small systems have fewer
	// tiles than that: the dense solver used to write past the end of this buffer, into the matrix that was allocated right behind it)
	const size_t need = (size_t)std::max(c->n_tiles, kDenseChunks) * c->n_pad * 3;
	return c->d_part.reserve(c, need);
}

// resolve alpha defaults, rebuild k tables when box/options changed
int mpmc::prepare(mpmc_ctx *c, bool defer_static) {
	if (!c->box_set) return fail(c, MPMC_ERR_BOX, "energy: no box set (mpmc_set_box)");
	if (!c->atoms_set) return fail(c, MPMC_ERR_INVALID_DATUM, "energy: no atoms set (mpmc_set_atoms)");
	HIP_TRY(c, hipSetDevice(c->device));
	if (c->opts.feynman_hibbs && c->h_mass.empty())
		return fail(c, MPMC_ERR_INVALID_DATUM, "energy: feynman_hibbs needs atom masses (mpmc_set_atoms was called without them)");
	if (c->atoms_dirty) {
		int rc = upload_atoms(c);
		if (rc != MPMC_OK) return rc;
	}
	if (c->k_dirty) {
		// System::update_pbc, reference src/System.cpp:871-874
		c->ewald_alpha = (c->opts.ewald_alpha > 0) ? c->opts.ewald_alpha : 3.5 / c->box.cutoff;
		c->polar_ewald_alpha = (c->opts.polar_ewald_alpha > 0) ? c->opts.polar_ewald_alpha : 3.5 / c->box.cutoff;
		int rc = build_k_tables(c);
		if (rc != MPMC_OK) return rc;
		c->k_dirty = false;
	}
	// pair LRC (O(N) moment form), self LRC, Ewald self term: position independent (lj_lrc_corr / lj_lrc_self :1036-1096, coulombic_self
	// :1626-1643), cached in h_static.  A general evaluation takes them along when they are stale (defer_static: enqueue() launches the
	// kernel behind its clear of the scalar block and wait_and_fill adopts the three values); everybody else gets them here and now.
	if (c->static_dirty && !defer_static) {
		c->scal_clean = false; // (the kernel writes its slots of the scalar block: the next evaluation clears the block first)
		launch_atom_terms(c->stream, atoms_view(c), lrc_box(c), c->ewald_alpha, c->opts.rd_lrc, /*self term*/ 1, c->d_atom_part, c->d_scal);
		HIP_TRY(c, hipGetLastError());
		double tmp[S_COUNT];
		HIP_TRY(c, hipMemcpyAsync(tmp, c->d_scal, sizeof(tmp), hipMemcpyDeviceToHost, c->stream));
		HIP_TRY(c, hipStreamSynchronize(c->stream));
		c->h_static[0] = tmp[S_LRC_PAIR];
		c->h_static[1] = tmp[S_LRC_SELF];
		c->h_static[2] = tmp[S_ES_SELF];
		c->static_dirty = false;
	}
	return MPMC_OK;
}

// lj_lrc_corr / lj_lrc_self take the cutoff lj() hands them (:916-919, 931, 1028): under rd_crystal 2 cutoff (order - 0.5).  Only the cutoff
// and the volume of this box are read by the atom-terms kernels.
Box mpmc::lrc_box(const mpmc_ctx *c) {
	Box b = c->box;
	if (crystal_on(c)) b.cutoff = 2.0 * c->box.cutoff * ((double)c->kept.rc_order - 0.5);
	return b;
}
CrystalParams mpmc::crystal_params(const mpmc_ctx *c) {
	CrystalParams cp = c->rc_par;
	FusedParams fp{};
	ext_params(c, fp, false);
	cp.fh_order = fp.fh_order;
	cp.fh_c2 = fp.fh_c2;
	cp.fh_c4 = fp.fh_c4;
	return cp;
}

RdModelParams mpmc::rd_model_params(const mpmc_ctx *c) {
	RdModelParams rp{};
	rp.form = c->kept.rdm_form;
	rp.mix = c->kept.rdm_mix;
	rp.t_in = (rp.form == RD_FORM_LJ) ? c->box.t_lj : c->box.t_es; // (rimg - 1e-12 < cutoff :934 | !(rimg > cutoff) :1229, :2127)
	if (rp.form == RD_FORM_LJ) { // (lj_buffered_14_7() and dreiding() carry no Feynman-Hibbs correction)
		FusedParams fp{};
		ext_params(c, fp, false);
		rp.fh_order = fp.fh_order;
		rp.fh_c2 = fp.fh_c2;
		rp.fh_c4 = fp.fh_c4;
	}
	return rp;
}

AtomsDev mpmc::atoms_view(const mpmc_ctx *c) {
	AtomsDev a;
	a.xyzq = c->d_xyzq;
	a.lj = c->d_lj;
	a.mf = c->d_mf;
	a.alpha = c->d_alpha;
	a.eps = c->d_eps;
	a.inv_molmass = c->d_inv_molmass;
	a.n = c->n;
	a.n_pad = c->n_pad;
	return a;
}
RecipDev mpmc::recip_view(const mpmc_ctx *c) {
	RecipDev r;
	r.kvec = c->d_kvec;
	r.w_en = c->d_w_en;
	r.kw = c->d_kw;
	r.lvec = c->kept.tune.no_recip_tab ? nullptr : c->d_lvec;
	r.sf = c->d_sf;
	r.K = c->K;
	return r;
}

// the tile pairs' common-image lattice vectors, or null when the tile-pair-wide images are switched off (the kernels then take every image per pair)
static inline const double4 *shift_view(const mpmc_ctx *c) { return (c->kept.tune.no_uniform || c->kept.tune.no_classes) ? nullptr : c->d_tp_shift.p; }

// the Wolf / Feynman-Hibbs fields of the pair parameters (pair sweep and per-move delta kernels)
void mpmc::ext_params(const mpmc_ctx *c, FusedParams &fp, bool wolf_on) {
	const mpmc_options &o = c->opts;
	fp.wolf = wolf_on ? 1 : 0;
	fp.fh_order = o.feynman_hibbs ? ((o.feynman_hibbs_order == 4) ? 4 : 2) : 0;
	fp.fh_c2 = fp.fh_c4 = 0.0;
	if (fp.fh_order) { // reference constants.h:15-33: M2A2 hBar2 / (24 kB T) and M2A4 hBar4 / (1152 kB2 T^2), reduced mass in kg
		const double hBar2 = 1.11211999e-68, hBar4 = 1.23681087e-136, kB = 1.3806503e-23, kB2 = 1.90619525e-46, amu = 1.66053873e-27;
		fp.fh_c2 = 1.0e20 * (hBar2 / (24.0 * kB * o.temperature)) / amu;
		fp.fh_c4 = 1.0e40 * (hBar4 / (1152.0 * kB2 * o.temperature * o.temperature)) / (amu * amu);
	}
	fp.wolf_erfa_over_r = std::erf(c->ewald_alpha * c->box.cutoff) / c->box.cutoff;
	fp.wolf_inv_r2 = 1.0 / (c->box.cutoff * c->box.cutoff);
}

// two waves per tile pair in the fast pair sweep (half-length workgroups): by default for the LAST quarter of the work table only -- a lone
// launch drains on units half as long, an ensemble (whose other kernels fill the drain anyway) pays the halved form's overhead on a quarter of
// the work.  The rule is a function of the table alone (never of the call): an evaluation gives the same bits alone and inside an ensemble.
static inline int sweep_split_mode(const mpmc_ctx *c) { return c->kept.tune.pair_split < 0 ? 2 : (c->kept.tune.pair_split != 0 ? 1 : 0); }
static inline int sweep_split_tail(const mpmc_ctx *c) {
	const int permille = c->kept.tune.pair_split_tail >= 0 ? c->kept.tune.pair_split_tail : kSweepSplitTailPermille;
	return (int)((long long)c->n_sweep_blocks * permille / 1000);
}

// ---- the plan of one evaluation ---------------------------------------------------------------------------------------------------------
// Everything enqueue() decides, decided once and in one place, from the context's state alone: no HIP call, no allocation.  make_room()
// may still take the tensor store out of it (AUTO, and the store does not fit); after that it is const, and the stages only read it.
struct JacobiPlan {
	bool dense, dense_sym, compact;
	int iter_slots;
};
static JacobiPlan jacobi_plan(const mpmc_ctx *c, int solver) {
	JacobiPlan jp;
	jp.dense = (solver == MPMC_SOLVER_DENSE) && !c->opts.polar_gs && !gs_ranked_on(c);
	jp.dense_sym = jp.dense && c->kept.tune.dense_symmetric;
	jp.compact = solver == MPMC_SOLVER_COMPACT;
	jp.iter_slots = (jp.dense && !jp.dense_sym) ? kDenseChunks : c->n_tiles;
	return jp;
}
struct EvalPlan {
	unsigned mask = 0;
	bool single = false;      // small LJ box: the whole evaluation is one launch, and nothing below is filled in
	bool static_ride = false; // stale position-independent terms ride along (an insertion / removal makes them stale every time)
	// streams and side work
	bool need_sf = false, need_intra = false, side_work = false;
	bool sf_part = false;     // the structure factors go through the per-tile partials of the factorised phases (d_sf_part)
	bool two_streams = false, side_fork = false, side_deferred = false;
	// pair pass
	bool pair_pass = false, sweep = false;
	FusedParams fp{};         // (c->last_fp is a copy of it)
	bool use_panels = false, panel_side = false; // the panel table is built in this evaluation / on the side stream
	bool reduce_in_tail = false;
	// dipole solve
	int solver = MPMC_SOLVER_MATRIX_FREE;
	bool compact = false;     // this evaluation fills and reads the tensor store
	bool solve = false, direct = false, gs = false;
	bool ranked = false;      // `polar_gs_ranked`: the sweeps behind the first run on the ranked view (stage_gauss_seidel_solve)
	int n_pol = 0, chol_np = 0; // direct solve: polarizable atoms, padded order of the factor
	JacobiPlan jp{};
	bool by_precision = false, moments = false, lazy = false;
	int want_rrms = 0, half = 0, last_it = 0, check_every = kCheckEvery;
	double allowed = 0.0;
	bool palmo = false;
	bool zodid = false;       // `polar_zodid`: the solve is the start vector (thole_iterative :3470); no stage between the static field and the energy runs
	int relax = RELAX_NONE;   // `polar_sor` / `polar_esor` in the iterative solves and under ewald_full (never read by the direct solve)
	bool pef = false;         // `polar_ewald_full`: the solve is stage_ewald_full_solve's (by_precision and allowed as for the iterative solves)
};

static inline size_t store_elements(const mpmc_ctx *c) { return (size_t)c->n_tile_pairs * (kTile * kTile); } // double2 elements, 16 B each
// how the dipole iteration runs (room for what it stores: reserve_solver_store)
static int choose_solver(const mpmc_ctx *c) {
	if (ewald_full_on(c)) return MPMC_SOLVER_MATRIX_FREE; // `polar_ewald_full` keeps a store of its own (stage_ewald_full_solve): the sweep stores nothing
	if (zodid_on(c)) return MPMC_SOLVER_MATRIX_FREE; // `polar_zodid`: no A matrix at all (System::polar :2548), nothing is stored
	if (direct_solve(c)) return MPMC_SOLVER_MATRIX_FREE; // no iteration: nothing is stored (the one contraction behind the solve, for the residual, is matrix-free)
	int want = c->opts.solver;
	if (c->opts.polar_gs || gs_ranked_on(c)) want = MPMC_SOLVER_MATRIX_FREE; // Gauss-Seidel sweeps rebuild the tensors row block by row block (kernels_gs.hip)
	if (want == MPMC_SOLVER_AUTO) {
		const size_t budget_mb = (size_t)c->kept.tune.tensor_budget_mb;
		want = (store_elements(c) * sizeof(double2) <= budget_mb * (size_t)1048576) ? MPMC_SOLVER_COMPACT : MPMC_SOLVER_MATRIX_FREE;
		// building the store costs about as much as three iterations save (0.10 ms against 0.03 ms per iteration at 10 000 atoms)
		if (c->opts.polar_precision == 0.0 && c->opts.polar_max_iter <= 3) want = MPMC_SOLVER_MATRIX_FREE;
	}
	return want;
}
// what follows from the solver (twice when AUTO has to give up the store: plan_evaluation, reserve_solver_store)
static void plan_solver(const mpmc_ctx *c, EvalPlan &p, int solver) {
	p.solver = solver;
	p.compact = (p.mask & RUN_SOLVE) && solver == MPMC_SOLVER_COMPACT;
	p.fp.do_thole = p.compact ? 1 : 0;
	// panels of the Jacobi contraction: two tile pairs of equal class behind one j-tile per workgroup (compact solver)
	p.use_panels = p.pair_pass && p.compact && c->kept.tune.use_panels && !c->kept.tune.no_classes && !c->kept.tune.no_uniform && c->n_tiles >= 3;
	// the table is needed by the first Jacobi launch only: it is made beside the pair sweep (side stream, joined after the sweep)
	p.panel_side = p.use_panels && p.two_streams;
	p.jp = jacobi_plan(c, solver);
	p.check_every = p.jp.dense ? 1 : kCheckEvery;
}

static EvalPlan plan_evaluation(const mpmc_ctx *c, unsigned mask, bool on_demand) {
	const mpmc_options &o = c->opts;
	const mpmc_tuning &t = c->kept.tune;
	EvalPlan p;
	p.mask = mask;
	p.static_ride = c->static_dirty;
	// small LJ box (BASELINE configs[1]): the whole evaluation is one launch -- pair sweep without classes, the block that finishes last
	// folds the partials into the pinned result vector; the LRC terms are the cached position-independent ones
	p.single = t.single_launch && mask == (RUN_PAIR | RUN_ATOMTERMS) && !o.feynman_hibbs && c->n_tiles <= kSingleLaunchTiles && !c->kept.prof && !p.static_ride;
	if (p.single) return p;

	// ---- reciprocal space + O(N) atom terms on the side stream, next to the pair sweep ------------------------------
	p.need_sf = (mask & RUN_RECIP) || ((mask & RUN_FIELD) && field_is_ewald(c));
	// intramolecular charge-to-screen term of coulombic_real: position dependent but independent of the pair sweep; identically zero
	// when every molecule is a single atom
	p.need_intra = (mask & RUN_PAIR) && (mask & RUN_PAIR_ES) && !(o.wolf && (mask & RUN_WOLF)) && (c->n_molecules != c->n);
	p.side_work = p.need_sf || p.need_intra;
	p.sf_part = p.need_sf && recip_view(c).lvec && o.ewald_kmax <= kRecipTabMaxK;
	// a fork/join costs ~20 us of dispatch latency: worth it next to reciprocal-space work, not for the O(N) atom terms alone -- and not
	// for small tables at all (kOneStreamMaxPairs).  Decided here, once per evaluation: nothing is forked at this point.
	// (round 4: ... and not when the caller keeps kOneStreamMinInflight or more evaluations in flight: other evaluations fill the device then,
	// and the fork and join are pure cost -- 1018-1025 against 1006-1012 evaluations/s with 32 beads, 1021 against 1002 with 8; one
	// evaluation at a time the fork is worth 1.5 %.  The choice of streams does not touch the arithmetic.)
	// Only for evaluations with a dipole solve: there the side work is 5 % of the evaluation; a 10 000-atom LJ + Ewald evaluation (sweep 95 us,
	// reciprocal space 25 us) loses 4 % in flight without the overlap (9365 against 9600-9960 evaluations/s).
	p.two_streams = (t.stream_mode == 1) ||
	                (t.stream_mode < 0 && c->n_tile_pairs > kOneStreamMaxPairs && !((mask & RUN_SOLVE) && c->inflight_hint >= kOneStreamMinInflight));
	p.side_fork = p.two_streams && (p.need_sf || p.need_intra);
	// (two streams: enqueued BEHIND the pair sweep -- the main stream's critical path (classes, sweep) reaches the device first; one
	// evaluation at a time the host used to be ~15 us late with the sweep because nine API calls of side work stood in front of it)
	p.side_deferred = p.side_work && p.side_fork && (mask & (RUN_PAIR | RUN_FIELD | RUN_STORE)) != 0 && t.side_after_sweep;

	// ---- pairwise pass: one symmetric sweep (energies + counts, static-field partials, Thole tensor store) ----------
	p.pair_pass = (mask & (RUN_PAIR | RUN_FIELD | RUN_STORE)) != 0;
	if (p.pair_pass) {
		FusedParams &fp = p.fp;
		fp.ewald_alpha = c->ewald_alpha;
		fp.polar_ewald_alpha = c->polar_ewald_alpha;
		fp.polar_damp = o.polar_damp;
		fp.rd_lrc = o.rd_lrc;
		fp.do_es = ((mask & RUN_PAIR_ES) || (mask & RUN_FIELD)) ? 1 : 0;
		// (`polar_wolf`: the field is k_wolf_field's, below; the sweep keeps its energies and the tensor store)
		fp.do_field = ((mask & RUN_FIELD) && !wolf_field_on(c)) ? (field_is_ewald(c) ? 1 : 2) : 0;
		ext_params(c, fp, (o.wolf && (mask & RUN_WOLF)) != 0);
		fp.thole_far_x = kTholeFarX;
		fp.pair_waves = t.pair_waves ? t.pair_waves : (c->n_tile_pairs <= kPairSplitMax ? 4 : 1);
		fp.store_only = ((mask & RUN_STORE) && !(mask & (RUN_PAIR | RUN_FIELD))) ? 1 : 0;
		fp.touch_n = fp.store_only ? c->touch_n : -1;
		for (int k = 0; k < 8; k++) fp.touch[k] = c->touch[k];
		// the fast sweep (kernels_pair.hip) where it applies -- Ewald electrostatics, alpha r_c inside its erfc table --
		// and, by default, where the table has more than kSweepMinPairs tile pairs (below that the 64 dependent steps of its one wave per
		// tile pair are a latency chain: four waves per tile pair in k_pair_fused); the tile pairs with a special atom, which it skips,
		// go through k_pair_fused on their list
		p.sweep = t.pair_kernel != 1 && c->d_sweep_blocks && (t.pair_kernel == 2 || c->n_tile_pairs > kSweepMinPairs) && pair_sweep_covers(c->box, fp, c->ewald_alpha);
	}
	// the scalar totals of the sweep are only read back at the very end.  Polarizable evaluations on two streams fold them in the launch
	// that closes the evaluation (second block of the polarization-energy kernel: launch_polar_energy_and_pairs) -- rounds 2-3 forked the
	// side stream for it, which put an event record in front of the static field and a join in front of the posted results (~10 us of
	// barrier packets on the main stream, one evaluation at a time)
	p.reduce_in_tail = (mask & RUN_PAIR) && (mask & RUN_SOLVE); // (on one stream too: one launch fewer)

	// ---- thole_iterative, reference src/System.Energy.cpp:3450-3543 ------------------------------------------------
	plan_solver(c, p, (mask & (RUN_FIELD | RUN_SOLVE | RUN_STORE)) ? choose_solver(c) : c->solver_used);
	p.solve = (mask & RUN_SOLVE) != 0;
	p.direct = p.solve && direct_solve(c);
	p.pef = p.solve && ewald_full_on(c);
	p.zodid = p.solve && zodid_on(c);
	p.relax = (p.solve && !p.direct && !p.zodid) ? c->kept.relax_scheme : RELAX_NONE;
	if (p.zodid) { // (nothing below applies: no iteration, no rrms, no moments, no Palmo-Krimm contraction)
	} else if (p.pef) { // (no rrms, no moments, never lazy: every entry runs all its passes)
		p.by_precision = (o.polar_precision != 0.0);
		p.allowed = p.by_precision ? o.polar_precision * o.polar_precision * kDebye2SKA * kDebye2SKA : 0.0;
	} else if (p.direct) {
		for (int i = 0; i < c->n; i++) p.n_pol += (c->h_alpha[i] != 0.0) ? 1 : 0;
		p.chol_np = chol_padded(p.n_pol);
	} else if (p.solve) {
		p.ranked = gs_ranked_on(c);
		p.gs = o.polar_gs != 0 || p.ranked;
		p.by_precision = (o.polar_precision != 0.0);
		p.want_rrms = (o.polar_rrms || o.polar_precision > 0) ? 1 : 0;
		p.allowed = p.by_precision ? o.polar_precision * o.polar_precision * kDebye2SKA * kDebye2SKA : 0.0;
		// fixed-count solves from alpha E0: the energy is the moment sum of the first `half` dipole differences, whether or not the other
		// iterations run now (on demand: they wait for somebody who reads the dipoles) -- alone or as a bead, an evaluation gives the same bits
		p.moments = polar_moments_apply(c);
		p.half = moments_half(o.polar_max_iter);
		p.lazy = p.moments && on_demand && t.dipoles_on_demand && p.half < o.polar_max_iter;
		p.last_it = p.lazy ? p.half : o.polar_max_iter;
		p.palmo = c->kept.palmo_enabled && p.gs; // (and the iteration must not have failed: stage_palmo)
	}
	return p;
}

// ---- room: every allocation, table upload and size guard of the evaluation, before anything of it is enqueued -----------------------------
// (a refusal here leaves nothing of the evaluation on the device, and no buffer is born after the side stream has been forked, where its
// first writer would not be ordered behind its fill -- see DevBuf::reserve)
// (COMPACT, DENSE) room for what the solver stores; AUTO falls back to recomputing the tensors when the store cannot be had
static int reserve_solver_store(mpmc_ctx *c, EvalPlan &p) {
	if (p.solver == MPMC_SOLVER_DENSE && !direct_solve(c)) { // the reference's layout, on request only: (3 n_pad)^2 doubles
		const int rc = c->d_adense.reserve(c, (size_t)3 * c->n_pad * (size_t)3 * c->n_pad);
		if (rc != MPMC_OK) return rc;
	}
	if (p.solver == MPMC_SOLVER_COMPACT) {
		const int rc = c->d_ab.reserve(c, store_elements(c));
		if (rc != MPMC_OK) {
			if (c->opts.solver == MPMC_SOLVER_COMPACT) return rc; // explicitly requested: report
			(void)hipGetLastError();
			plan_solver(c, p, MPMC_SOLVER_MATRIX_FREE); // AUTO: fall back to recomputing the tensors (still the HIP path)
		}
	}
	c->solver_used = p.solver;
	return MPMC_OK;
}
// the panel table's segments (its layout depends on the tile count only), the table and its per-entry slots
static int reserve_panels(mpmc_ctx *c) {
	int rc;
	if (c->seg_tiles != c->n_tiles) {
		std::vector<int> seg((size_t)c->n_tiles + 1, 0);
		for (int J = 0; J < c->n_tiles; J++) seg[J + 1] = seg[J] + panel_segment_entries(J);
		if ((rc = c->d_seg.reserve(c, seg.size())) != MPMC_OK) return rc;
		HIP_TRY(c, hipMemcpyAsync(c->d_seg, seg.data(), seg.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
		HIP_TRY(c, hipStreamSynchronize(c->stream)); // `seg` dies here
		c->n_panel_entries = seg[c->n_tiles];
		c->seg_tiles = c->n_tiles;
	}
	const size_t need = (size_t)c->n_panel_entries;
	if ((rc = c->d_panels.reserve(c, need)) != MPMC_OK) return rc;
	if ((rc = c->d_gpart.reserve(c, need * kTile * 3)) != MPMC_OK) return rc;
	if (c->kept.tune.trace_panel && (rc = c->d_trace.reserve(c, need * 4)) != MPMC_OK) return rc;
	return MPMC_OK;
}
// `polar_iterative off`: the factor must fit what the device has free (or the budget of the tuning switch); then the factor and its vectors
static int reserve_direct_solve(mpmc_ctx *c, const EvalPlan &p) {
	const int np = p.chol_np;
	const size_t elems = (size_t)np * (size_t)np, bytes = elems * sizeof(double);
	int rc;
	if ((rc = c->d_chol_status.reserve(c, 4)) != MPMC_OK) return rc;
	if ((rc = c->d_chol_info.reserve(c, 4)) != MPMC_OK) return rc;
	if ((rc = c->h_chol_info.reserve(c, 4)) != MPMC_OK) return rc;
	{ // size guard
		size_t free_b = 0, total_b = 0;
		HIP_TRY(c, hipMemGetInfo(&free_b, &total_b));
		size_t avail = free_b + c->d_chol.cap * sizeof(double);
		if (c->kept.tune.direct_budget_mb >= 0) avail = std::min(avail, (size_t)c->kept.tune.direct_budget_mb * (size_t)1048576);
		if (bytes > avail) {
			char buf[256];
			std::snprintf(buf, sizeof buf, "direct dipole solve: the factor of %d unknowns needs %.1f MB (%d x %d doubles), %.1f MB are available", 3 * p.n_pol,
			              (double)bytes / 1048576.0, np, np, (double)avail / 1048576.0);
			return fail(c, MPMC_ERR_MEMORY, buf);
		}
	}
	if (c->d_chol.reserve(c, elems) != MPMC_OK) {
		(void)hipGetLastError();
		return fail(c, MPMC_ERR_MEMORY, "direct dipole solve: cannot allocate the factor (" + std::to_string(bytes) + " bytes): " + c->err);
	}
	// (v0 = [0, np) and v1 = [np, 2 np); the one element more is a spare that no kernel addresses, kept so that the bytes held stay what they were)
	if ((rc = c->d_chol_v.reserve(c, (size_t)2 * np, (size_t)2 * np + 1)) != MPMC_OK) return rc;
	// (room for every slot of the context: the number of polarizable atoms changes with the atom list and can then never outgrow it)
	return c->d_chol_list.reserve(c, (size_t)p.n_pol, (size_t)c->max_pad);
}
// `polar_ewald_full`: the pair-factor store and the phase table must fit what the device has free; then the small tables
static int reserve_ewald_full(mpmc_ctx *c) {
	const size_t store = store_elements(c), phases = c->kept.tune.pef_phase_table ? (size_t)c->K * (size_t)c->max_pad : 0;
	const size_t grow = (store > c->d_pef_store.cap ? store * sizeof(double2) : 0) + (phases > c->d_pef_phases.cap ? phases * sizeof(double2) : 0);
	int rc;
	if (grow) { // size guard
		size_t free_b = 0, total_b = 0;
		HIP_TRY(c, hipMemGetInfo(&free_b, &total_b));
		const size_t avail = free_b + (store > c->d_pef_store.cap ? c->d_pef_store.cap * sizeof(double2) : 0) +
		                     (phases > c->d_pef_phases.cap ? c->d_pef_phases.cap * sizeof(double2) : 0);
		if (grow > avail) {
			char buf[256];
			std::snprintf(buf, sizeof buf, "polar_ewald_full: the pair-factor store of %d tile pairs and the phase table of %d k vectors need %.1f MB, %.1f MB are available",
			              c->n_tile_pairs, c->K, (double)grow / 1048576.0, (double)avail / 1048576.0);
			return fail(c, MPMC_ERR_MEMORY, buf);
		}
	}
	if (c->d_pef_store.reserve(c, store) != MPMC_OK || c->d_pef_phases.reserve(c, phases) != MPMC_OK) {
		(void)hipGetLastError();
		return fail(c, MPMC_ERR_MEMORY, "polar_ewald_full: cannot allocate the pair-factor store and the phase table (" + std::to_string(grow) + " bytes): " + c->err);
	}
	if ((rc = c->d_pef_cnt.reserve(c, (size_t)c->n_tile_pairs)) != MPMC_OK) return rc;
	if ((rc = c->d_pef_psum.reserve(c, 2 * (size_t)c->K + 4)) != MPMC_OK) return rc;
	if ((rc = c->d_pef_pairs.reserve(c, 1)) != MPMC_OK) return rc;
	return c->h_pef_pairs.reserve(c, 1);
}
// `polar_gs_ranked`: the rank pass's results and the second set of per-atom arrays and tile tables (grow-only, sized for the context's capacity)
static int reserve_ranked_view(mpmc_ctx *c) {
	const size_t np = (size_t)c->max_pad, mt = np / kTile, mtp = mt * (mt + 1) / 2;
	int rc;
	if ((rc = c->d_gr_info.reserve(c, 1)) != MPMC_OK) return rc;
	if ((rc = c->h_gr_info.reserve(c, 1)) != MPMC_OK) return rc;
	if ((rc = c->d_gr_rank.reserve(c, 2 * np)) != MPMC_OK) return rc;
	if ((rc = c->d_gr_atoms.reserve(c, np * kAtomRecordBytes)) != MPMC_OK) return rc;
	if ((rc = c->d_gr_vec.reserve(c, 15 * np)) != MPMC_OK) return rc;
	if ((rc = c->d_gr_blocks.reserve(c, gs_block_store_elements(c->n_tiles), gs_block_store_elements((int)mt))) != MPMC_OK) return rc;
	if ((rc = c->d_gr_bounds.reserve(c, 12 * mt)) != MPMC_OK) return rc;
	if ((rc = c->d_gr_cls.reserve(c, (size_t)c->n_tile_pairs, mtp)) != MPMC_OK) return rc;
	return c->d_gr_shift.reserve(c, (size_t)c->n_tile_pairs, mtp);
}
static int make_room(mpmc_ctx *c, EvalPlan &p) {
	int rc;
	if (p.mask & (RUN_FIELD | RUN_SOLVE | RUN_STORE)) {
		if ((rc = ensure_polar_buffers(c)) != MPMC_OK) return rc;
		if ((rc = reserve_solver_store(c, p)) != MPMC_OK) return rc;
	}
	if (p.sf_part && (rc = c->d_sf_part.reserve(c, (size_t)c->n_tiles * (size_t)c->K)) != MPMC_OK) return rc;
	if (p.use_panels && (rc = reserve_panels(c)) != MPMC_OK) return rc;
	if (p.direct && (rc = reserve_direct_solve(c, p)) != MPMC_OK) return rc;
	if (p.pef && (rc = reserve_ewald_full(c)) != MPMC_OK) return rc;
	// the in-tile blocks of the Gauss-Seidel sweeps
	if (p.gs && (rc = c->d_gs_blocks.reserve(c, gs_block_store_elements(c->n_tiles))) != MPMC_OK) return rc;
	if (p.ranked && (rc = reserve_ranked_view(c)) != MPMC_OK) return rc;
	return MPMC_OK;
}

// ---- launches written once ------------------------------------------------------------------------------------------------------------------
// One Jacobi iteration on the main stream: the contraction of the solver in use, then new_mu = alpha (E0 + F) into the other dipole
// vector.  Shared by the solve inside an evaluation and by finish_pending_dipoles, which runs the iterations an on-demand evaluation
// left undone: same kernels, same tables, same order.  dk (may be null): this iteration's slot of the ring of dipole differences.
static void enqueue_jacobi_iteration(mpmc_ctx *c, const AtomsDev &at, const JacobiPlan &jp, int it, int want_rrms, double allowed, int *ctl, int *host_flag,
                                     double *dk, const RelaxWeights *relax = nullptr /*`polar_sor` / `polar_esor`: this iteration's weights*/) {
	hipStream_t st = c->stream;
	const mpmc_options &o = c->opts;
	const int *converged = ctl ? ctl + 1 : nullptr;
	if (jp.dense) {
		ProfScope p(c, MPMC_K_DIPOLE_ITER);
		if (jp.dense_sym) launch_dense_symv(st, c->d_adense, c->n_pad, c->d_mu[c->mu_cur], c->d_tile_pairs, c->n_tile_pairs, c->d_part);
		else launch_dense_matvec(st, c->d_adense, c->n_pad, c->d_mu[c->mu_cur], kDenseChunks, c->d_part);
	} else if (jp.compact) {
		ProfScope p(c, MPMC_K_DIPOLE_ITER);
		if (c->panels_built) // every tile pair through the panel table: two per wave where classes allow
			launch_dipole_iter_panel(st, at, c->box, c->d_mu[c->mu_cur], c->d_tile_pairs, c->d_tp_shift, c->d_panels,
			                         c->n_panel_entries, c->d_ab, c->d_part, c->d_gpart, converged, c->d_trace);
		else
			launch_dipole_iter_hybrid(st, at, c->box, c->d_mu[c->mu_cur], c->d_tile_pairs, c->d_cls,
			                          shift_view(c), c->n_tile_pairs, c->d_ab, c->d_part, o.polar_damp,
			                          converged);
	} else { // matrix-free: the same symmetric tile-pair walk with nothing stored (null store => damped tensors rebuilt)
		ProfScope p(c, MPMC_K_DIPOLE_ITER);
		launch_dipole_iter_hybrid(st, at, c->box, c->d_mu[c->mu_cur], c->d_tile_pairs, c->d_cls,
		                          shift_view(c), c->n_tile_pairs, nullptr, c->d_part, o.polar_damp,
		                          converged);
	}
	{
		ProfScope p(c, MPMC_K_REDUCE);
		if (jp.compact && c->panels_built && !jp.dense)
			launch_dipole_update_panel(st, at, c->d_e_static, c->d_part, c->d_gpart, c->d_seg, c->d_mu[c->mu_cur], c->d_mu[1 - c->mu_cur],
			                           c->d_e_induced, want_rrms, c->d_rrms, allowed, ctl, host_flag, it, dk, relax);
		else
			launch_dipole_update(st, at, c->d_e_static, c->d_part, jp.iter_slots, c->d_mu[c->mu_cur], c->d_mu[1 - c->mu_cur], c->d_e_induced,
			                     want_rrms, c->d_rrms, allowed, ctl, host_flag, it, dk, relax);
	}
	c->mu_cur = 1 - c->mu_cur;
}

// The iterations an on-demand evaluation left undone, from mu_half on: dipoles, induced field and iteration count come out as an eager
// evaluation leaves them.  Enqueued behind whatever the stream still carries and waited for.
int mpmc::finish_pending_dipoles(mpmc_ctx *c) {
	if (c->polar_pending == mpmc_ctx::PEND_NONE) return MPMC_OK;
	if (c->polar_pending == mpmc_ctx::PEND_DROPPED)
		return fail(c, MPMC_ERR_ARG, "the dipoles of the last evaluation were left to be computed on demand, and its positions, cell, options or buffers "
		                             "have been overwritten since: evaluate again (or mpmc_set_dipoles_on_demand(ctx, 0))");
	HIP_TRY(c, hipSetDevice(c->device));
	const AtomsDev at = atoms_view(c);
	const JacobiPlan jp = jacobi_plan(c, c->solver_used);
	for (int it = c->pend_done + 1; it <= c->pend_target; it++) enqueue_jacobi_iteration(c, at, jp, it, 0, 0.0, nullptr, nullptr, nullptr);
	HIP_TRY(c, hipGetLastError());
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	c->polar_pending = mpmc_ctx::PEND_NONE;
	c->pend_done = c->pend_target;
	if (!c->pending) prof_harvest(c);
	return MPMC_OK;
}

// The pair pass on the main stream: the fast sweep with k_pair_fused on its list of generic tile pairs, or k_pair_fused on the whole table
// (c->last_pair_was_sweep says which).  Shared by the evaluation and by mpmc_debug_time_pair, which replays it.
static void launch_pair_pass(mpmc_ctx *c, const AtomsDev &at, const FusedParams &fp, bool compact, int lds_pad, int replicas) {
	hipStream_t st = c->stream;
	if (c->last_pair_was_sweep) {
		launch_pair_sweep(st, at, c->box, fp, c->n_molecules != c->n, c->d_sweep_blocks, c->n_sweep_blocks, c->d_cls,
		                  shift_view(c), c->d_erf_tab, c->d_block_part, c->d_block_cnt, c->d_part,
		                  compact ? c->d_ab : nullptr, sweep_split_mode(c), sweep_split_tail(c), c->kept.tune.fast_geometry, lds_pad, replicas);
		if (c->n_generic > 0)
			launch_pair_fused(st, at, c->box, fp, c->d_tile_pairs, c->d_cls, c->n_generic, c->d_block_part, c->d_block_cnt, c->d_part,
			                  compact ? c->d_ab : nullptr, c->d_generic_list);
	} else if (!(fp.store_only && !compact)) // (a store-only pass without a store to fill has nothing to do beyond the classes)
		launch_pair_fused(st, at, c->box, fp, c->d_tile_pairs, c->d_cls, c->n_tile_pairs, c->d_block_part, c->d_block_cnt, c->d_part,
		                  compact ? c->d_ab : nullptr);
}

// F = -(A_off mu) of the dipoles `mu` into `field`: one matrix-free Jacobi contraction (nothing stored), its slots summed by the update
// kernel, whose new dipoles go to `spare` and are dropped (rrms untouched); `tail` launches what the caller reads the field with.  The sum
// and the tail share one MPMC_K_REDUCE bracket; the contraction is inside it too, or in a MPMC_K_DIPOLE_ITER bracket of its own.
template <class Tail>
static void contract_into_field(mpmc_ctx *c, const AtomsDev &at, double *mu, double *spare, double *field, bool own_bracket, Tail &&tail) {
	hipStream_t st = c->stream;
	int cur;
	prof_begin(c, own_bracket ? MPMC_K_DIPOLE_ITER : MPMC_K_REDUCE, cur, st);
	launch_dipole_iter_hybrid(st, at, c->box, mu, c->d_tile_pairs, c->d_cls, shift_view(c), c->n_tile_pairs, nullptr, c->d_part, c->opts.polar_damp, nullptr);
	if (own_bracket) {
		prof_end(c, cur, st);
		prof_begin(c, MPMC_K_REDUCE, cur, st);
	}
	launch_dipole_update(st, at, c->d_e_static, c->d_part, c->n_tiles, mu, spare, field, 0, c->d_rrms, 0.0, nullptr, nullptr, 1);
	tail();
	prof_end(c, cur, st);
}

// reciprocal space and the O(N) intramolecular term, on the stream they are given
static void enqueue_side_work(mpmc_ctx *c, const EvalPlan &p, const AtomsDev &at, const RecipDev &rcp, hipStream_t s2) {
	const mpmc_options &o = c->opts;
	if (p.need_intra) {
		ProfScope ps(c, MPMC_K_PAIR, s2);
		launch_intra_terms(s2, at, c->d_slot_of, c->ewald_alpha, c->d_scal);
	}
	{
		ProfScope ps(c, MPMC_K_RECIP, s2);
		if (p.need_sf) launch_recip_sf(s2, at, c->box, rcp, o.ewald_kmax, c->d_sf_part);
		if (p.mask & RUN_RECIP) launch_recip_energy(s2, rcp, c->box, c->d_scal); // (the LRC and self terms are cached: prepare())
	}
	if ((p.mask & RUN_FIELD) && field_is_ewald(c)) {
		ProfScope ps(c, MPMC_K_FIELD, s2);
		launch_field_recip(s2, at, c->box, rcp, o.ewald_kmax, c->d_e_recip_part);
	}
}

// ---- the stages of one evaluation, in the order enqueue() runs them: each looks at the plan for whether it has anything to do, and none
// returns anything but a HIP error (everything that can be refused was refused by make_room) ---------------------------------------------
static int stage_single_launch(mpmc_ctx *c, const EvalPlan &, const AtomsDev &at, const RecipDev &) {
	FusedParams fp{};
	fp.rd_lrc = c->opts.rd_lrc;
	c->single_seq += 1.0;
	launch_pair_lj_single(c->stream, at, c->box, fp, c->d_tile_pairs, c->n_tile_pairs, c->d_block_part, c->d_block_cnt, c->d_counter, c->h_scal,
	                      c->single_seq);
	HIP_TRY(c, hipGetLastError());
	c->last_was_single = true;
	c->pending = true;
	return MPMC_OK;
}

static int stage_clear_and_static_terms(mpmc_ctx *c, const EvalPlan &p, const AtomsDev &at, const RecipDev &) {
	hipStream_t st = c->stream;
	// the scalar block: zeroed by the post kernel of the evaluation before this one; cleared here only when something else used it since
	// (the static-terms pass, an upload of the atoms, an evaluation that failed half way)
	if (!c->scal_clean) HIP_TRY(c, hipMemsetAsync(c->d_scal, 0, (S_COUNT + C_COUNT) * sizeof(double), st));
	c->scal_clean = false;
	if (p.static_ride) { // first thing on the main stream: its slots are nobody else's (S_LRC_PAIR, S_LRC_SELF, S_ES_SELF)
		launch_atom_terms(st, at, lrc_box(c), c->ewald_alpha, c->opts.rd_lrc, /*self term*/ 1, c->d_atom_part, c->d_scal);
		HIP_TRY(c, hipGetLastError());
		c->static_ride_gen = c->static_gen;
	}
	return MPMC_OK;
}

static int stage_side_work(mpmc_ctx *c, const EvalPlan &p, const AtomsDev &at, const RecipDev &rcp) {
	c->two_streams = p.two_streams; // (fork_side takes it back when the side stream cannot be had)
	if (p.side_work && !p.side_deferred) enqueue_side_work(c, p, at, rcp, p.side_fork ? fork_side(c) : c->stream);
	return MPMC_OK;
}

// classes, panel table, pair launch, the side work that was left for behind it, join
static int stage_pair_pass(mpmc_ctx *c, const EvalPlan &p, const AtomsDev &at, const RecipDev &rcp) {
	hipStream_t st = c->stream;
	const mpmc_options &o = c->opts;
	if (p.pair_pass) {
		// tile-pair classes from this configuration's tile bounding boxes
		{
			ProfScope pc(c, MPMC_K_CLASSES);
			if (c->kept.tune.no_classes) HIP_TRY(c, hipMemsetAsync(c->d_cls, 0, (size_t)c->n_tile_pairs * sizeof(int), st));
			else launch_tile_classes(st, at, c->box, c->d_tile_pairs, c->n_tile_pairs, (o.polarization && !o.rd_only) ? o.polar_damp : 0.0,
			                         c->d_tile_bounds, c->d_cls, c->kept.tune.no_uniform ? nullptr : c->d_tp_shift, c->sort_origin_f, kTholeFarX);
		}
		if (!p.fp.store_only && p.compact) c->store_dirty_tiles.clear(); // a full sweep rebuilds every stored tile pair
		c->panels_built = false;
		if (p.use_panels) {
			if (!p.panel_side) {
				ProfScope pc(c, MPMC_K_CLASSES, st);
				launch_build_panels(st, c->d_cls, c->n_tiles, c->d_seg, c->d_panels);
			}
			c->panels_built = true;
		}
		// the side stream starts behind the classes (what it reads of the main stream's work: positions, classes); its kernels are
		// enqueued after the sweep's launch call
		hipStream_t s_side = (p.side_deferred || p.panel_side) ? fork_side(c) : st;
		c->last_fp = p.fp;
		c->last_fp_valid = !p.fp.store_only;
		ProfScope pp(c, MPMC_K_PAIR);
		c->last_pair_was_sweep = p.sweep;
		launch_pair_pass(c, at, p.fp, p.compact, (p.side_deferred || p.panel_side) ? c->kept.tune.sweep_lds_pad : 0, 1);
		if (p.side_deferred) enqueue_side_work(c, p, at, rcp, s_side);
		if (p.panel_side) {
			ProfScope pc(c, MPMC_K_CLASSES, s_side);
			launch_build_panels(s_side, c->d_cls, c->n_tiles, c->d_seg, c->d_panels);
		}
	}
	if ((p.side_work && p.side_fork) || p.panel_side) join_side(c);
	return MPMC_OK;
}

static int stage_pair_reduce(mpmc_ctx *c, const EvalPlan &p, const AtomsDev &, const RecipDev &) {
	if ((p.mask & RUN_PAIR) && !p.reduce_in_tail) {
		ProfScope ps(c, MPMC_K_REDUCE);
		launch_reduce_pairs(c->stream, c->d_block_part, c->d_block_cnt, c->n_tile_pairs, c->d_scal, c->d_cnt);
	}
	return MPMC_OK;
}

static int stage_static_field(mpmc_ctx *c, const EvalPlan &p, const AtomsDev &at, const RecipDev &) {
	if (!(p.mask & RUN_FIELD)) return MPMC_OK;
	hipStream_t st = c->stream;
	ProfScope ps(c, MPMC_K_FIELD);
	c->mu_cur = 0;
	if (wolf_field_on(c)) // thole_field_wolf (:3337-3396) into the real-space slots, behind the classes of the pairwise pass
		launch_wolf_field(st, at, c->box, wolf_field_params(c->kept.pw_alpha, c->box.cutoff), c->d_tile_pairs, c->d_cls, c->n_tile_pairs, c->d_part);
	// (`polar_ewald_full`: mu_0 = alpha E0 without polar_gamma, init_dipoles_ewald :2944-2956; nor under `polar_sor` / `polar_esor`, :3555)
	launch_field_finalize(st, at, c->box, field_is_ewald(c) ? 1 : 0, c->d_e_recip_part, c->d_part, c->n_tiles, start_gamma(c), c->d_e_static,
	                      c->d_mu[0], c->d_e_real, polar_moments_apply(c) ? c->d_dk_ring.p : nullptr);
	c->e_real_valid = (p.mask == full_mask(c)); // (with the accepted positions resident: what trial moves update incrementally)
	return MPMC_OK;
}

// `polar_iterative off` (System::polar :2590-2607; thole_bmatrix + thole_bmatrix_dipoles :2596-2600): A mu = E0 solved directly
// (kernels_chol.hip), behind the static field.  Leaves the dipoles in d_mu[mu_cur], mu / alpha - E0 in d_e_induced and { status, max |r|,
// max |E0| } on their way to the pinned info block.
static int stage_direct_solve(mpmc_ctx *c, const EvalPlan &p, const AtomsDev &at, const RecipDev &) {
	if (!p.direct) return MPMC_OK;
	hipStream_t st = c->stream;
	const int n_pol = p.n_pol, np = p.chol_np;
	c->mu_cur = 0;
	double *mu = c->d_mu[0], *v0 = c->d_chol_v, *v1 = c->d_chol_v + np;
	HIP_TRY(c, hipMemsetAsync(c->d_chol_status, 0, sizeof(int), st));
	HIP_TRY(c, hipMemsetAsync(mu, 0, 3 * (size_t)at.n_pad * sizeof(double), st));
	if (n_pol > 0) {
		{
			ProfScope ps(c, MPMC_K_TENSOR);
			launch_chol_build(st, at, c->box, c->opts.polar_damp, c->d_chol_list, n_pol, np, c->d_chol);
		}
		{
			ProfScope ps(c, MPMC_K_DIPOLE_ITER);
			launch_chol_rhs(st, c->d_chol_list, n_pol, np, c->d_e_static, v0, c->d_chol_status);
			launch_chol_factor(st, c->d_chol, np, c->d_chol_status);
			launch_chol_solve(st, c->d_chol, np, v0, v1, c->d_chol_status);
			launch_chol_scatter(st, c->d_chol_list, n_pol, v0, mu, c->d_chol_status);
		}
	}
	// the residual from an independent product: one matrix-free contraction, -(A_off mu) into d_e_induced (d_mu[1] is scratch)
	contract_into_field(c, at, mu, c->d_mu[1], c->d_e_induced, false,
	                    [&] { launch_chol_finish(st, at, mu, c->d_e_static, c->d_e_induced, c->d_chol_status, c->d_chol_info); });
	HIP_TRY(c, hipGetLastError());
	HIP_TRY(c, hipMemcpyAsync(c->h_chol_info, c->d_chol_info, 3 * sizeof(double), hipMemcpyDeviceToHost, st));
	c->direct.n_unknowns = 3 * (int64_t)n_pol;
	c->direct.factor_bytes = (int64_t)(c->d_chol.cap * sizeof(double));
	c->direct_ran = true;
	c->polar_pending = mpmc_ctx::PEND_NONE;
	return MPMC_OK;
}

// what an iterative solve leaves behind after `it` iterations
static void close_solve(mpmc_ctx *c, const EvalPlan &p, int it) {
	const int ran = c->failed ? it - 1 : it; // (a failed solve stops in front of its 128th contraction)
	c->relax_info.acted = (p.relax != RELAX_NONE && ran > 0) ? 1 : 0;
	c->relax_info.contractions = ran;
	c->relax_info.last_weight = relax_weights(p.relax, c->opts.polar_gamma, ran).w_new;
	c->relax_info.store_filled = (p.compact || p.jp.dense) ? 1 : 0;
	c->iters = p.lazy ? c->opts.polar_max_iter : it; // (what the solve comes to once its dipoles are asked for)
	c->polar_pending = p.lazy ? mpmc_ctx::PEND_OPEN : mpmc_ctx::PEND_NONE;
	c->pend_done = it, c->pend_target = c->opts.polar_max_iter;
}

// What one Gauss-Seidel sweep reads and writes: the context's own arrays (atom order), or the ranked view of `polar_gs_ranked`
struct SweepView {
	AtomsDev at;
	double *e_static, *mu[2], *e_induced, *rrms;
	const int *cls;
	const double4 *shift;
	const double2 *blocks;
};
// `polar_gs_ranked`, between the first sweep and the second (update_ranking :3631-3656 behind an iteration that is followed by another): the
// view in sweep order -- atoms, E0 and the current dipoles gathered, then everything that is derived from the order of the atoms: tile
// bounding boxes, tile-pair classes and common images, the in-tile blocks
static SweepView build_ranked_view(mpmc_ctx *c, const SweepView &id) {
	hipStream_t st = c->stream;
	const mpmc_options &o = c->opts;
	const size_t np = (size_t)c->max_pad;
	const int *order = c->d_gr_rank + np;
	GsRankView g;
	int32_t *unused_perm, *unused_slot;
	atom_block_layout(c->d_gr_atoms, np, [&](double4 *xyzq, double2 *lj, int2 *mf, double *al, double *ep, double *imm, int32_t *perm, int32_t *slot) {
		g.xyzq = xyzq, g.lj = lj, g.mf = mf, g.alpha = al, g.eps = ep, g.inv_molmass = imm, unused_perm = perm, unused_slot = slot;
	});
	(void)unused_perm, (void)unused_slot;
	double *vec = c->d_gr_vec;
	SweepView v;
	v.e_static = g.e_static = vec;
	v.mu[0] = vec + 3 * np, v.mu[1] = vec + 6 * np;
	v.e_induced = vec + 9 * np;
	v.rrms = vec + 12 * np;
	g.mu = v.mu[c->mu_cur];
	v.at = id.at;
	v.at.xyzq = g.xyzq, v.at.lj = g.lj, v.at.mf = g.mf, v.at.alpha = g.alpha, v.at.eps = g.eps, v.at.inv_molmass = g.inv_molmass;
	{
		ProfScope ps(c, MPMC_K_CLASSES);
		launch_gs_rank_gather(st, order, id.at, g, id.e_static, id.mu[c->mu_cur]);
		if (c->kept.tune.no_classes) (void)hipMemsetAsync(c->d_gr_cls, 0, (size_t)c->n_tile_pairs * sizeof(int), st);
		else launch_tile_classes(st, v.at, c->box, c->d_tile_pairs, c->n_tile_pairs, o.polar_damp, c->d_gr_bounds, c->d_gr_cls,
		                         c->kept.tune.no_uniform ? nullptr : c->d_gr_shift.p, c->sort_origin_f, kTholeFarX);
	}
	v.cls = c->d_gr_cls;
	v.shift = (c->kept.tune.no_uniform || c->kept.tune.no_classes) ? nullptr : c->d_gr_shift.p;
	{
		ProfScope ps(c, MPMC_K_TENSOR);
		launch_gs_blocks(st, v.at, c->box, o.polar_damp, c->d_gr_blocks);
	}
	v.blocks = c->d_gr_blocks;
	return v;
}

// Gauss-Seidel sweeps: in place, in atom order (`polar_gs_ranked`: in ranked order behind the first); the host asks for the verdict of a
// precision-terminated solve after every sweep
static int stage_gauss_seidel_solve(mpmc_ctx *c, const EvalPlan &p, const AtomsDev &at, const RecipDev &) {
	if (!p.solve || p.direct || p.pef || p.zodid || !p.gs) return MPMC_OK;
	hipStream_t st = c->stream;
	const mpmc_options &o = c->opts;
	{ // the in-tile blocks of the sweeps: positions and polarizabilities only, once per evaluation
		ProfScope ps(c, MPMC_K_TENSOR);
		launch_gs_blocks(st, at, c->box, o.polar_damp, c->d_gs_blocks);
	}
	SweepView v{at, c->d_e_static, {c->d_mu[0], c->d_mu[1]}, c->d_e_induced, c->d_rrms, c->d_cls, shift_view(c), c->d_gs_blocks};
	const SweepView identity = v;
	const int *order = nullptr;
	if (p.ranked) { // System::pairs :1001-1029, on every evaluation: the positions changed
		ProfScope ps(c, MPMC_K_CLASSES);
		launch_gs_rank(st, at, c->box, c->d_tile_pairs, c->n_tile_pairs, c->d_gr_info, c->d_gr_rank, c->d_gr_rank + c->max_pad);
		HIP_TRY(c, hipMemcpyAsync(c->h_gr_info, c->d_gr_info, sizeof(GsRankInfoDev), hipMemcpyDeviceToHost, st));
		c->gr_ran = true;
		c->gr_pos_gen = c->pos_gen, c->gr_static_gen = c->static_gen;
		c->gr_info.acted = 1;
	}
	int it = 0;
	for (bool keep = true; keep;) {
		it++;
		if (it >= kMaxIterationCount && p.by_precision) { // divergence: mu = alpha E0, iterator_failed (:3483-3494)
			launch_dipole_reset(st, v.at, v.e_static, v.mu[c->mu_cur]);
			c->failed = 1;
			break;
		}
		if (p.ranked && it == 2) { // the first sweep is followed by another: from here on the sweeps run on the ranked view
			v = build_ranked_view(c, identity);
			order = c->d_gr_rank + c->max_pad;
		}
		if (p.by_precision) HIP_TRY(c, hipMemsetAsync(c->d_flag, 0, sizeof(int), st));
		// in-place sweep in atom order; old_mu is kept only when rrms / precision or a relaxation scheme need it (:3503-3507)
		double *mu = v.mu[c->mu_cur], *mu_old = v.mu[1 - c->mu_cur];
		if (p.want_rrms || p.relax) HIP_TRY(c, hipMemcpyAsync(mu_old, mu, 3 * (size_t)at.n_pad * sizeof(double), hipMemcpyDeviceToDevice, st));
		{
			ProfScope ps(c, MPMC_K_DIPOLE_ITER);
			launch_gs_sweep(st, v.at, c->box, o.polar_damp, v.e_static, mu, v.e_induced, c->d_part, c->d_tile_pairs, v.cls, v.shift, c->n_tile_pairs, c->d_gs_ul,
			                c->d_gs_ul + 3 * (size_t)c->max_pad, v.blocks);
		}
		if (order) c->gr_info.ranked_sweeps++;
		if (p.want_rrms) {
			ProfScope ps(c, MPMC_K_REDUCE);
			launch_gs_finish(st, v.at, mu_old, mu, p.want_rrms, v.rrms, p.allowed, c->d_flag);
		}
		if (p.relax) { // :3526-3536, behind rrms and the verdict, which saw the swept values: the blend goes where old_mu was and becomes the
			// current vector; the swept one stays in the other buffer, where stage_palmo finds it
			ProfScope ps(c, MPMC_K_REDUCE);
			launch_gs_blend(st, v.at, mu, mu_old, mu_old, relax_weights(p.relax, o.polar_gamma, it));
			c->mu_cur = 1 - c->mu_cur;
		}
		if (p.by_precision) {
			HIP_TRY(c, hipMemcpyAsync(c->h_flag, c->d_flag, sizeof(int), hipMemcpyDeviceToHost, st));
			HIP_TRY(c, hipStreamSynchronize(st));
			keep = (*c->h_flag != 0);
		} else {
			keep = (it != o.polar_max_iter);
		}
	}
	if (order) { // back to atom order: the dipoles (under a relaxation scheme the swept vector too: stage_palmo contracts it), the induced field of
		// the last sweep and the per-atom rrms; the energy, rrms and Palmo-Krimm stages then run on the context's own arrays as under polar_gs
		ProfScope ps(c, MPMC_K_CLASSES);
		GsRankScatter sc{};
		sc.src3[0] = v.mu[c->mu_cur], sc.dst3[0] = c->d_mu[c->mu_cur];
		if (p.relax) sc.src3[1] = v.mu[1 - c->mu_cur], sc.dst3[1] = c->d_mu[1 - c->mu_cur];
		sc.src3[2] = v.e_induced, sc.dst3[2] = c->d_e_induced;
		if (p.want_rrms) sc.src1 = v.rrms, sc.dst1 = c->d_rrms;
		launch_gs_rank_scatter(st, order, at.n_pad, sc);
	}
	close_solve(c, p, it);
	return MPMC_OK;
}

static int stage_jacobi_solve(mpmc_ctx *c, const EvalPlan &p, const AtomsDev &at, const RecipDev &) {
	if (!p.solve || p.direct || p.pef || p.zodid || p.gs) return MPMC_OK;
	hipStream_t st = c->stream;
	const mpmc_options &o = c->opts;
	const size_t dk_stride = 3 * (size_t)at.n_pad;
	if (p.jp.dense) { // thole_amatrix into device memory, once per evaluation (the positions changed)
		ProfScope ps(c, MPMC_K_TENSOR);
		launch_dense_build(st, at, c->box, o.polar_damp, c->d_adense, p.jp.dense_sym);
	}
	// Precision-terminated Jacobi solves: are_we_done_yet (:3215-3239) runs on the device (ctl = {broke, converged-at, ticket}); the host
	// enqueues kCheckEvery iterations at a time and reads the verdict once per batch -- the iterations enqueued behind the one that
	// converged return at once and leave the dipoles alone.  (Gauss-Seidel sweeps and the dense solver still ask after every iteration.)
	int *ctl = p.by_precision ? c->d_flag + 1 : nullptr;
	const int mu_start = c->mu_cur;
	int done_at = 0;
	int *host_flag = ctl ? c->h_flag + 2 : nullptr; // pinned {last closed iteration, converged-at} the closing update block posts
	if (ctl) {
		HIP_TRY(c, hipMemsetAsync(ctl, 0, 3 * sizeof(int), st));
		c->h_flag[2] = c->h_flag[3] = 0; // (nothing of an earlier solve can still be in flight: every evaluation is waited for)
	}
	int it = 0;
	for (bool keep = true; keep;) {
		it++;
		if (it >= kMaxIterationCount && p.by_precision) { // divergence: mu = alpha E0, iterator_failed (:3483-3494)
			launch_dipole_reset(st, at, c->d_e_static, c->d_mu[c->mu_cur]);
			c->failed = 1;
			break;
		}
		const RelaxWeights rw = relax_weights(p.relax, o.polar_gamma, it); // (every launch of a batch carries its own: they depend on `it` alone)
		enqueue_jacobi_iteration(c, at, p.jp, it, p.want_rrms, p.allowed, ctl, host_flag, (p.moments && it <= p.half) ? c->d_dk_ring + (size_t)it * dk_stride : nullptr,
		                         p.relax ? &rw : nullptr);
		if (p.by_precision) {
			if (it % p.check_every == 0 || it + 1 >= kMaxIterationCount) { // the verdict of this batch
				HIP_TRY(c, hipGetLastError());
				// spin on the pinned flag until iteration `it` is closed (or an earlier one converged); a stream synchronisation costs
				// ~15 us, this ~2.  Past a generous budget fall back to the blocking read (correct either way).
				volatile const int *hf = host_flag;
				const bool seen = poll_posted(c, [&] { return hf[0] >= it || hf[1] != 0; }, std::chrono::microseconds(50000));
				if (seen) {
					done_at = hf[1];
				} else {
					c->kept.n_stream_syncs++;
					HIP_TRY(c, hipMemcpyAsync(c->h_flag, ctl + 1, sizeof(int), hipMemcpyDeviceToHost, st));
					HIP_TRY(c, hipStreamSynchronize(st));
					done_at = *c->h_flag;
				}
				keep = (done_at == 0);
			}
		} else {
			keep = (it != p.last_it);
		}
	}
	if (done_at > 0) { // the iterations enqueued behind the converged one did nothing: the result is where iteration done_at left it
		it = done_at;
		c->mu_cur = (mu_start + done_at) & 1;
	}
	close_solve(c, p, it);
	return MPMC_OK;
}

// `polar_ewald_full` (System::ewald_full :2785-2830), behind the static field: the pair-factor store and the phases once, then per pass the
// real-space contraction, the dipole structure factors and the update.  A precision-terminated solve asks for the verdict after every
// pass, as the Gauss-Seidel sweeps do.  Leaves the dipoles after the last update in d_mu[mu_cur] and the last pass's field in d_e_induced.
static int stage_ewald_full_solve(mpmc_ctx *c, const EvalPlan &p, const AtomsDev &at, const RecipDev &rcp) {
	if (!p.pef) return MPMC_OK;
	hipStream_t st = c->stream;
	const mpmc_options &o = c->opts;
	const double a = c->polar_ewald_alpha;
	EwaldFullParams ep;
	ep.vector_weight = (c->kept.pef_flags & MPMC_PEF_VECTOR_KWEIGHT) ? 1 : 0;
	ep.recip_scale = 8.0 * kPi / c->box.volume;
	ep.c_total = -4.0 * kPi / (3.0 * c->box.volume);
	ep.c_self = 4.0 * a * a * a / (3.0 * std::sqrt(kPi));
	ep.allowed_sqerr = p.allowed;
	double2 *phases = c->kept.tune.pef_phase_table ? c->d_pef_phases.p : nullptr;
	{
		ProfScope ps(c, MPMC_K_TENSOR);
		launch_pef_fill(st, at, c->box, a, o.polar_damp, c->d_tile_pairs, p.pair_pass ? c->d_cls.p : nullptr /*made by this evaluation's pair pass*/, c->n_tile_pairs,
		                c->d_pef_store, c->d_pef_cnt, c->d_pef_pairs);
		if (phases) launch_pef_phases(st, at, rcp.kvec, c->K, phases);
	}
	HIP_TRY(c, hipMemcpyAsync(c->h_pef_pairs, c->d_pef_pairs, sizeof(long long), hipMemcpyDeviceToHost, st));
	int passes = 0;
	for (bool keep = true; keep;) {
		if (passes >= kMaxIterationCount && p.by_precision) { // :2802-2805: the dipoles stay as they are
			c->failed = 1;
			break;
		}
		if (p.by_precision) HIP_TRY(c, hipMemsetAsync(c->d_flag, 0, sizeof(int), st));
		{
			ProfScope ps(c, MPMC_K_DIPOLE_ITER);
			launch_pef_contract(st, at, c->box, c->d_mu[c->mu_cur], c->d_tile_pairs, c->n_tile_pairs, c->d_pef_cnt, c->d_pef_store, c->d_part);
			launch_pef_sf(st, at, rcp.kvec, c->K, phases, c->d_mu[c->mu_cur], c->d_pef_psum);
		}
		{
			ProfScope ps(c, MPMC_K_REDUCE);
			const RelaxWeights rw = relax_weights(p.relax, o.polar_gamma, passes + 1); // (the 0-based counter + 1, :3196-3204)
			launch_pef_finish(st, at, ep, c->d_e_static, c->d_part, c->n_tiles, phases, rcp.kvec, rcp.kw, c->K, c->d_pef_psum, c->d_mu[c->mu_cur],
			                  c->d_mu[1 - c->mu_cur], c->d_e_induced, p.by_precision ? c->d_flag.p : nullptr, p.relax ? &rw : nullptr);
		}
		c->mu_cur = 1 - c->mu_cur;
		if (p.by_precision) { // are_we_done_yet :3227-3236
			HIP_TRY(c, hipMemcpyAsync(c->h_flag, c->d_flag, sizeof(int), hipMemcpyDeviceToHost, st));
			HIP_TRY(c, hipStreamSynchronize(st));
			keep = (*c->h_flag != 0);
		} else {
			keep = (passes != o.polar_max_iter); // :3222-3225: the 0-based counter against polar_max_iter
		}
		passes++;
	}
	HIP_TRY(c, hipGetLastError());
	c->iters = 0; // (the reference never writes polarization_iterations on this path)
	c->polar_pending = mpmc_ctx::PEND_NONE;
	c->pef_ran = true;
	c->pef_info.passes = passes;
	c->pef_info.n_k = c->K;
	c->pef_info.store_bytes = (int64_t)(c->d_pef_store.cap * sizeof(double2));
	c->relax_info.acted = (p.relax != RELAX_NONE && passes > 0) ? 1 : 0;
	c->relax_info.contractions = passes;
	c->relax_info.last_weight = relax_weights(p.relax, o.polar_gamma, passes).w_new;
	c->relax_info.store_filled = 1;
	return MPMC_OK;
}

// -1/2 mu . E0 (or the moment sum of a fixed-count Jacobi solve) into the scalar block; with the pair totals as the launch's second block
// when this is the tail of the evaluation (plan: reduce_in_tail).  The one place that picks among the four kernels.
static int stage_polar_energy(mpmc_ctx *c, const EvalPlan &p, const AtomsDev &at, const RecipDev &) {
	if (!p.solve) return MPMC_OK;
	hipStream_t st = c->stream;
	if (p.zodid) { // mu = mu_0, which the static field's finalize (or the trial move's) has just written; no induced field (:3470)
		c->mu_cur = 0;
		HIP_TRY(c, hipMemsetAsync(c->d_e_induced, 0, 3 * (size_t)at.n_pad * sizeof(double), st));
		c->polar_pending = mpmc_ctx::PEND_NONE;
		c->relax_info.acted = 1;
	}
	const double *mu = c->d_mu[c->mu_cur], *rrms = p.want_rrms ? c->d_rrms.p : nullptr;
	ProfScope ps(c, MPMC_K_REDUCE);
	if (p.moments && p.reduce_in_tail)
		launch_polar_moments_and_pairs(st, at, c->d_dk_ring, c->d_e_static, c->opts.polar_max_iter, c->d_block_part, c->d_block_cnt, c->n_tile_pairs, c->d_scal,
		                               c->d_cnt);
	else if (p.moments) launch_polar_moments(st, at, c->d_dk_ring, c->d_e_static, c->opts.polar_max_iter, c->d_scal);
	else if (p.reduce_in_tail)
		launch_polar_energy_and_pairs(st, at, mu, c->d_e_static, rrms, c->d_block_part, c->d_block_cnt, c->n_tile_pairs, c->d_scal, c->d_cnt);
	else launch_polar_energy(st, at, mu, c->d_e_static, rrms, c->d_scal);
	c->have_polar = true;
	return MPMC_OK;
}

// `polar_palmo` (:3517-3519, palmo_contraction :3602-3627): one more contraction with the final dipoles.  Under Jacobi the reference
// contracts the dipoles the last iteration read (mu is overwritten with new_mu only afterwards, :3526-3536), so it subtracts from the
// induced field that very field: zero to the bit, and nothing runs here.  Under Gauss-Seidel sweeps the dipoles are the swept ones:
// F = -(A_off mu) through the matrix-free Jacobi contraction (Gauss-Seidel contexts store nothing), against the induced field the
// last sweep used.  A failed iteration leaves the correction at 0 (:3483-3488).
static int stage_palmo(mpmc_ctx *c, const EvalPlan &p, const AtomsDev &at, const RecipDev &) {
	if (!p.palmo || c->failed) return MPMC_OK;
	double *mu = c->d_mu[c->mu_cur];
	// (the slots summed by the update kernel: d_palmo_f = F; its new dipoles go to the spare vector and are dropped, rrms untouched)
	// Under `polar_sor` / `polar_esor` palmo_contraction runs in front of the blend (:3517-3536): it contracts the swept dipoles, which the
	// last sweep left in the other vector, and the energy term takes the blended ones; the spare is then d_palmo_change, rewritten behind.
	double *contracted = p.relax ? c->d_mu[1 - c->mu_cur].p : mu, *spare = p.relax ? c->d_palmo_change.p : c->d_mu[1 - c->mu_cur].p;
	contract_into_field(c, at, contracted, spare, c->d_palmo_f, true,
	                    [&] { launch_palmo_reduce(c->stream, at, mu, c->d_palmo_f, c->d_e_induced, c->d_palmo_change, c->d_scal); });
	c->palmo_ran = true;
	c->relax_info.contractions += 1;
	return MPMC_OK;
}

// the terms added on top: each into its slots of the scalar block, in front of the post
static int stage_added_terms(mpmc_ctx *c, const EvalPlan &p, const AtomsDev &at, const RecipDev &) {
	hipStream_t st = c->stream;
	// ---- Axilrod-Teller, System::axilrod_teller (:129-136): into its slot of the scalar block, in front of the post below ----------------
	if (p.mask & RUN_THREE_BODY) {
		ProfScope ps(c, MPMC_K_THREE_BODY);
		launch_three_body(st, at, c->d_tb_au, c->box, kThreeBodyScale, c->d_tb_part, c->d_scal + S_THREE_BODY);
	}
	// ---- disp-expansion, System::disp_expansion (:121-122, 1939-2018): pair sum and the cached corrections into their three slots ----------
	if (p.mask & RUN_DISP) {
		ProfScope ps(c, MPMC_K_PAIR);
		launch_disp_expansion(st, at, c->d_de_co, c->d_de_t10, c->d_tile_pairs, c->n_tile_pairs, c->box, disp_params(c), c->de_lrc[0], c->de_lrc[1],
		                      c->d_de_part, c->d_scal + S_DISP);
	}
	// ---- rd_crystal, System::lj (:916-963): the lattice sum and its image-term count into their two slots ---------------------------------
	if (p.mask & RUN_CRYSTAL) {
		ProfScope ps(c, MPMC_K_PAIR);
		launch_crystal(st, at, c->box, crystal_params(c), c->d_rc_shift, c->d_tile_pairs, c->n_tile_pairs, c->d_rc_part, c->d_scal + S_CRYSTAL);
	}
	// ---- the rd model (:113-127): the pair sum, its kept terms and the skipped tile pairs into their three slots.  Tile pairs beyond the
	// cutoff are skipped by this evaluation's classes, where the pairwise pass made them and the cell is orthorhombic ----------------------
	if (p.mask & RUN_RDM) {
		ProfScope ps(c, MPMC_K_PAIR);
		const int *cls = (p.pair_pass && c->box.ortho && !c->kept.tune.no_classes) ? c->d_cls.p : nullptr;
		launch_rd_model(st, at, c->d_rdm_sp, c->d_tile_pairs, cls, c->n_tile_pairs, c->box, rd_model_params(c), c->d_rdm_part, c->d_scal + S_RDM);
	}
	// ---- Silvera-Goldman, System::sg (:115-116, 1763-1867): the pair sum and its kept terms into their two slots ------------------------
	if (p.mask & RUN_SG) {
		ProfScope ps(c, MPMC_K_PAIR);
		launch_sg(st, at, c->d_perm, c->d_tile_pairs, c->n_tile_pairs, c->box, sg_params(c), c->d_sg_part, c->d_scal + S_SG);
	}
	// ---- cavity_autoreject: the contact counts and the tile pairs it skipped into their three slots.  Its own tile-pair classes come from
	// this evaluation's tile bounding boxes, where the pairwise pass made them and the cell is orthorhombic ----------------------------------
	if (p.mask & RUN_CONTACT) {
		ProfScope ps(c, MPMC_K_PAIR);
		const bool skip = p.pair_pass && c->box.ortho && !c->kept.tune.no_classes && !c->kept.tune.no_contact_skip;
		launch_contact(st, at, c->kept.de_enabled ? c->d_de_co.p : c->d_rdm_sp.p, c->d_tile_pairs, c->n_tile_pairs, c->box, contact_params(c),
		               skip ? c->d_tile_bounds.p : nullptr, c->d_ca_cls, c->d_ca_part, c->d_scal + S_CA_REPLACED);
	}
	HIP_TRY(c, hipGetLastError());
	return MPMC_OK;
}

static int stage_post(mpmc_ctx *c, const EvalPlan &, const AtomsDev &, const RecipDev &) {
	// results to the pinned block by a kernel of ours (a blit and a stream synchronisation cost more than the whole reciprocal space of a
	// small box): copy, zero the device block for the next evaluation, launch number last
	c->single_seq += 1.0;
	launch_post_results(c->stream, c->d_scal, c->h_scal, c->single_seq);
	HIP_TRY(c, hipGetLastError());
	c->scal_clean = true;
	// short evaluations are polled for (a few us against ~10-15 for the synchronisation); long ones, and profiled ones (the event
	// harvest needs an idle stream), are waited for the ordinary way
	// (round 4: long evaluations are polled for as well, with a budget of a few of their own durations -- one evaluation at a time the
	// posted launch number is seen ~10 us before hipStreamSynchronize returns; an ensemble's first wait outlasts the budget and synchronises)
	c->spin_on_post = c->ev_used.empty() && (c->kept.tune.poll_long || c->n_tile_pairs <= kOneStreamMaxPairs);
	c->poll_budget_us = (c->n_tile_pairs <= kOneStreamMaxPairs) ? 1000 : 4000;
	c->pending = true;
	return MPMC_OK;
}

using Stage = int (*)(mpmc_ctx *, const EvalPlan &, const AtomsDev &, const RecipDev &);
static constexpr Stage kStages[] = {stage_clear_and_static_terms, stage_side_work,         stage_pair_pass,    stage_pair_reduce, stage_static_field,
                                    stage_direct_solve,           stage_gauss_seidel_solve, stage_jacobi_solve, stage_ewald_full_solve, stage_polar_energy,
                                    stage_palmo,
                                    stage_added_terms,            stage_post};

int mpmc::enqueue(mpmc_ctx *c, unsigned mask, bool on_demand, bool volume_trial) {
	// one evaluation per context at a time: a second enqueue would overwrite the scalar block and the result slots under the first
	if (c->pending) return fail(c, MPMC_ERR_ARG, "an evaluation of this context is still in flight (mpmc_energy_wait first)");
	// While a volume trial is open the resident cell, tables and positions may be the trial's: an evaluation would describe the trial
	// configuration, and a complete one would re-base the accepted totals on it, which a following reject then declares valid for the
	// accepted cell.  Refused, like the setters; the trial stays open.
	if (c->trial.open && c->trial.volume && !volume_trial)
		return fail(c, MPMC_ERR_ARG, "an evaluation was asked for while a volume trial is open (mpmc_trial_accept or mpmc_trial_reject first)");
	drop_pending_dipoles(c); // (its tables, slots and dipole vectors are this evaluation's from here on)
	// stale position-independent terms ride along with this evaluation (an insertion / removal makes them stale every time)
	int rc = prepare(c, true);
	if (rc != MPMC_OK) return rc;
	if ((mask & RUN_THREE_BODY) && (rc = three_body_ready(c)) != MPMC_OK) return rc;
	if ((mask & RUN_DISP) && (rc = disp_ready(c)) != MPMC_OK) return rc;
	if ((mask & RUN_CRYSTAL) && (rc = crystal_ready(c)) != MPMC_OK) return rc;
	if ((mask & RUN_RDM) && (rc = rd_model_ready(c)) != MPMC_OK) return rc;
	if ((mask & RUN_SG) && (rc = sg_ready(c)) != MPMC_OK) return rc;
	if ((mask & RUN_CONTACT) && (rc = contact_ready(c)) != MPMC_OK) return rc;
	if ((mask & RUN_SOLVE) && ewald_full_on(c)) {
		if (c->kept.palmo_enabled)
			return fail(c, MPMC_ERR_UNSUPPORTED, "polar_ewald_full with polar_palmo: ewald_palmo_contraction (System.Energy.cpp:3243-3267) is not part of the library");
		if (c->opts.polar_precision == 0.0 && c->opts.polar_max_iter < 0)
			return fail(c, MPMC_ERR_INVALID_SETTING, "polar_ewald_full: polar_max_iter must be >= 0 when polar_precision is 0 (the reference never terminates)");
		if (c->opts.polar_precision < 0.0) return fail(c, MPMC_ERR_INVALID_SETTING, "polar_ewald_full: polar_precision < 0");
	}
	if ((mask & RUN_SOLVE) && c->opts.polarization && !c->opts.rd_only) {
		if (c->kept.zodid && !c->opts.polar_iterative)
			return fail(c, MPMC_ERR_INCOMPATIBLE, "polar_zodid with polar_iterative off: the zeroth-order dipoles are the iterative solver's start (SimulationControl.cpp:2634)");
		if (c->kept.relax_scheme != RELAX_NONE && c->opts.polar_gamma < 0.0)
			return fail(c, MPMC_ERR_INVALID_SETTING, "polar_sor / polar_esor: polar_gamma must not be negative (SimulationControl.cpp:2714-2730)");
	}
	if ((mask & RUN_SOLVE) && c->kept.gs_ranked && c->opts.polar_gs && c->opts.polarization && !c->opts.rd_only)
		return fail(c, MPMC_ERR_INVALID_SETTING, "polar_gs and polar_gs_ranked are both on: choose one (SimulationControl.cpp:2732)");
	if (mask & RUN_SOLVE) {
		c->gr_info = mpmc_gs_ranked_info{};
		c->gr_ran = false;
		c->relax_info = mpmc_relax_info{};
		c->relax_info.scheme = c->kept.relax_scheme;
		c->relax_info.zodid = c->kept.zodid ? 1 : 0;
		c->relax_info.last_weight = 1.0;
	}
	c->static_ride_gen = 0;
	c->run_mask = mask;
	c->have_polar = c->direct_ran = c->palmo_ran = c->pef_ran = false;
	c->iters = c->failed = 0;
	c->last_was_single = c->spin_on_post = false;

	EvalPlan made = plan_evaluation(c, mask, on_demand);
	if (!made.single && (rc = make_room(c, made)) != MPMC_OK) return rc; // (before anything of this evaluation is on a stream)
	const EvalPlan &plan = made;
	const AtomsDev at = atoms_view(c);
	const RecipDev rcp = recip_view(c);
	if (plan.single) return stage_single_launch(c, plan, at, rcp);
	for (Stage stage : kStages)
		if ((rc = stage(c, plan, at, rcp)) != MPMC_OK) return rc;
	return MPMC_OK;
}


// measurement only (bench.py's roofline, cross-check): the panel Jacobi kernel `reps` times back to back between ONE pair of HIP events
// on the context's stream, per launch.  It agrees with the profiling mode's per-launch event brackets (92.7 against 92.9 us): what
// separates both from rocprofv3's kernel trace (86 us) is the dispatch / completion time between consecutive kernels of a stream, not
// the event records.  Needs the state a polarizable evaluation of a box on the panel path leaves behind; the partial slots it
// overwrites are dead by then.
extern "C" int mpmc_debug_time_panel(mpmc_ctx *c, int reps, double *ms_per_launch) {
	if (!c || !ms_per_launch || reps <= 0) return MPMC_ERR_ARG;
	if (c->pending) return fail(c, MPMC_ERR_ARG, "mpmc_debug_time_panel: an evaluation is in flight");
	if (!c->have_polar || !c->panels_built || c->solver_used != MPMC_SOLVER_COMPACT)
		return fail(c, MPMC_ERR_ARG, "mpmc_debug_time_panel: the last evaluation did not run the panel kernel");
	HIP_TRY(c, hipSetDevice(c->device));
	{ // (the launches below overwrite the partial slots an open on-demand solve would still read)
		const int rc_f = finish_pending_dipoles(c);
		if (rc_f != MPMC_OK) return rc_f;
	}
	const AtomsDev at = atoms_view(c);
	hipEvent_t e0, e1;
	HIP_TRY(c, hipEventCreate(&e0));
	HIP_TRY(c, hipEventCreate(&e1));
	// the contraction as the solve launches it (the update is a launch of its own and does not run here): it writes only the partial slots,
	// so the evaluation's results stay as they are
	for (int r = 0; r < 3; r++) // (warm)
		launch_dipole_iter_panel(c->stream, at, c->box, c->d_mu[c->mu_cur], c->d_tile_pairs, c->d_tp_shift, c->d_panels, c->n_panel_entries,
		                         c->d_ab, c->d_part, c->d_gpart);
	HIP_TRY(c, hipEventRecord(e0, c->stream));
	const int replicas = c->debug_panel_replicas; // (> 1: every launch carries the grid that many times: what a batched launch would cost per system)
	for (int r = 0; r < reps; r++)
		launch_dipole_iter_panel(c->stream, at, c->box, c->d_mu[c->mu_cur], c->d_tile_pairs, c->d_tp_shift, c->d_panels, c->n_panel_entries,
		                         c->d_ab, c->d_part, c->d_gpart, nullptr, nullptr, replicas);
	HIP_TRY(c, hipEventRecord(e1, c->stream));
	HIP_TRY(c, hipGetLastError());
	HIP_TRY(c, hipEventSynchronize(e1));
	float ms = 0;
	HIP_TRY(c, hipEventElapsedTime(&ms, e0, e1));
	(void)hipEventDestroy(e0);
	(void)hipEventDestroy(e1);
	*ms_per_launch = (double)ms / reps;
	return MPMC_OK;
}

// the same for the pair pass of the last evaluation (fast sweep or k_pair_fused, whichever ran): `reps` launches back to back between one
// pair of events.  Needs the classes of a complete evaluation; what it overwrites (block partials, field slots, tensor store) is rewritten
// identically, the configuration being the same.
extern "C" int mpmc_debug_time_pair(mpmc_ctx *c, int reps, double *ms_per_launch) {
	if (!c || !ms_per_launch || reps <= 0) return MPMC_ERR_ARG;
	if (c->pending) return fail(c, MPMC_ERR_ARG, "mpmc_debug_time_pair: an evaluation is in flight");
	if (!c->cache_valid || !c->last_fp_valid) return fail(c, MPMC_ERR_ARG, "mpmc_debug_time_pair: no complete evaluation has run");
	HIP_TRY(c, hipSetDevice(c->device));
	{ // (the sweep rewrites the slots and the store an open on-demand solve would still read)
		const int rc_f = finish_pending_dipoles(c);
		if (rc_f != MPMC_OK) return rc_f;
	}
	const AtomsDev at = atoms_view(c);
	const FusedParams &fp = c->last_fp;
	const bool compact = c->solver_used == MPMC_SOLVER_COMPACT && fp.do_thole;
	bool timed = false; // (the warm-up launches run the plain grid; the timed ones carry the replicas of "panel_replicas", if any)
	auto launch = [&] { launch_pair_pass(c, at, fp, compact, c->two_streams ? c->kept.tune.sweep_lds_pad : 0, timed ? c->debug_panel_replicas : 1); };
	hipEvent_t e0, e1;
	HIP_TRY(c, hipEventCreate(&e0));
	HIP_TRY(c, hipEventCreate(&e1));
	for (int r = 0; r < 2; r++) launch();
	timed = true;
	HIP_TRY(c, hipEventRecord(e0, c->stream));
	for (int r = 0; r < reps; r++) launch();
	HIP_TRY(c, hipEventRecord(e1, c->stream));
	HIP_TRY(c, hipGetLastError());
	HIP_TRY(c, hipEventSynchronize(e1));
	float ms = 0;
	HIP_TRY(c, hipEventElapsedTime(&ms, e0, e1));
	(void)hipEventDestroy(e0);
	(void)hipEventDestroy(e1);
	*ms_per_launch = (double)ms / reps;
	return MPMC_OK;
}

int mpmc::wait_and_fill(mpmc_ctx *c, mpmc_result *out) {
	if (!c->pending) return fail(c, MPMC_ERR_ARG, "mpmc_energy_wait: nothing enqueued");
	// a wait that fails must not leave the context refusing every later enqueue ("still in flight"): whatever happens below, the
	// evaluation is over for the host -- best-effort drain, state back to idle, scalar block marked dirty so that the next one clears it
	auto abandon = [c](hipError_t e, const char *what) {
		(void)hipStreamSynchronize(c->stream);
		if (c->two_streams && c->stream2) (void)hipStreamSynchronize(c->stream2);
		c->sync_stream = nullptr;
		c->pending = false;
		c->scal_clean = false;
		c->static_ride_gen = 0;
		drop_pending_dipoles(c);
		return fail(c, MPMC_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
	};
	hipError_t werr = c->kept.tune.fail_next_wait ? hipErrorUnknown : hipSetDevice(c->device);
	c->kept.tune.fail_next_wait = 0;
	if (werr != hipSuccess) return abandon(werr, "mpmc_energy_wait: hipSetDevice");
	bool seen = false;
	if (c->last_was_single || c->spin_on_post) {
		// the kernel posts its launch number behind the results (system-scope release): a short spin on the pinned slot returns a few
		// microseconds before the driver's own completion path would; past the budget, or if anything is off, fall back to the sync
		volatile const double *flag = c->h_scal + S_COUNT + C_COUNT;
		const double want = c->single_seq;
		seen = poll_posted(c, [&] { return *flag == want; }, std::chrono::microseconds(c->last_was_single ? 200 : c->poll_budget_us));
	}
	if (!seen) {
		c->kept.n_stream_syncs++;
		werr = hipStreamSynchronize(c->sync_stream ? c->sync_stream : c->stream);
		if (werr != hipSuccess) return abandon(werr, "mpmc_energy_wait: hipStreamSynchronize");
	} else if (c->kept.tune.poll_retire && c->n_tile_pairs > kOneStreamMaxPairs) {
		// the results are in, but the runtime has not been told: a stream that is never synchronised keeps its finished commands, and
		// the next asynchronous copy on it pays for the backlog (measured with positions handed over in host memory: 900 against 966
		// evaluations/s).  A query is enough to let it retire them.  Long evaluations only: the query costs a few microseconds, which is
		// a third of a 1000-atom LJ evaluation (23 -> 30 us when it ran behind every poll).
		(void)hipStreamQuery(c->stream);
		if (c->two_streams && c->stream2) (void)hipStreamQuery(c->stream2);
	}
	c->sync_stream = nullptr;
	c->pending = false;
	prof_harvest(c);
	if (c->direct_ran) { // the direct solve's verdict came with the results (copied in front of the post)
		c->direct.status = (int64_t)c->h_chol_info[0];
		c->direct.residual = (c->h_chol_info[2] > 0.0) ? c->h_chol_info[1] / c->h_chol_info[2] : 0.0;
		if (c->direct.status != 0) {
			c->failed = 1; // A is not positive definite: the caller rejects the configuration
			c->err = "direct dipole solve: the matrix is not positive definite (pivot " + std::to_string((long long)c->direct.status) + " of " +
			         std::to_string((long long)c->direct.n_unknowns) + " is not positive): dipoles and polarization energy set to 0";
		}
	}
	if (c->pef_ran) c->pef_info.n_real_pairs = (int64_t)c->h_pef_pairs[0]; // (copied in front of the post)
	if (c->gr_ran) { // the rank pass's scalars, likewise
		c->gr_info.rmin = c->h_gr_info[0].rmin;
		c->gr_info.max_rank = c->h_gr_info[0].max_rank;
		c->gr_info.n_moved = c->h_gr_info[0].n_moved;
	}
	ConfigTotals &ev = c->eval;
	if (c->run_mask & RUN_CONTACT) { // cavity_autoreject: the counts of this evaluation
		ev.ca.replaced = (int64_t)c->h_scal[S_CA_REPLACED];
		ev.ca.absolute = (int64_t)c->h_scal[S_CA_ABSOLUTE];
		c->ca_skipped = (int64_t)c->h_scal[S_CA_SKIPPED];
		c->ca_walked = (int64_t)c->n_tile_pairs - c->ca_skipped;
	}
	if (!out) return MPMC_OK;
	std::memset(out, 0, sizeof(*out));
	const double *s = c->h_scal;
	if (c->static_ride_gen) { // the position-independent terms came along: adopt them, unless something made them stale again meanwhile
		if (c->static_ride_gen == c->static_gen) {
			c->h_static[0] = s[S_LRC_PAIR];
			c->h_static[1] = s[S_LRC_SELF];
			c->h_static[2] = s[S_ES_SELF];
			c->static_dirty = false;
		}
		c->static_ride_gen = 0;
	}
	if (c->run_mask & RUN_DISP) { // disp_expansion() replaces lj() (:121-122): the LJ sums of the pair kernels are not used
		out->lj_pairs = s[S_DISP];
		out->lrc_pair = s[S_DISP_LRC_PAIR];
		out->lrc_self = s[S_DISP_LRC_SELF];
	} else {
		const bool lrc = (c->run_mask & RUN_ATOMTERMS) && c->opts.rd_lrc;
		out->lj_pairs = s[S_LJ];
		out->lrc_pair = lrc ? c->h_static[0] : 0.0;
		out->lrc_self = lrc ? c->h_static[1] : 0.0;
	}
	RdForm form = RdForm::PLAIN; // (by what this evaluation RAN: a component call's mask need not follow the switches)
	if (c->run_mask & RUN_CRYSTAL) { // the lattice sum replaces the LJ sum of the pair kernels; crystal_self joins in lj()'s order (:1011-1028)
		out->lj_pairs = s[S_CRYSTAL];
		form = RdForm::CRYSTAL_SELF;
		ev.rc_terms = (int64_t)s[S_CRYSTAL_TERMS];
		c->rc_info.order = c->rc_table_order;
		c->rc_info.n_images = c->rc_par.n_img;
		c->rc_info.cutoff = c->rc_cut;
		c->rc_info.n_image_terms = ev.rc_terms;
		c->rc_info.crystal_self = c->rc_self;
	}
	if (c->run_mask & RUN_RDM) { // the model's sum replaces the LJ sum of the pair kernels; the LJ form keeps lj()'s order of composition
		out->lj_pairs = s[S_RDM];
		if (c->kept.rdm_form == RD_FORM_LJ) {
			const bool lrc = (c->run_mask & RUN_ATOMTERMS) && c->opts.rd_lrc;
			out->lrc_pair = lrc ? c->rdm_lrc : 0.0;
			out->lrc_self = lrc ? c->h_static[1] : 0.0;
			form = RdForm::PLAIN;
		} else { // (lj_buffered_14_7() and dreiding() have no long-range correction)
			out->lrc_pair = out->lrc_self = 0.0;
			form = RdForm::NO_CORRECTIONS;
		}
		ev.rdm_terms = (int64_t)s[S_RDM_TERMS];
		c->rdm_info.form = c->kept.rdm_form;
		c->rdm_info.mixing = c->kept.rdm_mix;
		c->rdm_info.n_terms = ev.rdm_terms;
		c->rdm_info.n_tile_pairs = c->n_tile_pairs;
		c->rdm_info.n_tile_pairs_skipped = (int64_t)s[S_RDM_SKIPPED];
	}
	if (c->run_mask & RUN_SG) { // sg() is the whole of rd_energy (:115-116): no long-range correction, no rd_crystal sum
		out->lj_pairs = s[S_SG];
		out->lrc_pair = out->lrc_self = 0.0;
		form = RdForm::NO_CORRECTIONS;
		ev.sg_terms = (int64_t)s[S_SG_TERMS];
		c->sg_info.feynman_hibbs = c->opts.feynman_hibbs ? 1 : 0;
		c->sg_info.n_terms = ev.sg_terms;
		c->sg_info.cutoff = c->box.cutoff;
	}
	out->es_real = s[S_ES_REAL] - s[S_ES_INTRA];
	out->es_recip = s[S_ES_RECIP];
	out->es_self = (c->run_mask & RUN_RECIP) ? c->h_static[2] : 0.0;
	out->coulombic_energy = (out->es_real + out->es_recip) + out->es_self; // coulombic() :1412
	out->polarization_energy = s[S_POLAR];
	if (c->run_mask & RUN_SOLVE) c->palmo_correction = c->palmo_ran ? s[S_PALMO] : 0.0;
	out->dipole_rrms = s[S_RRMS];
	out->three_body_energy = (c->run_mask & RUN_THREE_BODY) ? s[S_THREE_BODY] : 0.0;
	out->N = c->N_movable;
	compose_totals(c, form, out);
	out->n_pairs = (int64_t)c->n * (c->n - 1) / 2;
	out->n_lj_in_cutoff = (c->run_mask & RUN_SG) ? 0 : c->h_cnt[C_LJ_IN]; // (no Lennard-Jones pass under Silvera-Goldman: mpmc_silvera_goldman_info counts its pairs)
	out->n_es_in_cutoff = c->h_cnt[C_ES_IN];
	out->n_intra = c->static_cnt[0];
	out->n_rd_excluded = c->static_cnt[1];
	out->n_es_excluded = c->static_cnt[2];
	out->n_frozen = c->static_cnt[3];
	out->polar_iterations = c->iters;
	out->iterator_failed = c->failed;
	ev.res = *out; // (whether this re-bases the accepted record is the caller's decision: rebase_on_eval)
	return MPMC_OK;
}

void mpmc::compose_totals(const mpmc_ctx *c, RdForm form, mpmc_result *r) {
	switch (form) {
	case RdForm::PLAIN: r->rd_energy = (r->lj_pairs + r->lrc_pair) + r->lrc_self; break;
	case RdForm::CRYSTAL_SELF: r->rd_energy = ((r->lj_pairs + r->lrc_pair) + c->rc_self) + r->lrc_self; break;
	case RdForm::NO_CORRECTIONS: r->rd_energy = r->lj_pairs; break;
	}
	r->energy = r->rd_energy + r->coulombic_energy + r->polarization_energy + r->vdw_energy + r->three_body_energy; // :136
	r->NU = r->N * r->energy; // :162
}

unsigned mpmc::full_mask(const mpmc_ctx *c) {
	if (sg_on(c)) // (:46, :115-116: sg() alone, no electrostatics, no polarization, no pair pass; Axilrod-Teller and the absolute contacts on top)
		return RUN_SG | (c->kept.tb_enabled ? RUN_THREE_BODY : 0u) | (contact_on(c) ? RUN_CONTACT : 0u);
	unsigned m = RUN_PAIR | RUN_ATOMTERMS;
	if (!c->opts.rd_only) {
		m |= RUN_PAIR_ES;
		m |= c->opts.wolf ? RUN_WOLF : RUN_RECIP; // coulombic() :1404-1413: Wolf replaces real + reciprocal + self
		if (c->opts.polarization) m |= RUN_FIELD | RUN_SOLVE;
	}
	if (c->kept.tb_enabled) m |= RUN_THREE_BODY; // (summed on top of everything else, rd_only too: :129-136)
	if (c->kept.de_enabled) m |= RUN_DISP;       // (in place of the LJ part of rd_energy; never the single-launch form)
	if (crystal_on(c)) m |= RUN_CRYSTAL;         // (in place of the LJ sum; disp_expansion() ignores rd_crystal)
	if (rd_model_on(c)) m |= RUN_RDM;            // (in place of the LJ part of rd_energy; never the single-launch form)
	if (contact_on(c)) m |= RUN_CONTACT;         // (cavity_autoreject: counts beside the energies; never the single-launch form)
	return m;
}

extern "C" int mpmc_energy_async(mpmc_ctx *c) {
	if (!c) return MPMC_ERR_ARG;
	return enqueue(c, full_mask(c), c->kept.on_demand);
}
extern "C" int mpmc_set_dipoles_on_demand(mpmc_ctx *c, int enabled) {
	if (!c) return MPMC_ERR_ARG;
	c->kept.on_demand = enabled != 0; // (from the next evaluation on; an open solve stays open)
	return MPMC_OK;
}
extern "C" int mpmc_hint_in_flight(mpmc_ctx *c, int n) {
	if (!c || n < 1) return MPMC_ERR_ARG;
	c->inflight_hint = n;
	return MPMC_OK;
}
// What leaves the library under cavity_autoreject.  r is the unpenalised result of a configuration with the contact counts n: the sigma
// rule's pairs get MAXVALUE in lj_pairs, and rd_energy, energy and NU follow (compose_totals); the absolute rule stays out of
// mpmc_result (it mirrors the observables) and shows in the info struct, which belongs to this delivery.
void mpmc::contact_penalise(const mpmc_ctx *c, mpmc_result *r, int64_t n_replaced) {
	if (!(c->kept.ca_rules & CA_RULE_SIGMA)) return;
	r->lj_pairs = r->lj_pairs + (double)n_replaced * kMaxValue;
	// (disp-expansion composes like lj(); the sigma rule never meets rd_crystal, contact_ready, so the form is never the one with crystal_self)
	compose_totals(c, rd_form_of(c), r);
}
void mpmc::contact_deliver(mpmc_ctx *c, mpmc_result *r, const ConfigTotals &t) {
	if (!contact_on(c) || !r) return;
	const ContactCounts &n = t.ca;
	const bool sigma = (c->kept.ca_rules & CA_RULE_SIGMA) != 0, absolute = (c->kept.ca_rules & CA_RULE_ABSOLUTE) != 0;
	struct mpmc_cavity_autoreject_info &info = c->ca_info;
	info = {};
	info.n_replaced = sigma ? n.replaced : 0;
	info.n_absolute = absolute ? n.absolute : 0;
	info.n_unmeasured_frozen = (absolute && !c->opts.polarization) ? (t.frozen_pairs >= 0 ? t.frozen_pairs : c->ca_frozen_pairs) : 0;
	info.tile_pairs_walked = c->ca_walked;
	info.tile_pairs_skipped = c->ca_skipped;
	contact_penalise(c, r, info.n_replaced);
	info.absolute_penalty = (info.n_absolute + info.n_unmeasured_frozen > 0) ? kMaxValue : 0.0;
	info.returned_energy = r->energy + info.absolute_penalty;
}

extern "C" int mpmc_energy_wait(mpmc_ctx *c, mpmc_result *out) {
	if (!c) return MPMC_ERR_ARG;
	const int rc = wait_and_fill(c, out);
	if (rc != MPMC_OK || !out) return rc;
	if (c->run_mask == full_mask(c)) rebase_on_eval(c); // a complete energy(): it re-bases the trial-move totals
	if (c->run_mask & RUN_CONTACT) contact_deliver(c, out, c->eval);
	return rc;
}
extern "C" int mpmc_energy(mpmc_ctx *c, mpmc_result *out) {
	if (!c || !out) return MPMC_ERR_ARG;
	c->inflight_hint = 1; // (a synchronous call: nothing else of this caller is in flight)
	int rc = enqueue(c, full_mask(c), c->kept.on_demand);
	if (rc != MPMC_OK) return rc;
	return mpmc_energy_wait(c, out);
}


// ---- component entry points --------------------------------------------------------------------------------
static int run_piece(mpmc_ctx *c, unsigned mask, mpmc_result *r) {
	if (!c) return MPMC_ERR_ARG;
	int rc = enqueue(c, mask);
	if (rc != MPMC_OK) return rc;
	rc = wait_and_fill(c, r);
	if (rc == MPMC_OK && c->run_mask == full_mask(c)) rebase_on_eval(c); // (a component call that is a complete energy(): lj() of an rd_only box)
	return rc;
}
extern "C" int mpmc_lj(mpmc_ctx *c, double *out) {
	mpmc_result r;
	if (!c) return MPMC_ERR_ARG;
	if (sg_on(c)) { // (sg() in place of lj(): a complete energy() when nothing else is on, and then it re-bases like one)
		int rc = run_piece(c, RUN_SG, &r);
		if (rc == MPMC_OK && out) *out = r.rd_energy;
		return rc;
	}
	// (cavity_autoreject: the sigma rule lives inside lj(); the absolute rule belongs to energy() alone)
	const bool contact = (c->kept.ca_rules & CA_RULE_SIGMA) != 0 && !c->kept.de_enabled; // (under disp-expansion the rule is disp_expansion()'s: mpmc_disp_expansion)
	int rc = run_piece(c, RUN_PAIR | RUN_ATOMTERMS | (crystal_on(c) ? RUN_CRYSTAL : 0u) | (rd_model_on(c) ? RUN_RDM : 0u) | (contact ? RUN_CONTACT : 0u), &r);
	if (rc == MPMC_OK && contact) contact_deliver(c, &r, c->eval);
	if (rc == MPMC_OK && out) *out = r.rd_energy;
	return rc;
}
extern "C" int mpmc_coulombic_real(mpmc_ctx *c, double *out) {
	mpmc_result r;
	int rc = run_piece(c, RUN_PAIR | RUN_PAIR_ES, &r);
	if (rc == MPMC_OK && out) *out = r.es_real;
	return rc;
}
extern "C" int mpmc_coulombic_reciprocal(mpmc_ctx *c, double *out) {
	mpmc_result r;
	int rc = run_piece(c, RUN_RECIP, &r);
	if (rc == MPMC_OK && out) *out = r.es_recip;
	return rc;
}
extern "C" int mpmc_coulombic_self(mpmc_ctx *c, double *out) {
	mpmc_result r;
	int rc = run_piece(c, RUN_RECIP, &r);
	if (rc == MPMC_OK && out) *out = r.es_self;
	return rc;
}
extern "C" int mpmc_coulombic(mpmc_ctx *c, double *out) {
	if (!c) return MPMC_ERR_ARG;
	mpmc_result r;
	int rc = run_piece(c, RUN_PAIR | RUN_PAIR_ES | (c->opts.wolf ? RUN_WOLF : RUN_RECIP), &r);
	if (rc == MPMC_OK && out) *out = r.coulombic_energy;
	return rc;
}
extern "C" int mpmc_polar(mpmc_ctx *c, double *out) {
	if (!c) return MPMC_ERR_ARG;
	if (!c->opts.polarization) return fail(c, MPMC_ERR_INVALID_SETTING, "mpmc_polar: polarization is off");
	mpmc_result r;
	int rc = run_piece(c, RUN_FIELD | RUN_SOLVE, &r);
	if (rc == MPMC_OK && out) *out = r.polarization_energy;
	return rc;
}
extern "C" int mpmc_axilrod_teller(mpmc_ctx *c, double *out) {
	if (!c) return MPMC_ERR_ARG;
	if (!c->kept.tb_enabled) return fail(c, MPMC_ERR_INVALID_SETTING, "mpmc_axilrod_teller: the term is off (mpmc_set_axilrod_teller)");
	mpmc_result r;
	int rc = run_piece(c, RUN_THREE_BODY, &r);
	if (rc == MPMC_OK && out) *out = r.three_body_energy;
	return rc;
}
extern "C" int mpmc_disp_expansion(mpmc_ctx *c, double *out) {
	if (!c) return MPMC_ERR_ARG;
	if (!c->kept.de_enabled) return fail(c, MPMC_ERR_INVALID_SETTING, "mpmc_disp_expansion: the term is off (mpmc_set_disp_expansion)");
	mpmc_result r;
	const bool contact = (c->kept.ca_rules & CA_RULE_SIGMA) != 0; // (cavity_autoreject: the sigma rule lives inside disp_expansion() too)
	int rc = run_piece(c, RUN_DISP | (contact ? RUN_CONTACT : 0u), &r);
	if (rc == MPMC_OK && contact) contact_deliver(c, &r, c->eval);
	if (rc == MPMC_OK && out) *out = r.rd_energy;
	return rc;
}
// device per-atom vectors are in slot order; everything handed to the caller is in original atom order
static int fetch_atoms3(mpmc_ctx *c, const double *d_src, double *out) {
	std::vector<double> tmp(3 * (size_t)c->n);
	HIP_TRY(c, hipMemcpyAsync(tmp.data(), d_src, tmp.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	for (int k = 0; k < c->n; k++) {
		const int i = c->perm[k];
		out[3 * (size_t)i] = tmp[3 * (size_t)k];
		out[3 * (size_t)i + 1] = tmp[3 * (size_t)k + 1];
		out[3 * (size_t)i + 2] = tmp[3 * (size_t)k + 2];
	}
	return MPMC_OK;
}

extern "C" int mpmc_thole_field(mpmc_ctx *c, double *ef_static) {
	if (!c) return MPMC_ERR_ARG;
	mpmc_result r;
	int rc = run_piece(c, RUN_FIELD, &r);
	if (rc != MPMC_OK) return rc;
	if (ef_static) return fetch_atoms3(c, c->d_e_static, ef_static);
	return MPMC_OK;
}

extern "C" int mpmc_thole_amatrix(mpmc_ctx *c, int row0, int nrows, double *a) {
	if (!c || !a || row0 < 0 || nrows <= 0) return MPMC_ERR_ARG;
	int rc = prepare(c);
	if (rc != MPMC_OK) return rc;
	if (row0 % 3 || nrows % 3 || row0 + nrows > 3 * c->n) return fail(c, MPMC_ERR_ARG, "mpmc_thole_amatrix: rows must cover whole atoms (multiples of 3) inside 3N");
	const size_t need = (size_t)nrows * 3 * c->n;
	if ((rc = c->d_arows.reserve(c, need)) != MPMC_OK) return rc;
	{
		ProfScope p(c, MPMC_K_TENSOR);
		launch_amatrix_rows(c->stream, atoms_view(c), c->d_slot_of, c->box, c->opts.polar_damp, row0, nrows, c->d_arows);
	}
	HIP_TRY(c, hipGetLastError());
	HIP_TRY(c, hipMemcpyAsync(a, c->d_arows, need * sizeof(double), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	prof_harvest(c);
	return MPMC_OK;
}

extern "C" int mpmc_polar_direct_info(mpmc_ctx *c, mpmc_direct_info *out) {
	if (!c || !out) return MPMC_ERR_ARG;
	if (c->pending) return fail(c, MPMC_ERR_ARG, "mpmc_polar_direct_info: an evaluation is in flight");
	*out = c->direct;
	return MPMC_OK;
}

// the Palmo-Krimm correction of the last evaluation with a dipole solve and its per-atom ef_induced_change (zeros where no contraction ran)
extern "C" int mpmc_polar_palmo_info(mpmc_ctx *c, double *energy_correction, double *ef_induced_change) {
	if (!c) return MPMC_ERR_ARG;
	if (c->pending) return fail(c, MPMC_ERR_ARG, "mpmc_polar_palmo_info: an evaluation is in flight");
	if (energy_correction) *energy_correction = c->palmo_correction;
	if (ef_induced_change) {
		if (c->palmo_ran && c->d_palmo_change) {
			HIP_TRY(c, hipSetDevice(c->device));
			return fetch_atoms3(c, c->d_palmo_change, ef_induced_change);
		}
		std::fill(ef_induced_change, ef_induced_change + 3 * (size_t)c->n, 0.0);
	}
	return MPMC_OK;
}

extern "C" int mpmc_get_dipoles(mpmc_ctx *c, double *mu, double *ef_static, double *ef_induced) {
	if (!c) return MPMC_ERR_ARG;
	if (!c->d_e_static) return fail(c, MPMC_ERR_ARG, "mpmc_get_dipoles: no polarization evaluation has run");
	HIP_TRY(c, hipSetDevice(c->device));
	int rc = finish_pending_dipoles(c); // an on-demand evaluation's remaining iterations; an error when its inputs are gone
	if (rc != MPMC_OK) return rc;
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	if (mu && rc == MPMC_OK) rc = fetch_atoms3(c, c->d_mu[c->mu_cur], mu);
	if (ef_static && rc == MPMC_OK) rc = fetch_atoms3(c, c->d_e_static, ef_static);
	if (ef_induced && rc == MPMC_OK) rc = fetch_atoms3(c, c->d_e_induced, ef_induced);
	return rc;
}

// update_com + wrap_all, reference src/System.cpp:1347-1425, over the host mirror of the accepted atom list (which must carry masses): the
// centres of mass, the lattice shift of each (zero for a frozen molecule) and every atom's wrapped_pos = its position minus that shift.
// Any pointer may be null.  (host side, O(N): mpmc_update_com hands it out, mpmc_cavity_update bins it)
void mpmc::wrap_molecules(const mpmc_ctx *c, double *com, double *wrapped_com, double *wrapped_pos) {
	int m = 0;
	for (int i0 = 0; i0 < c->n;) {
		int i1 = i0;
		while (i1 + 1 < c->n && c->h_mol[i1 + 1] == c->h_mol[i0]) i1++;
		double cm[3] = {0, 0, 0}, mass = 0;
		for (int i = i0; i <= i1; i++) {
			mass += c->h_mass[i];
			for (int p = 0; p < 3; p++) cm[p] += c->h_mass[i] * c->h_pos[3 * i + p];
		}
		for (int p = 0; p < 3; p++) cm[p] /= mass;
		const bool mol_frozen = c->h_frozen[i1] != 0;
		double w[3] = {0, 0, 0};
		if (!mol_frozen) {
			double d[3];
			for (int p = 0; p < 3; p++) {
				d[p] = 0;
				for (int q = 0; q < 3; q++) d[p] += c->box.r[3 * q + p] * cm[q];
				d[p] = std::rint(d[p]);
			}
			for (int p = 0; p < 3; p++) {
				w[p] = 0;
				for (int q = 0; q < 3; q++) w[p] += c->box.b[3 * q + p] * d[q];
			}
		}
		if (com)
			for (int p = 0; p < 3; p++) com[3 * m + p] = cm[p];
		if (wrapped_com)
			for (int p = 0; p < 3; p++) wrapped_com[3 * m + p] = w[p]; // the reference stores the lattice shift here (:1404)
		if (wrapped_pos)
			for (int i = i0; i <= i1; i++)
				for (int p = 0; p < 3; p++) wrapped_pos[3 * i + p] = mol_frozen ? c->h_pos[3 * i + p] : c->h_pos[3 * i + p] - w[p];
		m++;
		i0 = i1 + 1;
	}
}

extern "C" int mpmc_update_com(mpmc_ctx *c, double *com, double *wrapped_com, double *wrapped_pos, int *n_molecules) {
	if (!c) return MPMC_ERR_ARG;
	if (!c->atoms_set || !c->box_set) return fail(c, MPMC_ERR_ARG, "mpmc_update_com: atoms and box must be set");
	if (c->h_mass.empty()) return fail(c, MPMC_ERR_ARG, "mpmc_update_com: mpmc_set_atoms was called without masses");
	if (n_molecules) *n_molecules = c->n_molecules;
	wrap_molecules(c, com, wrapped_com, wrapped_pos);
	return MPMC_OK;
}
