// trial.cpp -- per-move delta energies (mpmc_trial_*): the device-side counterpart of the reference's per-pair cache
// (part of libmpmc_energy.so; shared state and helpers: context.h.  There is no CPU fallback anywhere in this library.)
#include <atomic>
#include <chrono>

#include "context.h"


using namespace mpmc;

// ---- trial moves -----------------------------------------------------------------------------------------------
constexpr size_t kMvBlobBytes = MPMC_TRIAL_MAX_ATOMS * (2 * sizeof(int) + sizeof(double4));
static int ensure_trial_buffers(mpmc_ctx *c) {
	int rc;
	if (!c->h_mv_blob) { // (the last step of the first use)
		if ((rc = c->d_mv_blob.reserve(c, kMvBlobBytes)) != MPMC_OK) return rc;
		c->d_mv_new = reinterpret_cast<double4 *>(c->d_mv_blob.p); // 32-byte records first (alignment), then the two int lists
		c->d_mv_slot = reinterpret_cast<int *>(c->d_mv_blob + MPMC_TRIAL_MAX_ATOMS * sizeof(double4));
		c->d_mv_orig = c->d_mv_slot + MPMC_TRIAL_MAX_ATOMS;
		if ((rc = c->d_moved_idx.reserve(c, (size_t)c->max_pad)) != MPMC_OK) return rc;
		if ((rc = c->d_delta_out.reserve(c, D_COUNT)) != MPMC_OK) return rc; // (the D_* slots, kernels.h)
		HIP_TRY(c, hipMemsetAsync(c->d_delta_out, 0, D_COUNT * sizeof(double), c->stream));
		c->d_delta_cnt = reinterpret_cast<long long *>(c->d_delta_out + D_CNT_LJ);
		HIP_TRY(c, hipMemsetAsync(c->d_moved_idx, 0xff, (size_t)c->max_pad * sizeof(int), c->stream)); // all -1; on our stream (ordered before the first delta kernel)
		if ((rc = c->h_delta_out.reserve(c, kDeltaHostCount)) != MPMC_OK) return rc;
		for (int k = kDeltaHostSeq; k < kDeltaHostCount; k++) c->h_delta_out[k] = 0.0;
		c->h_delta_cnt = reinterpret_cast<long long *>(c->h_delta_out + delta_host_index(D_CNT_LJ));
		if ((rc = c->h_mv_blob.reserve(c, kMvBlobBytes)) != MPMC_OK) return rc;
	}
	return c->d_sf_trial.reserve(c, (size_t)c->K);
}

// a trial of `count` atoms from `at` on is open: a displacement (kind 0), an insertion (+1) or a removal (-1); nothing of it is evaluated yet
static void open_trial(mpmc_ctx *c, int kind, int at, int count) {
	TrialState &t = c->trial;
	t.xch_kind = kind;
	t.xch_at = t.first = at;
	t.count = count;
	t.xch_saved.clear();
	t.volume = t.vol_swapped = t.vol_host_pos = false;
	t.open = true;
	t.evaluated = t.enqueued = t.noop = false;
}

extern "C" int mpmc_trial_begin(mpmc_ctx *c, int first, int count, const double *new_pos) {
	if (!c || !new_pos || first < 0 || count <= 0) return MPMC_ERR_ARG;
	if (!c->atoms_set || first + count > c->n) return fail(c, MPMC_ERR_ARG, "mpmc_trial_begin: range outside the atom list");
	if (c->trial.open) return fail(c, MPMC_ERR_ARG, "mpmc_trial_begin: a trial move is already open (accept or reject it first)");
	if (!c->cache_valid) return fail(c, MPMC_ERR_ARG, "mpmc_trial_begin: no accepted configuration (call mpmc_energy first)");
	for (int t = 0; t < 3 * count; t++)
		if (!std::isfinite(new_pos[t])) return fail(c, MPMC_ERR_INVALID_DATUM, "mpmc_trial_begin: non-finite position");
	open_trial(c, 0, first, count);
	c->trial.pos_new.assign(new_pos, new_pos + 3 * (size_t)count);
	c->trial.pos_old.assign(c->h_pos.begin() + 3 * (size_t)first, c->h_pos.begin() + 3 * (size_t)(first + count));
	// a "move" that leaves every coordinate as it is (e.g. the box a two-box move does not touch): the trial totals ARE the accepted
	// totals, nothing is evaluated.  (The reference's bead moves re-centre the whole chain, so they do touch every image.)
	c->trial.noop = (std::memcmp(new_pos, c->h_pos.data() + 3 * (size_t)first, 3 * (size_t)count * sizeof(double)) == 0);
	return MPMC_OK;
}

// ---- exchange trials: insertion / removal of one molecule ----------------------------------------------------------------------------------
static int xch_begin_checks(mpmc_ctx *c, const char *who) {
	const std::string w(who);
	if (!c->atoms_set) return fail(c, MPMC_ERR_ARG, w + ": no atoms set");
	if (c->trial.open) return fail(c, MPMC_ERR_ARG, w + ": a trial move is already open (accept or reject it first)");
	// (the per-atom coefficients of these two terms belong to one atom list, and an exchange trial has no way to hand over the new atoms';
	// in front of the accepted-configuration check: switching either term on drops the accepted totals, and the answer to an exchange trial
	// on such a context is "never", not "call mpmc_energy first")
	if (c->kept.tb_enabled || c->kept.de_enabled)
		return fail(c, MPMC_ERR_UNSUPPORTED, w + ": a context with Axilrod-Teller or disp-expansion coefficients changes its composition through mpmc_set_atoms");
	if (!c->cache_valid) return fail(c, MPMC_ERR_ARG, w + ": no accepted configuration (call mpmc_energy first)");
	return MPMC_OK;
}

// an inserted molecule's data, `n_poses` poses of it: finite positions, sane parameters, masses where the list has them
static int xch_molecule_checks(mpmc_ctx *c, const char *who, int count, int n_poses, const double *pos, const double *charge, const double *polarizability,
                               const double *epsilon, const double *sigma, const double *mass) {
	const std::string w(who);
	for (size_t t = 0; t < 3 * (size_t)count * (size_t)n_poses; t++)
		if (!std::isfinite(pos[t])) return fail(c, MPMC_ERR_INVALID_DATUM, w + ": non-finite position");
	for (int i = 0; i < count; i++)
		if (epsilon[i] < 0.0 || !std::isfinite(epsilon[i]) || !std::isfinite(sigma[i]) || !std::isfinite(charge[i]) || !std::isfinite(polarizability[i]))
			return fail(c, MPMC_ERR_INVALID_DATUM, w + ": epsilon < 0 or non-finite atom parameter");
	if (!c->h_mass.empty() && !mass) return fail(c, MPMC_ERR_INVALID_DATUM, w + ": the atom list has masses, the molecule needs them too");
	return MPMC_OK;
}
// the largest molecule id in use: known from the host sums of the accepted list, else found now
static int32_t xch_largest_mol_id(const mpmc_ctx *c) {
	int32_t id = c->h_mol[0];
	if (c->xs_gen == c->static_gen) id = c->xs_acc.mol_max;
	else
		for (int i = 1; i < c->n; i++) id = std::max(id, c->h_mol[i]);
	return id;
}
// one new molecule with the id `id`, which no resident atom has (pos: the first pose)
static void xch_fill_molecule(const mpmc_ctx *c, AtomRun &m, int32_t id, int count, const double *pos, const double *charge, const double *polarizability,
                              const double *epsilon, const double *sigma, const int32_t *frozen, const int32_t *has_disp, const double *mass) {
	m.pos.assign(pos, pos + 3 * (size_t)count);
	m.q.assign(charge, charge + count);
	m.alpha.assign(polarizability, polarizability + count);
	m.eps.assign(epsilon, epsilon + count);
	m.sigma.assign(sigma, sigma + count);
	m.frozen.assign(frozen, frozen + count);
	if (has_disp) m.disp.assign(has_disp, has_disp + count);
	else m.disp.assign(count, 0);
	if (!c->h_mass.empty()) m.mass.assign(mass, mass + count); // (a list without masses takes none)
	else m.mass.clear();
	m.mol.assign(count, id);
}

extern "C" int mpmc_trial_insert_begin(mpmc_ctx *c, int at_index, int count, const double *pos, const double *charge, const double *polarizability,
                                       const double *epsilon, const double *sigma, const int32_t *frozen, const int32_t *has_disp, const double *mass) {
	if (!c || count <= 0 || !pos || !charge || !polarizability || !epsilon || !sigma || !frozen) return MPMC_ERR_ARG;
	int rc = xch_begin_checks(c, "mpmc_trial_insert_begin");
	if (rc != MPMC_OK) return rc;
	if (at_index < 0 || at_index > c->n) return fail(c, MPMC_ERR_ARG, "mpmc_trial_insert_begin: at_index outside the atom list");
	if (at_index > 0 && at_index < c->n && c->h_mol[at_index - 1] == c->h_mol[at_index])
		return fail(c, MPMC_ERR_ARG, "mpmc_trial_insert_begin: at_index lies inside a molecule (it must be a molecule boundary)");
	if ((rc = xch_molecule_checks(c, "mpmc_trial_insert_begin", count, 1, pos, charge, polarizability, epsilon, sigma, mass)) != MPMC_OK) return rc;
	const int32_t id = xch_largest_mol_id(c);
	if (id == INT32_MAX) return fail(c, MPMC_ERR_ARG, "mpmc_trial_insert_begin: no molecule id left");
	xch_fill_molecule(c, c->trial.xch_mol, id + 1, count, pos, charge, polarizability, epsilon, sigma, frozen, has_disp, mass);
	open_trial(c, +1, at_index, count);
	return MPMC_OK;
}

extern "C" int mpmc_trial_remove_begin(mpmc_ctx *c, int first, int count) {
	if (!c || count <= 0) return MPMC_ERR_ARG;
	int rc = xch_begin_checks(c, "mpmc_trial_remove_begin");
	if (rc != MPMC_OK) return rc;
	if (first < 0 || first + count > c->n) return fail(c, MPMC_ERR_ARG, "mpmc_trial_remove_begin: range outside the atom list");
	bool whole = (first == 0 || c->h_mol[first - 1] != c->h_mol[first]) && (first + count == c->n || c->h_mol[first + count] != c->h_mol[first + count - 1]);
	for (int i = first + 1; i < first + count; i++) whole = whole && c->h_mol[i] == c->h_mol[first];
	if (!whole) return fail(c, MPMC_ERR_ARG, "mpmc_trial_remove_begin: the range is not exactly one whole molecule");
	if (count == c->n) return fail(c, MPMC_ERR_ARG, "mpmc_trial_remove_begin: the last molecule cannot be removed");
	copy_atom_run(c, first, count, c->trial.xch_mol);
	open_trial(c, -1, first, count);
	return MPMC_OK;
}

// the trial list: the accepted one with the molecule in or out
static void xch_trial_list(const mpmc_ctx *c, const AtomRun &acc, AtomRun &out) {
	out = acc;
	const size_t at = (size_t)c->trial.xch_at, m = (size_t)c->trial.count;
	const AtomRun &mol = c->trial.xch_mol;
	auto edit = [&](auto &v, const auto &ins, size_t per) {
		if (c->trial.xch_kind > 0) v.insert(v.begin() + per * at, ins.begin(), ins.end());
		else v.erase(v.begin() + per * at, v.begin() + per * (at + m));
	};
	edit(out.pos, mol.pos, 3);
	edit(out.q, mol.q, 1);
	edit(out.alpha, mol.alpha, 1);
	edit(out.eps, mol.eps, 1);
	edit(out.sigma, mol.sigma, 1);
	edit(out.mol, mol.mol, 1);
	edit(out.frozen, mol.frozen, 1);
	edit(out.disp, mol.disp, 1);
	if (!out.mass.empty()) edit(out.mass, mol.mass, 1);
}

// mpmc_set_atoms closes the open trial and may rebuild the context in place (growth): the trial state, the accepted record and the
// diagnostic of the last trial cross the call in the caller's hands, each as a whole (cache_valid does not: the caller sets it again)
static int xch_replace_list(mpmc_ctx *c, const AtomRun &list, AtomRun &&saved) {
	TrialState trial = std::move(c->trial);
	const ConfigTotals accepted = c->accepted;
	const int last_kind = c->trial_last_kind;
	const int rc = set_atoms_from(c, list);
	c->trial = std::move(trial);
	c->accepted = accepted;
	c->trial_last_kind = last_kind;
	c->trial.xch_saved = std::move(saved);
	c->trial.open = true;
	c->trial.enqueued = c->trial.noop = false;
	return rc;
}

// What an exchange trial takes from the molecule's species and the accepted list alone, whatever the pose: the host sums of the trial
// composition (xs_trial) with its position-independent terms st = { lrc_pair, lrc_self, es_self } and its count N of movable molecules, and
// the staged records (rec[m]; the positions are mol.pos's).  The sums of the accepted list are made first where they are stale.
static void xch_species_terms(mpmc_ctx *c, int kind, const AtomRun &mol, XchSums &xs_trial, double st[3], double &N, XchAtom *rec) {
	const int m = mol.size();
	const double sg = kind > 0 ? 1.0 : -1.0;
	// the position-independent terms of the trial composition, from the sums of the accepted list
	if (c->xs_gen != c->static_gen || c->xs_edits >= kXchResum) {
		xch_sum_list(c, c->xs_acc);
		c->xs_gen = c->static_gen;
		c->xs_edits = 0;
		c->kept.n_xch_resums++;
	}
	xs_trial = c->xs_acc;
	double molmass = 0.0;
	for (double v : mol.mass) molmass += v;
	for (int k = 0; k < m; k++) {
		const int fl = atom_flag_word(c, mol.frozen[k], mol.eps[k], mol.sigma[k], mol.disp[k], mol.q[k], mol.alpha[k]);
		xch_sum_atom(c, xs_trial, sg, fl, mol.sigma[k], mol.eps[k], mol.q[k]);
		XchAtom &g = rec[k];
		g.xyzq = make_double4(mol.pos[3 * k], mol.pos[3 * k + 1], mol.pos[3 * k + 2], mol.q[k]);
		g.lj = make_double2(std::fabs(mol.sigma[k]), std::sqrt(mol.eps[k]));
		g.mf = make_int2(mol.mol[k], fl);
		g.inv_molmass = (molmass > 0.0) ? 1.0 / molmass : 0.0;
	}
	if (kind > 0) xs_trial.mol_max = std::max(xs_trial.mol_max, mol.mol[0]);
	xch_static_terms(c, xs_trial, st);
	N = c->N_movable + (mol.frozen[m - 1] ? 0.0 : sg); // (a molecule's flag is its last atom's, mpmc_set_atoms)
}

static int xch_energy_async(mpmc_ctx *c) {
	const mpmc_options &o = c->opts;
	const bool polar = o.polarization && !o.rd_only;
	const int m = c->trial.count, kind = c->trial.xch_kind;
	c->trial.polar_delta = false;
	c->trial.inline_move = false;
	if (polar || m > MPMC_TRIAL_MAX_ATOMS || crystal_on(c) || rd_model_on(c) || sg_on(c)) {
		// the dipole solve couples every atom, and the further terms have no exchange delta: the trial composition is evaluated in full
		AtomRun acc, list;
		copy_atom_run(c, 0, c->n, acc);
		xch_trial_list(c, acc, list);
		int rc = xch_replace_list(c, list, std::move(acc));
		if (rc != MPMC_OK) return rc;
		if ((rc = enqueue(c, full_mask(c))) != MPMC_OK) return rc;
		c->trial.was_full = true;
		c->trial_last_kind = 1;
		c->trial.enqueued = true;
		c->kept.n_xch_full++;
		return MPMC_OK;
	}
	drop_pending_dipoles(c);
	int rc = prepare(c);
	if (rc != MPMC_OK) return rc;
	if ((rc = ensure_trial_buffers(c)) != MPMC_OK) return rc;
	if ((rc = c->d_xch_mol.reserve(c, MPMC_TRIAL_MAX_ATOMS)) != MPMC_OK) return rc;
	if ((rc = c->h_xch_mol.reserve(c, MPMC_TRIAL_MAX_ATOMS)) != MPMC_OK) return rc;
	// (one more pair of partials than tiles: the molecule's own block; a one-tile table is shorter than that)
	if ((rc = c->d_block_part.reserve(c, 2 * ((size_t)c->n_tiles + 1))) != MPMC_OK) return rc;
	if ((rc = c->d_block_cnt.reserve(c, 2 * ((size_t)c->n_tiles + 1))) != MPMC_OK) return rc;
	const double sg = kind > 0 ? 1.0 : -1.0;
	xch_species_terms(c, kind, c->trial.xch_mol, c->xs_trial, c->trial.xch_static, c->trial.xch_N, c->h_xch_mol);
	hipStream_t st = c->stream;
	HIP_TRY(c, hipMemcpyAsync(c->d_xch_mol, c->h_xch_mol, (size_t)m * sizeof(XchAtom), hipMemcpyHostToDevice, st));
	const int do_es = o.rd_only ? 0 : 1;
	if (contact_on(c)) {
		// cavity_autoreject: the molecule's contacts with the residents, signed, into D_CA_REPLACED and D_CA_ABSOLUTE of the delta result block,
		// which k_delta_finish posts with everything else (the unmeasured frozen pairs of the trial composition: the wait, from the host's counts)
		if ((rc = contact_ready(c)) != MPMC_OK) return rc;
		if ((rc = c->d_ca_xpart.reserve(c, 2 * (size_t)c->n_tiles)) != MPMC_OK) return rc;
		ProfScope p(c, MPMC_K_PAIR);
		launch_exchange_contact(st, atoms_view(c), c->box, contact_params(c), c->d_xch_mol, m, 1, sg, c->d_ca_xpart, c->d_delta_out + D_CA_REPLACED, nullptr);
	}
	{
		FusedParams fp{};
		fp.ewald_alpha = c->ewald_alpha;
		ext_params(c, fp, o.wolf && do_es);
		ProfScope p(c, MPMC_K_PAIR);
		launch_exchange(st, atoms_view(c), c->box, recip_view(c), fp, do_es, c->d_xch_mol, m, sg, c->d_sf_trial, c->d_block_part, c->d_block_cnt, c->d_delta_out,
		                c->d_delta_cnt, c->h_delta_out, (c->trial_seq += 1.0));
	}
	HIP_TRY(c, hipGetLastError());
	c->trial.was_full = false;
	c->trial_last_kind = 0;
	c->trial.enqueued = true;
	c->kept.n_xch_delta++;
	return MPMC_OK;
}

// the position-independent pair counts an exchange changes (k_static_counts): the molecule's atoms against the classes of everybody else
// (`others`: the histogram of the list WITHOUT the molecule), and among themselves; d = { intra, rd_excluded, es_excluded, frozen }
static void xch_pair_counts(const mpmc_ctx *c, const AtomRun &mol, const long long *others, long long d[4]) {
	const int m = mol.size();
	d[0] = d[1] = d[2] = d[3] = 0;
	std::vector<int> fl((size_t)m);
	for (int k = 0; k < m; k++) fl[k] = atom_flag_word(c, mol.frozen[k], mol.eps[k], mol.sigma[k], mol.disp[k], mol.q[k], mol.alpha[k]);
	for (int cl = 0; cl < kXchClasses; cl++) {
		if (!others[cl]) continue;
		const int cf = ((cl & 1) ? AF_FROZEN : 0) | ((cl & 2) ? AF_NULL_RD : 0) | ((cl & 4) ? AF_HAS_DISP : 0) | ((cl & 8) ? AF_ZERO_Q : 0);
		for (int k = 0; k < m; k++) {
			const PairFlags f = pair_flags(0, fl[k], 1, cf);
			d[1] += f.rd_excluded ? others[cl] : 0;
			d[2] += f.es_excluded ? others[cl] : 0;
			d[3] += f.frozen ? others[cl] : 0;
		}
	}
	for (int k = 0; k < m; k++)
		for (int l = k + 1; l < m; l++) {
			const PairFlags f = pair_flags(0, fl[k], 0, fl[l]);
			d[0] += f.intra, d[1] += f.rd_excluded, d[2] += f.es_excluded, d[3] += f.frozen;
		}
}

// the result of an exchange of `m` atoms (kind +1 | -1) on the delta path: the accepted totals, the signed changes the device left (p), the
// position-independent terms st and count N of the trial composition, and the changes d of the position-independent pair counts.  The
// single trial (xch_result) and the batched insertion candidates (mpmc_insert_candidates) both end here.
static void xch_compose(const mpmc_ctx *c, int kind, int m, const InsCandOut &p, const double st[3], double N, const long long d[4], mpmc_result &r) {
	const mpmc_options &o = c->opts;
	const int do_es = o.rd_only ? 0 : 1;
	const mpmc_result &a = c->accepted.res;
	r = a;
	r.lj_pairs = a.lj_pairs + p.lj;
	r.lrc_pair = o.rd_lrc ? st[0] : 0.0;
	r.lrc_self = o.rd_lrc ? st[1] : 0.0;
	r.n_lj_in_cutoff = a.n_lj_in_cutoff + p.n_lj;
	if (do_es) {
		r.es_real = a.es_real + (p.es_real - p.es_intra);
		r.es_recip = p.es_recip;
		r.es_self = o.wolf ? 0.0 : st[2];
		r.coulombic_energy = (r.es_real + r.es_recip) + r.es_self;
		r.n_es_in_cutoff = a.n_es_in_cutoff + p.n_es;
	}
	r.N = N;
	compose_totals(c, RdForm::PLAIN, &r); // (rd_crystal and the rd models have no exchange delta: xch_energy_async)
	const int64_t n_new = (int64_t)c->n + (kind > 0 ? m : -m);
	r.n_pairs = n_new * (n_new - 1) / 2;
	const long long sgn = kind > 0 ? 1 : -1;
	r.n_intra = a.n_intra + sgn * d[0];
	r.n_rd_excluded = a.n_rd_excluded + sgn * d[1];
	r.n_es_excluded = a.n_es_excluded + sgn * d[2];
	r.n_frozen = a.n_frozen + sgn * d[3];
}

// the result of the open exchange trial of the delta path, from the block k_delta_finish posted
static void xch_result(mpmc_ctx *c, mpmc_result &r) {
	const double *dh = c->h_delta_out.p;
	InsCandOut p;
	p.lj = dh[delta_host_index(D_LJ)];
	p.es_real = dh[delta_host_index(D_ES_REAL)];
	p.es_intra = dh[delta_host_index(D_ES_INTRA)];
	p.es_recip = dh[delta_host_index(D_ES_RECIP)];
	p.n_lj = c->h_delta_cnt[0];
	p.n_es = c->h_delta_cnt[1];
	long long d[4];
	xch_pair_counts(c, c->trial.xch_mol, (c->trial.xch_kind > 0) ? c->xs_acc.cls : c->xs_trial.cls, d);
	xch_compose(c, c->trial.xch_kind, c->trial.count, p, c->trial.xch_static, c->trial.xch_N, d, r);
}

// accept of the delta path: the list is edited in place; a context that has to grow is rebuilt around the new list and evaluated once
// (the accepted record is the caller's: mpmc_trial_accept makes it the trial's)
static int xch_accept_delta(mpmc_ctx *c) {
	const int m = c->trial.count, kind = c->trial.xch_kind;
	const int n_new = c->n + (kind > 0 ? m : -m);
	if (n_new > c->max_atoms) { // (rare: the capacity grows by a quarter each time)
		AtomRun acc, list;
		copy_atom_run(c, 0, c->n, acc);
		xch_trial_list(c, acc, list);
		int rc = xch_replace_list(c, list, AtomRun{});
		c->trial.open = false;
		mpmc_result tmp;
		if (rc == MPMC_OK) rc = mpmc_energy(c, &tmp); // the fresh context's structure factors and position-independent terms (it re-bases, cache_valid with it)
		return rc;
	}
	std::swap(c->d_sf, c->d_sf_trial); // (each buffer with its own capacity)
	const int rc = splice_atoms(c, c->trial.xch_at, kind < 0 ? m : 0, kind > 0 ? &c->trial.xch_mol : nullptr);
	if (rc != MPMC_OK) return rc;
	for (int k = 0; k < 3; k++) c->h_static[k] = c->trial.xch_static[k];
	c->static_dirty = false;
	c->xs_acc = c->xs_trial;
	c->xs_edits++;
	return MPMC_OK;
}

// ---- volume trials: System::volume_change / volume_change_Gibbs / revert_volume_change (src/System.MonteCarlo.cpp:1235-1340, 1690-1727) -----
// The trial is a full evaluation of the scaled cell and the scaled positions, made in the ALTERNATES of everything the accepted
// configuration keeps on the device: a second position buffer (kernels_volume.hip writes it), a second set of k tables, and d_sf_trial for
// the structure factors.  They trade places with the accepted ones in front of the evaluation; reject trades them back and restores the
// host's cell, alphas and position-independent terms, so nothing is evaluated again; accept keeps them and brings the host mirrors up with
// the same expressions the kernel ran.
extern "C" int mpmc_trial_volume_begin(mpmc_ctx *c, double s) {
	if (!c) return MPMC_ERR_ARG;
	if (!c->atoms_set || !c->box_set || !c->cache_valid) return fail(c, MPMC_ERR_ARG, "mpmc_trial_volume_begin: no accepted configuration (call mpmc_energy first)");
	if (c->trial.open) return fail(c, MPMC_ERR_ARG, "mpmc_trial_volume_begin: a trial move is already open (accept or reject it first)");
	if (c->h_mass.empty()) return fail(c, MPMC_ERR_ARG, "mpmc_trial_volume_begin: mpmc_set_atoms was called without masses");
	if (!std::isfinite(s) || s <= 0.0) return fail(c, MPMC_ERR_INVALID_DATUM, "mpmc_trial_volume_begin: the scale factor must be finite and positive");
	if (c->box_in_has_recip || c->box_in[18] > 0 || c->box_in[19] > 0)
		return fail(c, MPMC_ERR_ARG, "mpmc_trial_volume_begin: the cell was set with a caller-supplied reciprocal, volume or cutoff (there is no rule for scaling an override)");
	double basis[9], R[9], vol = 0, cut = 0;
	for (int k = 0; k < 9; k++) basis[k] = c->box.b[k] * s;
	if (mpmc_pbc_compute(basis, R, &vol, &cut) != MPMC_OK || !(vol > 0) || !(cut > 0) || !std::isfinite(vol))
		return fail(c, MPMC_ERR_BOX, "mpmc_trial_volume_begin: the scaled cell has no positive finite volume");
	open_trial(c, 0, 0, c->n);
	TrialState &t = c->trial;
	t.volume = true;
	t.vol_s = s;
	box_from_cell(basis, R, vol, cut, t.vol_box);
	t.noop = (s == 1.0); // (the same cell and the same positions: the trial totals are the accepted totals, nothing is launched)
	return MPMC_OK;
}

// the host's restatement of k_volume_scale over its own mirror: trial positions into pos_new, every molecule's shift into pos_old
static void vol_host_positions(mpmc_ctx *c) {
	TrialState &t = c->trial;
	if (t.vol_host_pos) return;
	const double s = t.vol_s;
	t.pos_new.resize(3 * (size_t)c->n);
	t.pos_old.assign(3 * (size_t)c->n_molecules, 0.0);
	int m = 0;
	for (int i0 = 0; i0 < c->n; m++) {
		int i1 = i0;
		while (i1 + 1 < c->n && c->h_mol[i1 + 1] == c->h_mol[i0]) i1++;
		double cm[3] = {0, 0, 0}, mass = 0;
		for (int i = i0; i <= i1; i++) {
			mass += c->h_mass[i];
			for (int p = 0; p < 3; p++) cm[p] += c->h_mass[i] * c->h_pos[3 * (size_t)i + p];
		}
		for (int p = 0; p < 3; p++) {
			cm[p] /= mass;
			t.pos_old[3 * (size_t)m + p] = cm[p] * s - cm[p];
		}
		for (int i = i0; i <= i1; i++)
			for (int p = 0; p < 3; p++) t.pos_new[3 * (size_t)i + p] = c->h_pos[3 * (size_t)i + p] + t.pos_old[3 * (size_t)m + p];
		i0 = i1 + 1;
	}
	t.vol_host_pos = true;
}

extern "C" int mpmc_trial_volume_get(mpmc_ctx *c, double basis[9], double reciprocal[9], double *volume, double *cutoff, double *pos) {
	if (!c) return MPMC_ERR_ARG;
	if (!c->trial.open || !c->trial.volume) return fail(c, MPMC_ERR_ARG, "mpmc_trial_volume_get: no volume trial is open");
	const TrialState &t = c->trial;
	if (basis) std::memcpy(basis, t.vol_box.b, 9 * sizeof(double));
	if (reciprocal) std::memcpy(reciprocal, t.vol_box.r, 9 * sizeof(double));
	if (volume) *volume = t.vol_box.volume;
	if (cutoff) *cutoff = t.vol_box.cutoff;
	if (pos) {
		if (!t.noop) vol_host_positions(c);
		std::memcpy(pos, t.noop ? c->h_pos.data() : t.pos_new.data(), 3 * (size_t)c->n * sizeof(double));
	}
	return MPMC_OK;
}

extern "C" int mpmc_debug_volume_trial_counts(mpmc_ctx *c, long long *out4) {
	if (!c || !out4) return -1;
	for (int k = 0; k < 4; k++) out4[k] = c->kept.n_vol[k];
	return 0;
}

// diagnostics only: the positions RESIDENT on the device, in original atom order -- the trial's while an evaluated volume trial is open.
// A blocking copy behind everything enqueued on the context's stream.
extern "C" int mpmc_debug_device_positions(mpmc_ctx *c, double *pos) {
	if (!c || !pos) return MPMC_ERR_ARG;
	if (!c->atoms_set || c->atoms_dirty || !c->d_xyzq) return fail(c, MPMC_ERR_ARG, "mpmc_debug_device_positions: the atom list is not on the device");
	HIP_TRY(c, hipSetDevice(c->device));
	std::vector<double4> tmp((size_t)c->n_pad);
	HIP_TRY(c, hipMemcpyAsync(tmp.data(), c->d_xyzq, tmp.size() * sizeof(double4), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	for (int i = 0; i < c->n; i++) {
		const double4 &v = tmp[(size_t)c->slot_of[i]];
		pos[3 * (size_t)i] = v.x, pos[3 * (size_t)i + 1] = v.y, pos[3 * (size_t)i + 2] = v.z;
	}
	return MPMC_OK;
}

// the buffers of a volume trial, and the masses and molecule boundaries of the current atom list on the device
static int vol_ensure(mpmc_ctx *c) {
	int rc;
	if ((rc = c->d_vol_xyzq.reserve(c, (size_t)c->max_pad)) != MPMC_OK) return rc;
	if ((rc = c->d_sf_trial.reserve(c, (size_t)c->K)) != MPMC_OK) return rc;
	if (c->vol_list_gen != c->list_gen) { // (once per atom list: mpmc_set_atoms, an accepted exchange)
		std::vector<int> first;
		first.reserve((size_t)c->n_molecules + 1);
		c->vol_zero_mass = false;
		double mass = 0;
		for (int i = 0; i < c->n; i++) {
			if (i == 0 || c->h_mol[i] != c->h_mol[i - 1]) {
				if (i > 0 && !(mass > 0.0 && std::isfinite(mass))) c->vol_zero_mass = true;
				first.push_back(i);
				mass = 0;
			}
			mass += c->h_mass[i];
		}
		if (!(mass > 0.0 && std::isfinite(mass))) c->vol_zero_mass = true;
		first.push_back(c->n);
		if ((rc = c->d_vol_mass.reserve(c, (size_t)c->n, (size_t)c->max_atoms)) != MPMC_OK) return rc;
		if ((rc = c->d_vol_first.reserve(c, first.size(), (size_t)c->max_atoms + 1)) != MPMC_OK) return rc;
		HIP_TRY(c, hipMemcpyAsync(c->d_vol_mass, c->h_mass.data(), (size_t)c->n * sizeof(double), hipMemcpyHostToDevice, c->stream));
		HIP_TRY(c, hipMemcpyAsync(c->d_vol_first, first.data(), first.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
		HIP_TRY(c, hipStreamSynchronize(c->stream)); // (pageable sources; `first` dies here)
		c->vol_list_gen = c->list_gen;
	}
	if (c->vol_zero_mass) return fail(c, MPMC_ERR_INVALID_DATUM, "mpmc_trial_energy: a molecule without mass has no centre of mass to scale");
	return MPMC_OK;
}

// the accepted and the alternate device state trade places (both ways: the same three swaps and the position pointer)
static void vol_swap_device(mpmc_ctx *c, bool to_trial) {
	std::swap(c->d_sf, c->d_sf_trial); // (each buffer with its own capacity)
	std::swap(c->d_kvec, c->d_vol_kvec);
	std::swap(c->d_kw, c->d_vol_kw);
	std::swap(c->d_w_en, c->d_vol_w_en);
	if (to_trial) c->d_xyzq_acc = c->d_xyzq, c->d_xyzq = c->d_vol_xyzq;
	else c->d_xyzq = c->d_xyzq_acc;
}

// the accepted configuration is the resident one again, on the device and on the host, without an evaluation
static void vol_restore(mpmc_ctx *c) {
	TrialState &t = c->trial;
	if (!t.vol_swapped) return;
	vol_swap_device(c, false);
	c->box = t.vol_acc_box;
	c->ewald_alpha = t.vol_acc_alpha[0];
	c->polar_ewald_alpha = t.vol_acc_alpha[1];
	for (int k = 0; k < 3; k++) c->h_static[k] = t.vol_acc_static[k];
	c->static_dirty = t.vol_acc_static_dirty;
	c->k_dirty = false; // (the accepted cell's tables are back in place)
	// what was made for the trial cell (the rd_crystal image table, a ranked view) is stale again; what was made for the accepted cell and
	// not touched meanwhile (the host sums of the exchange trials, a cavity grid) is valid again
	c->static_gen++;
	if (c->xs_gen == t.vol_acc_gen) c->xs_gen = c->static_gen;
	if (c->cav_static_gen == t.vol_acc_gen) c->cav_static_gen = c->static_gen;
	t.vol_swapped = false;
}

// a call that replaces the cell, the options, the atom list or positions while a volume trial is open closes it first: the accepted state
// goes back into place (the caller's call then drops the accepted totals as it always does)
void mpmc::vol_abandon(mpmc_ctx *c) {
	if (!c->trial.open || !c->trial.volume) return;
	if (c->trial.enqueued) { // enqueued and never waited for: drain it first, as mpmc_trial_reject does (the evaluation holds `pending` and the scalar block)
		mpmc_result drop;
		(void)mpmc_trial_energy_wait(c, &drop); // (a wait that fails leaves the context idle all the same: wait_and_fill)
	}
	vol_restore(c);
	c->e_real_valid = false; // (as in vol_reject: field, store and dipoles are the abandoned cell's, whether or not the caller's call then goes through)
	c->trial.open = c->trial.volume = c->trial.enqueued = false;
}

static int vol_energy_async(mpmc_ctx *c) {
	TrialState &t = c->trial;
	drop_pending_dipoles(c);
	int rc = prepare(c); // (the pending upload behind an accepted exchange: the kernel below reads the accepted positions in their slots)
	if (rc != MPMC_OK) return rc;
	if ((rc = vol_ensure(c)) != MPMC_OK) return rc;
	{
		ProfScope p(c, MPMC_K_CLASSES); // (geometry in front of the evaluation, like the tile bounds)
		launch_volume_scale(c->stream, c->d_xyzq, c->d_slot_of, c->d_vol_mass, c->d_vol_first, c->n_molecules, c->n, c->n_pad, t.vol_s, c->d_vol_xyzq);
	}
	HIP_TRY(c, hipGetLastError());
	t.vol_acc_box = c->box;
	t.vol_acc_alpha[0] = c->ewald_alpha, t.vol_acc_alpha[1] = c->polar_ewald_alpha;
	for (int k = 0; k < 3; k++) t.vol_acc_static[k] = c->h_static[k];
	t.vol_acc_static_dirty = c->static_dirty;
	t.vol_acc_gen = c->static_gen;
	vol_swap_device(c, true);
	c->box = t.vol_box;
	c->k_dirty = true;      // (prepare: the alphas follow the new cutoff, the k tables are built into the alternates)
	c->static_dirty = true; // (the position-independent terms ride along with the evaluation)
	c->static_gen++;
	t.vol_swapped = true;
	if ((rc = enqueue(c, full_mask(c), false, /*volume_trial*/ true)) != MPMC_OK) {
		vol_restore(c);
		return rc;
	}
	t.was_full = true;
	t.polar_delta = t.inline_move = false;
	c->trial_last_kind = 1;
	t.enqueued = true;
	c->kept.n_vol[0]++;
	return MPMC_OK;
}

static int vol_accept(mpmc_ctx *c) {
	TrialState &t = c->trial;
	HIP_TRY(c, hipSetDevice(c->device));
	const size_t n = (size_t)c->n;
	// the device: the trial positions go into the atom block (stream-ordered behind the evaluation; 32 bytes per atom), the cell, the k
	// tables and the structure factors stay where the evaluation left them
	HIP_TRY(c, hipMemcpyAsync(c->d_xyzq_acc, c->d_vol_xyzq, (size_t)c->n_pad * sizeof(double4), hipMemcpyDeviceToDevice, c->stream));
	c->d_xyzq = c->d_xyzq_acc;
	t.vol_swapped = false;
	// the host: the same expressions over its own mirrors, no copy back
	vol_host_positions(c);
	if (c->h_pos_sorted.size() == 3 * n) // (where every atom stood at the last sort, in the new cell: the drift check measures from there)
		for (int i = 0, m = 0; i < c->n; i++) {
			if (i > 0 && c->h_mol[i] != c->h_mol[i - 1]) m++;
			for (int p = 0; p < 3; p++) c->h_pos_sorted[3 * (size_t)i + p] += t.pos_old[3 * (size_t)m + p];
		}
	c->h_pos.swap(t.pos_new);
	c->pos_gen++;
	const int rc_g = mirror_guard(c);
	if (rc_g != MPMC_OK) return rc_g;
	if (!c->atoms_dirty)
		for (int i = 0; i < c->n; i++) {
			double4 &v = c->h_xyzq[c->slot_of[i]];
			v.x = c->h_pos[3 * (size_t)i], v.y = c->h_pos[3 * (size_t)i + 1], v.z = c->h_pos[3 * (size_t)i + 2];
		}
	std::memset(c->box_in, 0, sizeof(c->box_in)); // (what mpmc_set_box(basis, NULL, 0, 0) of the new cell would have left)
	std::memcpy(c->box_in, t.vol_box.b, 9 * sizeof(double));
	c->box_in_has_recip = false;
	c->accepted = t.totals;
	c->accepted.frozen_pairs = -1;
	c->cache_valid = true;
	t.open = t.volume = false;
	c->kept.n_vol[1]++;
	return MPMC_OK;
}

static int vol_reject(mpmc_ctx *c) {
	TrialState &t = c->trial;
	t.open = t.volume = false;
	if (!t.vol_swapped) return MPMC_OK; // (never enqueued, or s == 1)
	vol_restore(c);
	c->cache_valid = true;   // (the accepted record, which the trial never touched, describes the configuration that is back)
	c->e_real_valid = false; // (field, store and dipoles are the rejected configuration's: the next polarizable trial evaluates in full)
	c->kept.n_vol[2]++;
	return MPMC_OK;
}

// the two halves of mpmc_trial_energy: everything up to the last enqueue, then the wait + host arithmetic (P images of a
// path-integral move overlap on the device when a driver enqueues all of them before the first wait)
extern "C" int mpmc_trial_energy_async(mpmc_ctx *c) {
	if (!c) return MPMC_ERR_ARG;
	if (!c->trial.open) return fail(c, MPMC_ERR_ARG, "mpmc_trial_energy: no trial move is open");
	if (c->trial.enqueued) return fail(c, MPMC_ERR_ARG, "mpmc_trial_energy_async: already enqueued");
	if (c->trial.noop) {
		c->trial.was_full = false;
		c->trial.enqueued = true;
		return MPMC_OK;
	}
	if (c->trial.volume) return vol_energy_async(c);
	if (c->trial.xch_kind) return xch_energy_async(c);
	const mpmc_options &o = c->opts;
	const bool polar = o.polarization && !o.rd_only;
	const int m = c->trial.count;
	c->trial.polar_delta = false;
	const bool no_polar_delta = c->kept.tune.no_polar_delta;
	// (Wolf electrostatics and the Feynman-Hibbs corrections are per-pair terms like the others: the delta kernels carry them; a
	// polarizable box under Wolf keeps the full evaluation -- its static field is the Ewald one, outside the reference's own combinations;
	// so does a box whose dipoles are solved directly, polar_iterative off: the matrix is rebuilt and factored again anyway)
	// (... and a box under `polar_ewald_full`: every pass reads every dipole; and one under `polar_gs_ranked`: a move changes the ranks)
	const bool polar_delta = polar && c->e_real_valid && !no_polar_delta && m <= MPMC_TRIAL_MAX_ATOMS && !o.wolf && !direct_solve(c) && !ewald_full_on(c) && !gs_ranked_on(c);
	if ((polar && !polar_delta) || m > MPMC_TRIAL_MAX_ATOMS) {
		// the dipole solve couples every atom: evaluate the trial configuration in full (still on the device)
		int rc = mpmc_update_positions(c, c->trial.first, m, c->trial.pos_new.data());
		if (rc != MPMC_OK) return rc;
		if ((rc = enqueue(c, full_mask(c))) != MPMC_OK) return rc; // (eager: an accepted trial's dipoles are its caller's at once)
		c->trial.was_full = true;
		c->trial_last_kind = 1;
		c->trial.enqueued = true;
		return MPMC_OK;
	}
	drop_pending_dipoles(c); // (the delta path swaps positions and rewrites the field and the store under an open on-demand solve)
	int rc = prepare(c);
	if (rc != MPMC_OK) return rc;
	if ((rc = ensure_trial_buffers(c)) != MPMC_OK) return rc;
	hipStream_t st = c->stream;
	// short moves of non-polarizable boxes travel in the kernel arguments: no staging copy (a trial is launch-bound on the host: every
	// call saved is ~5 us of a ~25 us move).  The polarizable path keeps the device lists (its field / store kernels read them).
	const bool no_inline = c->kept.tune.no_inline_move;
	// (the three-body, disp-expansion, rd_crystal, rd-model and contact deltas read the moved atoms from the device lists: a box with one of them always stages its move)
	c->trial.inline_move = !polar_delta && m <= kMvInline && !no_inline && !c->kept.tb_enabled && !c->kept.de_enabled && !crystal_on(c) && !rd_model_on(c) && !sg_on(c) && !contact_on(c);
	if (c->trial.inline_move) {
		for (int t = 0; t < m; t++) {
			const int i = c->trial.first + t;
			c->mv_inline.orig[t] = i;
			c->mv_inline.slot[t] = c->slot_of[i];
			for (int d = 0; d < 3; d++) c->mv_inline.nw[t][d] = c->trial.pos_new[3 * t + d];
			c->mv_inline.nw[t][3] = c->h_q[i];
		}
		for (int t = m; t < kMvInline; t++) { // (unused entries: defined values, never selected)
			c->mv_inline.orig[t] = c->mv_inline.slot[t] = 0;
			for (int d = 0; d < 4; d++) c->mv_inline.nw[t][d] = 0.0;
		}
	} else { // one pinned staging record, one host-to-device copy
		double4 *nw = reinterpret_cast<double4 *>(c->h_mv_blob.p);
		int *slots = reinterpret_cast<int *>(c->h_mv_blob + MPMC_TRIAL_MAX_ATOMS * sizeof(double4));
		int *origs = slots + MPMC_TRIAL_MAX_ATOMS;
		for (int t = 0; t < m; t++) {
			const int i = c->trial.first + t;
			origs[t] = i;
			slots[t] = c->slot_of[i];
			nw[t] = make_double4(c->trial.pos_new[3 * t], c->trial.pos_new[3 * t + 1], c->trial.pos_new[3 * t + 2], c->h_q[i]);
		}
		HIP_TRY(c, hipMemcpyAsync(c->d_mv_blob, c->h_mv_blob, kMvBlobBytes, hipMemcpyHostToDevice, st));
	}
	const int do_es = o.rd_only ? 0 : 1;
	if (c->kept.tb_enabled) {
		// Axilrod-Teller: the change of the triples with a moved atom, O(m N^2), with the accepted positions still resident; its sum lands in
		// D_THREE_BODY of the delta result block, which k_delta_finish copies out with the launch number it posts
		if ((rc = three_body_ready(c)) != MPMC_OK) return rc;
		ProfScope p(c, MPMC_K_THREE_BODY);
		launch_three_body_delta(st, atoms_view(c), c->d_tb_au, c->box, kThreeBodyScale, c->d_mv_slot, c->d_mv_new, m, c->d_moved_idx, c->d_tb_part,
		                        c->d_delta_out + D_THREE_BODY);
	}
	if (c->kept.de_enabled) {
		// disp-expansion: the change of the pairs with a moved atom, O(m N), old positions still resident; into D_DISP of the delta result
		// block.  It replaces the LJ delta of launch_delta.
		if ((rc = disp_ready(c)) != MPMC_OK) return rc;
		ProfScope p(c, MPMC_K_PAIR);
		launch_disp_expansion_delta(st, atoms_view(c), c->d_de_co, c->d_de_t10, c->box, disp_params(c), c->d_mv_slot, c->d_mv_new, m, c->d_moved_idx,
		                            c->d_de_part, c->d_delta_out + D_DISP);
	}
	if (crystal_on(c)) {
		// rd_crystal: the change of the lattice sums of the pairs with a moved atom, O(m N images), old positions still resident; into D_RD
		// and D_RD_TERMS of the delta result block.  It replaces the LJ delta of launch_delta.
		if ((rc = crystal_ready(c)) != MPMC_OK) return rc;
		ProfScope p(c, MPMC_K_PAIR);
		launch_crystal_delta(st, atoms_view(c), c->box, crystal_params(c), c->d_rc_shift, c->d_mv_slot, c->d_mv_new, m, c->d_moved_idx, c->d_rc_part,
		                     c->d_delta_out + D_RD);
	}
	if (rd_model_on(c)) {
		// the rd model: the change of the pairs with a moved atom, O(m N), old positions still resident; into D_RD and D_RD_TERMS of the
		// delta result block, which a context with the model never shares with rd_crystal (crystal_on, rd_model_ready).  It
		// replaces the LJ delta of launch_delta; the cached pair correction does not move with the atoms.
		if ((rc = rd_model_ready(c)) != MPMC_OK) return rc;
		ProfScope p(c, MPMC_K_PAIR);
		launch_rd_model_delta(st, atoms_view(c), c->d_rdm_sp, c->box, rd_model_params(c), c->d_mv_slot, c->d_mv_new, m, c->d_moved_idx, c->d_rdm_part,
		                      c->d_delta_out + D_RD);
	}
	if (sg_on(c)) {
		// Silvera-Goldman: the change of the pairs with a moved atom, O(m N), old positions still resident; into D_RD and D_RD_TERMS of the
		// delta result block (no model and no rd_crystal sum beside it: sg_ready, crystal_on).  It replaces the LJ delta of launch_delta,
		// which runs without electrostatics here (no structure-factor update) and posts the block.
		if ((rc = sg_ready(c)) != MPMC_OK) return rc;
		ProfScope p(c, MPMC_K_PAIR);
		launch_sg_delta(st, atoms_view(c), c->d_perm, c->box, sg_params(c), c->d_mv_slot, c->d_mv_new, m, c->d_moved_idx, c->d_sg_part, c->d_delta_out + D_RD);
	}
	if (contact_on(c)) {
		// cavity_autoreject: the change of the contact counts of the pairs with a moved atom, O(m N), old positions still resident; into
		// D_CA_REPLACED and D_CA_ABSOLUTE of the delta result block, which k_delta_finish posts with everything else
		if ((rc = contact_ready(c)) != MPMC_OK) return rc;
		ProfScope p(c, MPMC_K_PAIR);
		launch_contact_delta(st, atoms_view(c), c->kept.de_enabled ? c->d_de_co.p : c->d_rdm_sp.p, c->box, contact_params(c), c->d_mv_slot, c->d_mv_new, m,
		                     c->d_moved_idx, c->d_ca_part, c->d_delta_out + D_CA_REPLACED);
	}
	{
		FusedParams fp{};
		fp.ewald_alpha = c->ewald_alpha;
		ext_params(c, fp, o.wolf && do_es);
		ProfScope p(c, MPMC_K_PAIR);
		launch_delta(st, atoms_view(c), c->d_slot_of, c->box, recip_view(c), fp, do_es, c->d_mv_slot, c->d_mv_orig, c->d_mv_new, m,
		             c->d_moved_idx, c->d_sf_trial, c->d_block_part, c->d_block_cnt, c->d_delta_out, c->d_delta_cnt, c->h_delta_out,
		             (c->trial_seq += 1.0), c->trial.inline_move ? &c->mv_inline : nullptr);
	}
	HIP_TRY(c, hipGetLastError()); // (k_delta_finish posts the result into h_delta_out itself)
	c->trial.was_full = false;
	c->trial_last_kind = 0;
	if (polar_delta) {
		// Polarizable box: the pair energies and structure factors above are O(m N); the static field follows the same way -- real part:
		// delta of the pairs with a moved atom; reciprocal part: recomputed from the trial structure factors (O(K N), 30 us at 10 000
		// atoms) -- then the tensor store is rebuilt for the trial geometry (store-only sweep of the near tile pairs) and the dipoles are
		// solved from alpha E0 exactly as in a full evaluation (thole_iterative restarts every call, :3547-3560).  What is saved: the
		// energy / erfc / field arithmetic of the N^2/2 pair sweep and the O(K N) structure factors.
		// (room for the longest move at this tile count: a longer move of the same box does not allocate again)
		if ((rc = c->d_dk_part.reserve(c, (size_t)c->n_tiles * (size_t)m * 3, (size_t)c->n_tiles * MPMC_TRIAL_MAX_ATOMS * 3)) != MPMC_OK) return rc;
		const AtomsDev at = atoms_view(c);
		{
			ProfScope p(c, MPMC_K_FIELD);
			if (wolf_field_on(c)) // (`polar_wolf`: the same O(m N) difference of thole_field_wolf's pair sum)
				launch_wolf_field_delta(st, at, c->box, wolf_field_params(c->kept.pw_alpha, c->box.cutoff), c->d_mv_slot, c->d_mv_new, m, c->d_moved_idx, c->d_e_real,
				                        c->d_e_real_trial, c->d_dk_part);
			else
				launch_delta_field(st, at, c->box, c->polar_ewald_alpha, o.polar_ewald, c->d_mv_slot, c->d_mv_new, m, c->d_moved_idx, c->d_e_real,
				                   c->d_e_real_trial, c->d_dk_part);
			// from here on the resident positions are the TRIAL ones (the old ones wait in d_mv_new: reject swaps them back)
			launch_swap_positions(st, c->d_xyzq, c->d_mv_slot, c->d_mv_new, m);
			if (o.polar_ewald) {
				RecipDev rt = recip_view(c);
				rt.sf = c->d_sf_trial;
				launch_field_recip(st, at, c->box, rt, o.ewald_kmax, c->d_e_recip_part);
			}
			c->mu_cur = 0;
			if (polar_moments_apply(c) && (rc = reserve_dk_ring(c)) != MPMC_OK) return rc;
			launch_field_finalize(st, at, c->box, o.polar_ewald, c->d_e_recip_part, c->d_e_real_trial, 1, start_gamma(c), c->d_e_static, c->d_mu[0], nullptr,
			                      polar_moments_apply(c) ? c->d_dk_ring.p : nullptr);
		}
		HIP_TRY(c, hipGetLastError());
		c->trial.polar_delta = true;
		if (zodid_on(c)) { // `polar_zodid`: the dipoles are the start vector just written: no classes, no store, no iteration -- the reduction closes the move
			if ((rc = enqueue(c, RUN_SOLVE)) != MPMC_OK) return rc;
			c->trial.enqueued = true;
			return MPMC_OK;
		}
		// the store-only sweep rebuilds the tile pairs of the tiles the moved atoms live in, and of the tiles a rejected trial left behind:
		// no other tile pair's geometry (or class) changed
		c->trial_tiles.clear();
		for (int t = 0; t < m; t++) {
			const int tile = c->slot_of[c->trial.first + t] / kTile;
			if (std::find(c->trial_tiles.begin(), c->trial_tiles.end(), tile) == c->trial_tiles.end()) c->trial_tiles.push_back(tile);
		}
		std::vector<int> touch = c->trial_tiles;
		for (int tile : c->store_dirty_tiles)
			if (std::find(touch.begin(), touch.end(), tile) == touch.end()) touch.push_back(tile);
		c->touch_n = (touch.size() <= 8) ? (int)touch.size() : -1;
		for (int k = 0; k < c->touch_n; k++) c->touch[k] = touch[k];
		rc = enqueue(c, RUN_STORE | RUN_SOLVE); // classes + store of the trial geometry, the iterations, -1/2 mu.E0
		c->touch_n = -1;
		if (rc != MPMC_OK) return rc;
		c->store_dirty_tiles = c->trial_tiles; // until accepted: these tiles hold the TRIAL geometry's tensors
	}
	c->trial.enqueued = true;
	return MPMC_OK;
}

extern "C" int mpmc_trial_energy_wait(mpmc_ctx *c, mpmc_result *out) {
	if (!c || !out) return MPMC_ERR_ARG;
	if (!c->trial.open || !c->trial.enqueued) return fail(c, MPMC_ERR_ARG, "mpmc_trial_energy_wait: nothing enqueued");
	c->trial.enqueued = false;
	ConfigTotals &tr = c->trial.totals;
	if (c->trial.noop) {
		tr = c->accepted;
		c->trial.evaluated = true;
		*out = tr.res;
		contact_deliver(c, out, tr);
		return MPMC_OK;
	}
	if (c->trial.was_full) {
		int rc = wait_and_fill(c, out); // (the unpenalised result: what leaves is penalised below)
		if (rc != MPMC_OK) return rc;
		// the evaluation's record is the TRIAL's; the accepted one stays until mpmc_trial_accept.  The update of the positions or of the atom
		// list in front of the evaluation cleared cache_valid: the accepted record still holds, and from here on the flag says so again
		tr = c->eval;
		c->cache_valid = true;
		contact_deliver(c, out, tr);
		c->trial.evaluated = true;
		return MPMC_OK;
	}
	HIP_TRY(c, hipSetDevice(c->device));
	mpmc_result solved{};
	if (c->trial.polar_delta) { // the solve half went through enqueue(): its scalars (polarization energy, rrms, iterations) arrive the usual way
		int rc = wait_and_fill(c, &solved);
		if (rc != MPMC_OK) return rc;
	} else {
		// the finish kernel posts its launch number behind the result: poll for it (a trial is a few tens of microseconds; the stream
		// synchronisation alone costs 10-15); with profiling events outstanding, or past the budget, wait the ordinary way
		bool seen = false;
		if (c->ev_used.empty()) {
			volatile const double *flag = c->h_delta_out + kDeltaHostSeq;
			const double want = c->trial_seq;
			seen = poll_posted(c, [&] { return *flag == want; }, std::chrono::microseconds(1000));
		}
		if (!seen) {
			c->kept.n_stream_syncs++;
			HIP_TRY(c, hipStreamSynchronize(c->stream));
		}
		prof_harvest(c);
	}
	// the delta paths: the trial record is the accepted one plus what the device posted (the D_* slots at delta_host_index)
	const ConfigTotals &acc = c->accepted;
	const double *dh = c->h_delta_out.p;
	tr = acc;
	if (contact_on(c)) { // (cavity_autoreject: the accepted counts plus the signed change of the moved atoms' or the molecule's pairs)
		tr.ca.replaced = acc.ca.replaced + (int64_t)dh[delta_host_index(D_CA_REPLACED)];
		tr.ca.absolute = acc.ca.absolute + (int64_t)dh[delta_host_index(D_CA_ABSOLUTE)];
	}
	if (c->trial.xch_kind) {
		xch_result(c, tr.res);
		if (contact_on(c)) { // (the unmeasured frozen pairs of the trial composition, from the host's counts of the accepted list: contact_ready)
			int64_t fm = 0;
			for (int k = 0; k < c->trial.count; k++) fm += c->trial.xch_mol.frozen[k] ? 1 : 0;
			tr.frozen_pairs = c->ca_frozen_pairs + (c->trial.xch_kind > 0 ? fm * c->ca_frozen_atoms : -fm * (c->ca_frozen_atoms - fm));
		}
		c->trial.evaluated = true;
		*out = tr.res;
		contact_deliver(c, out, tr);
		return MPMC_OK;
	}
	const int do_es = c->opts.rd_only ? 0 : 1;
	const mpmc_result &a = acc.res;
	mpmc_result &r = tr.res;
	r.lj_pairs = a.lj_pairs + (c->kept.de_enabled ? dh[delta_host_index(D_DISP)] : dh[delta_host_index(D_LJ)]); // (with the disp-expansion term lj_pairs holds its pair sum)
	if (crystal_on(c)) { // (lj_pairs holds the lattice sum; crystal_self and the corrections do not move with the atoms)
		r.lj_pairs = a.lj_pairs + dh[delta_host_index(D_RD)];
		tr.rc_terms = acc.rc_terms + (int64_t)dh[delta_host_index(D_RD_TERMS)];
		c->rc_info.n_image_terms = tr.rc_terms;
	}
	if (rd_model_on(c)) { // (lj_pairs holds the model's sum; the corrections do not move with the atoms)
		r.lj_pairs = a.lj_pairs + dh[delta_host_index(D_RD)];
		tr.rdm_terms = acc.rdm_terms + (int64_t)dh[delta_host_index(D_RD_TERMS)];
		c->rdm_info.n_terms = tr.rdm_terms;
	}
	if (sg_on(c)) { // (lj_pairs holds sg()'s sum; n_lj_in_cutoff stays 0 under the term)
		r.lj_pairs = a.lj_pairs + dh[delta_host_index(D_RD)];
		tr.sg_terms = acc.sg_terms + (int64_t)dh[delta_host_index(D_RD_TERMS)];
		c->sg_info.n_terms = tr.sg_terms;
	}
	r.n_lj_in_cutoff = sg_on(c) ? 0 : a.n_lj_in_cutoff + c->h_delta_cnt[0];
	if (do_es) {
		r.es_real = a.es_real + (dh[delta_host_index(D_ES_REAL)] - dh[delta_host_index(D_ES_INTRA)]);
		r.es_recip = dh[delta_host_index(D_ES_RECIP)];
		r.coulombic_energy = (r.es_real + r.es_recip) + r.es_self;
		r.n_es_in_cutoff = a.n_es_in_cutoff + c->h_delta_cnt[1];
	}
	if (c->trial.polar_delta) {
		r.polarization_energy = solved.polarization_energy;
		r.dipole_rrms = solved.dipole_rrms;
		r.polar_iterations = solved.polar_iterations;
		r.iterator_failed = solved.iterator_failed;
	}
	if (c->kept.tb_enabled) r.three_body_energy = a.three_body_energy + dh[delta_host_index(D_THREE_BODY)];
	compose_totals(c, rd_form_of(c), &r);
	c->trial.evaluated = true;
	*out = r;
	contact_deliver(c, out, tr);
	return MPMC_OK;
}

extern "C" int mpmc_trial_energy(mpmc_ctx *c, mpmc_result *out) {
	if (!c || !out) return MPMC_ERR_ARG;
	int rc = mpmc_trial_energy_async(c);
	if (rc != MPMC_OK) return rc;
	return mpmc_trial_energy_wait(c, out);
}

extern "C" int mpmc_trial_accept(mpmc_ctx *c) {
	if (!c) return MPMC_ERR_ARG;
	if (!c->trial.open || !c->trial.evaluated) return fail(c, MPMC_ERR_ARG, "mpmc_trial_accept: no evaluated trial move");
	HIP_TRY(c, hipSetDevice(c->device));
	const int m = c->trial.count;
	if (c->trial.noop) {
		c->trial.open = false;
		return MPMC_OK;
	}
	if (c->trial.volume) return vol_accept(c);
	if (c->trial.xch_kind) { // an exchange: the full evaluation left the trial list resident; the delta path edits the list now
		if (!c->trial.was_full) {
			const int rc_x = xch_accept_delta(c);
			if (rc_x != MPMC_OK) return rc_x;
		}
		c->trial.xch_saved.clear();
		c->trial.xch_kind = 0;
	} else if (!c->trial.was_full) {
		if (c->trial.polar_delta) { // the trial positions are already resident; the trial real-space field becomes the accepted one
			std::swap(c->d_e_real, c->d_e_real_trial);
			c->store_dirty_tiles.clear(); // ... and so is the store
		} else {
			if (c->trial.inline_move) launch_commit_positions_inline(c->stream, c->d_xyzq, c->mv_inline, m);
			else launch_commit_positions(c->stream, c->d_xyzq, c->d_mv_slot, c->d_mv_new, m);
		}
		HIP_TRY(c, hipGetLastError());
		std::swap(c->d_sf, c->d_sf_trial); // the trial structure factors become the accepted ones (each buffer with its own capacity)
		// (no wait: whatever comes next on this context is enqueued behind the commit on the same stream, and the host mirrors below are
		// the host's own -- the stream synchronisation that stood here cost 13 us of a 41 us accepted move)
		for (int t = 0; t < 3 * m; t++) c->h_pos[3 * (size_t)c->trial.first + t] = c->trial.pos_new[t];
		c->pos_gen++;
		{
			const int rc_g = mirror_guard(c);
			if (rc_g != MPMC_OK) return rc_g;
		}
		for (int t = 0; t < m; t++) { // the slot-ordered mirror follows (a later position update uploads it as a whole)
			double4 &v = c->h_xyzq[c->slot_of[c->trial.first + t]];
			v.x = c->trial.pos_new[3 * t], v.y = c->trial.pos_new[3 * t + 1], v.z = c->trial.pos_new[3 * t + 2];
		}
	}
	// the trial becomes the accepted configuration, whichever way it was evaluated.  (The whole record: a count whose term is off is read by
	// nobody until the term is switched on, which drops cache_valid and this record with it.  Its frozen pairs are the resident list's own.)
	c->accepted = c->trial.totals;
	c->accepted.frozen_pairs = -1;
	c->cache_valid = true;
	c->trial.open = false;
	c->trial.polar_delta = false;
	return MPMC_OK;
}

// behind a rejected full-evaluation trial, once the accepted configuration is resident again
static int rebase_after_restore(mpmc_ctx *c) {
	c->cache_valid = true;   // (the accepted record, which the trial never touched, describes the configuration that is back)
	c->e_real_valid = false; // (the real-space field on the device is the rejected configuration's: the next polarizable trial evaluates in full)
	if ((c->opts.polarization && !c->opts.rd_only) || c->opts.wolf) return MPMC_OK;
	mpmc_result tmp; // the resident structure factors are the trial ones: re-base on the restored configuration
	return mpmc_energy(c, &tmp);
}

extern "C" int mpmc_trial_reject(mpmc_ctx *c) {
	if (!c) return MPMC_ERR_ARG;
	if (!c->trial.open) return fail(c, MPMC_ERR_ARG, "mpmc_trial_reject: no trial move is open");
	if (c->trial.enqueued) { // enqueued but never waited for: drain it first
		mpmc_result drop;
		int rc = mpmc_trial_energy_wait(c, &drop);
		if (rc != MPMC_OK) return rc;
	}
	if (c->trial.volume) return vol_reject(c);
	if (c->trial.xch_kind) { // an exchange: the delta path left nothing behind; after a full evaluation the accepted list goes back
		const bool restore = c->trial.xch_saved.size() > 0;
		int rc = MPMC_OK;
		if (restore) {
			AtomRun acc = std::move(c->trial.xch_saved);
			rc = xch_replace_list(c, acc, AtomRun{});
		}
		c->trial.xch_kind = 0;
		c->trial.open = false;
		return (restore && rc == MPMC_OK) ? rebase_after_restore(c) : rc;
	}
	c->trial.open = false;
	if (c->trial.polar_delta) { // (enqueued or evaluated) the device holds the trial positions: swap the accepted ones back
		HIP_TRY(c, hipSetDevice(c->device));
		launch_swap_positions(c->stream, c->d_xyzq, c->d_mv_slot, c->d_mv_new, c->trial.count);
		HIP_TRY(c, hipGetLastError()); // (stream-ordered in front of whatever comes next: nothing to wait for)
		c->trial.polar_delta = false;
		return MPMC_OK; // (the store, classes and dipoles describe the rejected geometry; the next trial or energy() rebuilds them)
	}
	if (c->trial.evaluated && c->trial.was_full) { // the resident configuration is the trial one: put the old positions back
		const int rc = mpmc_update_positions(c, c->trial.first, c->trial.count, c->trial.pos_old.data());
		return rc != MPMC_OK ? rc : rebase_after_restore(c);
	}
	return MPMC_OK;
}

// ---- batched insertion candidates: n_cand poses of one molecule against the accepted configuration, one launch chain, one wait -------------
// out[c] is what mpmc_trial_insert_begin(pose c) + mpmc_trial_energy + mpmc_trial_reject would give, bit for bit: the device runs the block
// roles of k_exchange_all and the reduction of k_delta_finish per candidate (kernels_insert_batch.hip), the host ends in xch_compose like
// xch_result.  No trial is opened and nothing an evaluation, a trial or a cavity update reads is written: the accepted totals, the
// structure factors, the atom list.  (The host sums of the ACCEPTED list, xs_acc, are made where they are stale, as a trial makes them.)
constexpr size_t kInsStageRecords = (size_t)1 << 17; // staged records per pass (8 MiB pinned, as much on the device)

extern "C" int mpmc_insert_candidates(mpmc_ctx *c, int count, int n_cand, const double *pos, const double *charge, const double *polarizability,
                                      const double *epsilon, const double *sigma, const int32_t *frozen, const int32_t *has_disp, const double *mass,
                                      mpmc_result *out) {
	if (!c) return MPMC_ERR_ARG;
	if (count < 1 || n_cand < 1 || n_cand > MPMC_INSERT_MAX_CANDIDATES || !pos || !out || !charge || !polarizability || !epsilon || !sigma || !frozen)
		return fail(c, MPMC_ERR_ARG, "mpmc_insert_candidates: count < 1, n_cand outside [1, MPMC_INSERT_MAX_CANDIDATES] or a null array");
	int rc = xch_begin_checks(c, "mpmc_insert_candidates");
	if (rc != MPMC_OK) return rc;
	const mpmc_options &o = c->opts;
	// only the delta path exists here: a batch of full evaluations is the loop of single trials the caller can already write
	if (o.polarization && !o.rd_only) return fail(c, MPMC_ERR_UNSUPPORTED, "mpmc_insert_candidates: a polarizable box has no insertion delta (use single trials)");
	if (crystal_on(c)) return fail(c, MPMC_ERR_UNSUPPORTED, "mpmc_insert_candidates: rd_crystal has no insertion delta (use single trials)");
	if (rd_model_on(c)) return fail(c, MPMC_ERR_UNSUPPORTED, "mpmc_insert_candidates: a non-default rd model has no insertion delta (use single trials)");
	if (sg_on(c)) return fail(c, MPMC_ERR_UNSUPPORTED, "mpmc_insert_candidates: the Silvera-Goldman term has no insertion delta (use single trials)");
	if (count > MPMC_TRIAL_MAX_ATOMS) return fail(c, MPMC_ERR_UNSUPPORTED, "mpmc_insert_candidates: count > MPMC_TRIAL_MAX_ATOMS (use single trials)");
	if ((rc = xch_molecule_checks(c, "mpmc_insert_candidates", count, n_cand, pos, charge, polarizability, epsilon, sigma, mass)) != MPMC_OK) return rc;
	const int32_t id = xch_largest_mol_id(c);
	if (id == INT32_MAX) return fail(c, MPMC_ERR_ARG, "mpmc_insert_candidates: no molecule id left");
	const int m = count;
	AtomRun mol;
	xch_fill_molecule(c, mol, id + 1, m, pos, charge, polarizability, epsilon, sigma, frozen, has_disp, mass);

	drop_pending_dipoles(c);
	if ((rc = prepare(c)) != MPMC_OK) return rc; // (the pending upload behind an accepted exchange, as a trial makes it)
	// candidates per pass of the staging block: whole launch chains where more than one fits
	size_t pass = std::max<size_t>(1, kInsStageRecords / (size_t)m);
	if (pass > (size_t)kInsBatchChunk) pass -= pass % kInsBatchChunk;
	pass = std::min(pass, (size_t)n_cand);
	const size_t chunk = std::min((size_t)kInsBatchChunk, (size_t)n_cand), nb = (size_t)c->n_tiles + 1;
	const int do_es = o.rd_only ? 0 : 1;
	const bool do_ewald = do_es && !o.wolf;
	if ((rc = c->h_ins_mol.reserve(c, pass * m)) != MPMC_OK) return rc;
	if ((rc = c->d_ins_mol.reserve(c, pass * m)) != MPMC_OK) return rc;
	if ((rc = c->d_ins_sf.reserve(c, do_ewald ? chunk * (size_t)c->K : 1)) != MPMC_OK) return rc;
	if ((rc = c->d_ins_part.reserve(c, chunk * nb * 2)) != MPMC_OK) return rc;
	if ((rc = c->d_ins_cnt.reserve(c, chunk * nb * 2)) != MPMC_OK) return rc;
	if ((rc = c->d_ins_out.reserve(c, (size_t)n_cand)) != MPMC_OK) return rc;
	if ((rc = c->h_ins_out.reserve(c, (size_t)n_cand)) != MPMC_OK) return rc;
	const bool contact = contact_on(c); // cavity_autoreject: per-candidate contacts by a sibling launch in every chain, behind the same wait
	if (contact) {
		if ((rc = contact_ready(c)) != MPMC_OK) return rc;
		if ((rc = c->d_ca_xpart.reserve(c, chunk * (size_t)c->n_tiles * 2)) != MPMC_OK) return rc;
		if ((rc = c->d_ins_ca.reserve(c, 2 * (size_t)n_cand)) != MPMC_OK) return rc;
		if ((rc = c->h_ins_ca.reserve(c, 2 * (size_t)n_cand)) != MPMC_OK) return rc;
	}
	c->ins_ca_n = -1;

	// the species part, once: the same for every pose
	XchSums xs_trial;
	double st3[3], N;
	std::vector<XchAtom> rec((size_t)m);
	xch_species_terms(c, +1, mol, xs_trial, st3, N, rec.data());
	long long d[4];
	xch_pair_counts(c, mol, c->xs_acc.cls, d);

	FusedParams fp{};
	fp.ewald_alpha = c->ewald_alpha;
	ext_params(c, fp, o.wolf && do_es);
	const AtomsDev at = atoms_view(c);
	const RecipDev rv = recip_view(c);
	hipStream_t st = c->stream;
	for (size_t p0 = 0; p0 < (size_t)n_cand; p0 += pass) {
		const size_t p1 = std::min(p0 + pass, (size_t)n_cand);
		if (p0 > 0) { // the staging block is written again: the copies out of it must have been made (long molecules times many candidates only)
			c->kept.n_stream_syncs++;
			HIP_TRY(c, hipStreamSynchronize(st));
		}
		for (size_t q = p0; q < p1; q++) {
			const double *x = pos + 3 * (size_t)m * q;
			XchAtom *g = c->h_ins_mol + (q - p0) * m;
			for (int k = 0; k < m; k++) {
				g[k] = rec[k];
				g[k].xyzq.x = x[3 * k], g[k].xyzq.y = x[3 * k + 1], g[k].xyzq.z = x[3 * k + 2];
			}
		}
		HIP_TRY(c, hipMemcpyAsync(c->d_ins_mol, c->h_ins_mol, (p1 - p0) * m * sizeof(XchAtom), hipMemcpyHostToDevice, st));
		ProfScope ps(c, MPMC_K_PAIR);
		for (size_t q0 = p0; q0 < p1; q0 += kInsBatchChunk) {
			const int nc = (int)std::min((size_t)kInsBatchChunk, p1 - q0);
			launch_insert_batch(st, at, c->box, rv, fp, do_es, c->d_ins_mol + (q0 - p0) * m, m, nc, c->d_ins_sf, c->d_ins_part, c->d_ins_cnt, c->d_ins_out + q0);
			if (contact)
				launch_exchange_contact(st, at, c->box, contact_params(c), c->d_ins_mol + (q0 - p0) * m, m, nc, 1.0, c->d_ca_xpart, nullptr, c->d_ins_ca + 2 * q0);
		}
	}
	HIP_TRY(c, hipGetLastError());
	HIP_TRY(c, hipMemcpyAsync(c->h_ins_out, c->d_ins_out, (size_t)n_cand * sizeof(InsCandOut), hipMemcpyDeviceToHost, st));
	if (contact) HIP_TRY(c, hipMemcpyAsync(c->h_ins_ca, c->d_ins_ca, 2 * (size_t)n_cand * sizeof(long long), hipMemcpyDeviceToHost, st));
	c->kept.n_stream_syncs++;
	HIP_TRY(c, hipStreamSynchronize(st)); // the one wait of the call
	prof_harvest(c);
	for (int q = 0; q < n_cand; q++) xch_compose(c, +1, m, c->h_ins_out[q], st3, N, d, out[q]);
	// (cavity_autoreject: the counts of each candidate's trial composition, and the sigma rule's penalty on out[q] as the single trial delivers it)
	c->ins_ca.assign(2 * (size_t)n_cand, 0);
	for (int q = 0; contact && q < n_cand; q++) {
		c->ins_ca[2 * (size_t)q] = (c->kept.ca_rules & CA_RULE_SIGMA) ? c->accepted.ca.replaced + c->h_ins_ca[2 * (size_t)q] : 0;
		c->ins_ca[2 * (size_t)q + 1] = (c->kept.ca_rules & CA_RULE_ABSOLUTE) ? c->accepted.ca.absolute + c->h_ins_ca[2 * (size_t)q + 1] : 0;
		contact_penalise(c, &out[q], c->ins_ca[2 * (size_t)q]);
	}
	c->ins_ca_n = n_cand;
	c->kept.n_ins_calls++;
	c->kept.n_ins_cands += n_cand;
	return MPMC_OK;
}

// diagnostics only: calls of mpmc_insert_candidates that ran, and the candidates they evaluated
extern "C" int mpmc_debug_insert_batch_counts(mpmc_ctx *c, long long *out2) {
	if (!c || !out2) return -1;
	out2[0] = c->kept.n_ins_calls;
	out2[1] = c->kept.n_ins_cands;
	return 0;
}
