"""shared helpers of the test-suite (tests may use the oracle; the product package may not)."""
import json
import re
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "oracle"))

from mpmcxx_amd import pqr  # noqa: E402

REL_TOL = 1e-9  # BASELINE.json north_star: energies within 1e-9 relative of the reference CPU path

SMALL = ["ar2", "lj64", "ion64_es", "ion216_polar", "ion216_polar_nopbc", "ion216_triclinic", "ion216_frozen",
         "ion216_precision", "ion216_gamma", "ion216_alpha", "water64_polar", "lj1000", "ion1000_polar",
         "ion216_wolf", "water64_fh2", "water64_fh4", "ion216_fh4_polar", "ion216_gs", "water64_gs_precision", "ion1000_gs", "ion216_framework",
         "ion1000_triclinic"]
LARGE = ["ion10k_es", "ion10k_polar", "ion8000_triclinic"]

ENERGY_KEYS = [("energy", "total"), ("rd_energy", "rd"), ("coulombic_energy", "es"), ("polarization_energy", "polar"),
               ("es_real", "es_real"), ("es_recip", "es_recip"), ("es_self", "es_self"),
               ("lj_pairs", "lj_pairs"), ("lrc_pair", "lrc_pair"), ("lrc_self", "lrc_self")]
COUNT_KEYS = ["n_pairs", "n_intra", "n_rd_excluded", "n_es_excluded", "n_frozen", "n_lj_in_cutoff"]


def golden(name):
    with open(os.path.join(GOLDEN, f"{name}.json")) as f:
        return json.load(f)


def load_fixture(name):
    """(atoms, basis, options) parsed from the committed reference-format files."""
    return pqr.load_case(os.path.join(GOLDEN, f"{name}.in"))


def load_generated(name, tmpdir):
    """large boxes are regenerated deterministically instead of being committed as text."""
    from mpmcxx_amd import gen_box

    inp, _ = gen_box.materialize(name, str(tmpdir))
    return pqr.load_case(inp)


def close(a, b, tol=REL_TOL):
    if b == 0.0:
        return abs(a) <= tol
    return abs(a - b) <= tol * abs(b)


def assert_energies(res, g, rd_only, tol=REL_TOL, label="", wolf=False):
    bad = []
    for k_ours, k_gold in ENERGY_KEYS:
        if rd_only and k_gold in ("es", "es_real", "es_recip", "es_self", "polar"):
            continue
        if wolf and k_gold in ("es_real", "es_recip", "es_self"):
            continue  # with wolf on, coulombic() is coulombic_wolf(); the harness' Ewald component columns are not part of it
        if not close(res[k_ours], g[k_gold], tol):
            bad.append(f"{k_gold}: ours {res[k_ours]!r} ref {g[k_gold]!r}")
    assert not bad, f"{label} energy mismatch (tol {tol}): " + "; ".join(bad)


def assert_counts(res, g, rd_only, label=""):
    keys = list(COUNT_KEYS) + ([] if rd_only else ["n_es_in_cutoff"])
    bad = [f"{k}: ours {res[k]} ref {g[k]}" for k in keys if int(res[k]) != int(g[k])]
    assert not bad, f"{label} pair-count mismatch (must be bit-exact): " + "; ".join(bad)


def max_rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = np.abs(b).max()
    return float(np.abs(a - b).max() / scale) if scale > 0 else float(np.abs(a).max())


# ---- trial moves (mpmc_trial_*): shared by test_gpu_trial_moves and test_gpu_trial_branches -------------------------------------------
TRIAL_KEYS = ["energy", "rd_energy", "coulombic_energy", "polarization_energy", "es_real", "es_recip", "lj_pairs"]


def molecules(atoms):
    """(first, end) of every molecule: consecutive atoms with one mol_id"""
    ids = atoms["mol_id"]
    starts = [0] + [i for i in range(1, len(ids)) if ids[i] != ids[i - 1]] + [len(ids)]
    return [(starts[k], starts[k + 1]) for k in range(len(starts) - 1)]


def nonpolar(opts):
    o = dict(opts)
    o.update(polarization=0, polar_iterative=0)
    return o


def moved(atoms, first, m, seed, sigma=0.3):
    """trial positions of atoms [first, first + m): seeded per-atom Gaussian noise, so intramolecular distances change too"""
    rng = np.random.default_rng(seed)
    return atoms["pos"][first:first + m] + rng.normal(scale=sigma, size=(m, 3))


def with_positions(atoms, pos):
    a = dict(atoms)
    a["pos"] = pos
    return a


def component_errors(got, ref, keys, rel):
    """the components of `keys` where |got - ref| > rel * |ref|.  Relative per component, with no absolute floor: a component that is
    identically zero (the polarization energy of a non-polarizable box, the Ewald parts under Wolf) must be exactly 0.0 on both sides,
    so a delta that leaves a residue where there is no term fails.  None of the boxes of the trial tests has a component small enough
    against its terms for rounding to reach these tolerances (1e-11 against a fresh context, 1e-9 against the oracle); a case that
    needs a floor has to state it, with its bound, next to the comparison."""
    return [f"{k}: {got[k]!r} vs {ref[k]!r} (rel {abs(got[k] - ref[k]) / abs(ref[k]) if ref[k] else float('inf'):.2e})"
            for k in keys if not abs(got[k] - ref[k]) <= rel * abs(ref[k])]


def check_trial_against_fresh(S, atoms, basis, opts, pos, rel=1e-11, label=""):
    """S's last trial against a stateless evaluation of the trial configuration `pos` in a new context: every energy component at `rel`,
    the in-cutoff counts exactly.  Returns the fresh context's dipoles (mu, E0, E_ind) for polarizable boxes (None otherwise)."""
    from mpmcxx_amd import energy

    T = energy.System(with_positions(atoms, pos), basis, opts)
    try:
        T.energy()
        got, ref = S.trial_observables, T.observables
        bad = component_errors(got, ref, TRIAL_KEYS, rel)
        assert not bad, f"{label}: trial vs fresh context (rel {rel}): " + "; ".join(bad)
        for k in ("n_lj_in_cutoff", "n_es_in_cutoff", "polar_iterations"):
            assert got[k] == ref[k], (label, k, got[k], ref[k])
        return T.dipoles() if opts.get("polarization") and not opts.get("rd_only") else None
    finally:
        T.close()


def check_trial_against_oracle(obs, atoms, basis, opts, pos, rel=REL_TOL, label=""):
    """trial observables against the oracle on the trial configuration: per component at `rel`, counts bit-exact, the same number of
    dipole iterations.  (Under Wolf the oracle reports the Coulomb energy alone, no Ewald parts and no count.)"""
    from oracle import OracleSystem

    ref = OracleSystem(with_positions(atoms, pos), basis, opts).energy(want_atoms=False)
    wolf = bool(opts.get("wolf"))
    keys = [k for k in TRIAL_KEYS if not (wolf and k in ("es_real", "es_recip"))]
    bad = component_errors(obs, ref, keys, rel)
    assert not bad, f"{label}: trial vs oracle (rel {rel}): " + "; ".join(bad)
    assert obs["n_lj_in_cutoff"] == ref["n_lj_in_cutoff"], (label, obs["n_lj_in_cutoff"], ref["n_lj_in_cutoff"])
    if not wolf:
        assert obs["n_es_in_cutoff"] == ref["n_es_in_cutoff"], (label, obs["n_es_in_cutoff"], ref["n_es_in_cutoff"])
    if opts.get("polarization") and not opts.get("rd_only"):
        assert obs["polar_iterations"] == ref["polar_iterations"], (label, obs["polar_iterations"], ref["polar_iterations"])
    return ref


# ---- the library's diagnostic counters (context.cpp) ---------------------------------------------------------------------------------------
def debug_counts(S, name, count):
    """`count` long longs of the diagnostic entry point `name(ctx, out)`"""
    import ctypes

    from mpmcxx_amd import energy

    fn = getattr(energy.lib(), name)
    fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_longlong)]
    out = (ctypes.c_longlong * count)()
    assert fn(S.handle, out) == 0, name
    return [int(v) for v in out]


def upload_counts(S):
    """(uploads of the atom list that carried the spatial order, uploads that sorted) since the context was made"""
    return tuple(debug_counts(S, "mpmc_debug_upload_counts", 2))


def exchange_counts(S):
    """(exchange trials on the delta path, exchange trials evaluated in full, summations of the host sums over the whole list)"""
    return tuple(debug_counts(S, "mpmc_debug_exchange_counts", 3))


def xch_resum():
    """kXchResum of context.h: accepted exchanges after which the host sums of the exchange delta are re-made from the list"""
    found = re.findall(r"\bkXchResum\s*=\s*(\d+)\s*[;,]", csrc_text("context.h"))
    assert len(found) == 1, found
    return int(found[0])


# ---- one comparison with the oracle: test_gpu_random.check (and through it test_gpu_pair_sweep), test_gpu_edge_cases, test_gpu_box_moves and
# test_gpu_size_ladder -------------------------------------------------------------------------------------------------------------------
def oracle_energy(atoms, basis, opts):
    """the oracle's energy() of one configuration, with the per-atom arrays"""
    from oracle import OracleSystem

    return OracleSystem(atoms, basis, opts).energy()


def field_errors(got, ref, rel=REL_TOL, floor=1e-12, absolute=0.0):
    """atoms i of a per-atom field where |got_i - ref_i|_inf > allowed_i = rel |ref_i|_inf + floor max_j |ref_j|_inf + absolute, the
    largest |got_i - ref_i|_inf / allowed_i (<= 1 exactly when no atom is bad) and the largest |got_i - ref_i|_inf / |ref_i|_inf"""
    got, ref = np.asarray(got, dtype=np.float64).reshape(-1, 3), np.asarray(ref, dtype=np.float64).reshape(-1, 3)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    d = np.abs(got - ref).max(axis=1)
    r = np.abs(ref).max(axis=1)
    top = float(r.max()) if r.size else 0.0
    allowed = rel * r + floor * top + absolute
    bad = np.nonzero(~(d <= allowed))[0]
    if not d.size:
        return bad, 0.0, 0.0
    ratio = float(np.where(allowed > 0, d / np.where(allowed > 0, allowed, 1.0), np.where(d > 0, np.inf, 0.0)).max())
    rel_dev = float(np.where(r > 0, d / np.where(r > 0, r, 1.0), np.where(d > 0, np.inf, 0.0)).max())
    return bad, ratio, rel_dev


def assert_matches_oracle(obs, dipoles, ref, atoms, opts, label="", rel=REL_TOL, fields=None, absolute=None, deviations=None):
    """One evaluation of `atoms` under `opts` (observables `obs`, `dipoles` = System.dipoles() or None) against the oracle's `ref`
    (OracleSystem.energy() with the per-atom arrays).

    - every energy component of ENERGY_KEYS at `rel` relative to the oracle's value, with no absolute floor: a component that is exactly
      zero in the oracle must be exactly 0.0 (under Wolf the oracle has no Ewald parts: they are skipped, as in assert_energies);
    - COUNT_KEYS bit-exact, n_es_in_cutoff too wherever the oracle counts it (not for rd_only boxes, not under Wolf);
    - polarizable boxes: the same number of dipole iterations and the same iterator_failed; dipole_rrms within its conditioning bound
      (test_gpu_parity.test_energy_matches_reference_golden): rrms is a difference of consecutive iterates, so dipoles that agree to eps_mu
      allow rel + 4 eps_mu / rrms; ef_static, mu and ef_induced atom by atom, |x_i - ref_i|_inf <= rel |ref_i|_inf + 1e-12 max_j |ref_j|_inf
      mu exactly zero where alpha = 0.
    A case that needs a looser bound states it next to its call, derived for that case and with the deviation measured: `fields` gives
    {field: (rel, floor)}, `absolute` {energy key or field: an absolute term added to its bound}.
    `deviations`, a dict, collects the largest deviation per key for reporting: relative for the energy components, as a fraction of the
    bound (max_i |d_i| / allowed_i) for the fields."""
    wolf = bool(opts.get("wolf"))
    rd_only = bool(opts.get("rd_only"))
    polar = bool(opts.get("polarization")) and not rd_only
    absolute = absolute or {}
    bad = []
    for k, _ in ENERGY_KEYS:
        if wolf and k in ("es_real", "es_recip", "es_self"):
            continue
        g, r = obs[k], ref[k]
        dev = abs(g - r) / abs(r) if r else (0.0 if g == 0.0 else float("inf"))
        if deviations is not None:
            deviations[k] = max(deviations.get(k, 0.0), dev)
        if not abs(g - r) <= rel * abs(r) + absolute.get(k, 0.0):
            bad.append(f"{k}: ours {g!r} ref {r!r} (rel {dev:.2e})")
    assert not bad, f"{label}: energy vs oracle (rel {rel}, no floor): " + "; ".join(bad)
    keys = list(COUNT_KEYS) + ([] if (rd_only or wolf) else ["n_es_in_cutoff"])
    bad = [f"{k}: ours {obs[k]} ref {ref[k]}" for k in keys if int(obs[k]) != int(ref[k])]
    assert not bad, f"{label}: pair counts vs oracle (bit-exact): " + "; ".join(bad)
    if not polar:
        return
    assert obs["polar_iterations"] == ref["polar_iterations"], (label, "polar_iterations", obs["polar_iterations"], ref["polar_iterations"])
    assert obs["iterator_failed"] == ref["iterator_failed"], (label, "iterator_failed", obs["iterator_failed"], ref["iterator_failed"])
    mu, E, F = dipoles
    bounds = {"ef_static": (rel, 1e-12), "mu": (rel, 1e-12), "ef_induced": (rel, 1e-12)}
    bounds.update(fields or {})
    for name, got in (("ef_static", E), ("mu", mu), ("ef_induced", F)):
        frel, ffloor = bounds[name]
        bad, ratio, rel_dev = field_errors(got, ref[name], frel, ffloor, absolute.get(name, 0.0))
        if deviations is not None:
            deviations[name] = max(deviations.get(name, 0.0), ratio)
        assert bad.size == 0, (f"{label}: {name} vs oracle at {bad.size} atoms (|d_i| <= {frel} |ref_i| + {ffloor} max|ref| + {absolute.get(name, 0.0)}), "
                               f"first {bad[:5].tolist()}, max |d_i| {float(np.abs(np.asarray(got) - np.asarray(ref[name])).max()):.2e}, "
                               f"max |d_i| / |ref_i| {rel_dev:.2e}, max |d_i| / allowed_i {ratio:.2e}")
    alpha0 = np.asarray(atoms["polarizability"]) == 0.0
    assert not np.any(np.asarray(mu).reshape(-1, 3)[alpha0]), f"{label}: non-zero dipole on an atom with alpha = 0"
    eps_mu = max_rel(np.asarray(mu).reshape(-1), np.asarray(ref["mu"]).reshape(-1))
    rr = ref["dipole_rrms"]
    tol_rrms = min(rel + (4.0 * eps_mu / rr if rr > 0 else 0.0), 1e-6)  # (and never looser than the flat 1e-6 the suite held before)
    if deviations is not None:
        deviations["dipole_rrms"] = max(deviations.get("dipole_rrms", 0.0), abs(obs["dipole_rrms"] - rr) / abs(rr) if rr else abs(obs["dipole_rrms"]))
    assert abs(obs["dipole_rrms"] - rr) <= tol_rrms * abs(rr), (label, "dipole_rrms", obs["dipole_rrms"], rr, tol_rrms)



# ---- the size ladder of enqueue() (test_gpu_size_ladder; test_static_rules checks that every constant is found) -------------------------
CSRC = os.path.join(ROOT, "mpmcxx_amd", "csrc")
# the constants that choose kernels and launch shapes by the size of the tile-pair table, and where each is defined
LADDER_CONSTANTS = {"kTile": "kernels.h", "kSingleLaunchTiles": "evaluate.cpp", "kOneStreamMaxPairs": "kernels.h", "kSweepMinPairs": "kernels.h",
                    "kPairSplitMax": "kernels.h", "kKSplit": "kernels.h", "kKSplitMax": "kernels.h", "kKSplitWaves": "kernels.h",
                    "kThreeBodyBlocks": "kernels.h"}
# how they are used: each switch as it is written in the sources (the rungs below assume these directions)
LADDER_USES = {"evaluate.cpp": [r"c->n_tiles <= kSingleLaunchTiles", r"c->n_tile_pairs > kOneStreamMaxPairs", r"c->n_tile_pairs > kSweepMinPairs",
                                r"c->n_tile_pairs <= kPairSplitMax \? 4 : 1"],
               "kernels.h": [r"const int nt = n_pad / kTile;\s*int ks = kKSplit;\s*while \(ks < kKSplitMax && nt \* ks < kKSplitWaves\) ks \*= 2;\s*return ks;"],
               # the three-body launches: one workgroup per tile triple (pair) up to kThreeBodyBlocks, a grid-stride loop above
               "kernels_three_body.hip": [r"std::min<long long>\(work_items, kThreeBodyBlocks\)"]}


def csrc_text(name):
    txt = open(os.path.join(CSRC, name)).read()
    txt = re.sub(r"//[^\n]*", "", txt)
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def ladder_constants():
    """{name: value} of LADDER_CONSTANTS, each read from the one `name = <integer>` of its file (AssertionError if it is missing or defined twice)"""
    out = {}
    for name, f in LADDER_CONSTANTS.items():
        found = re.findall(r"\b" + name + r"\s*=\s*(\d+)\s*[;,]", csrc_text(f))
        assert len(found) == 1, f"{name}: {len(found)} definitions in {f}"
        out[name] = int(found[0])
    return out


def recip_ksplit(nt, c):
    """k-slices of the reciprocal field kernel for nt tiles (kernels.h recip_ksplit; LADDER_USES pins its body)"""
    ks = c["kKSplit"]
    while ks < c["kKSplitMax"] and nt * ks < c["kKSplitWaves"]:
        ks *= 2
    return ks


def size_ladder():
    """The thresholds of enqueue() as tile counts: {rung: (nt, nt + 1)}, one side of the switch at nt tiles, the other at nt + 1.
    The rungs "ksplit_<slices>" are the tile counts from which on the field kernel uses <slices> k-slices."""
    c = ladder_constants()

    def last_within(pairs):  # the largest table of at most `pairs` tile pairs
        nt = 1
        while (nt + 1) * (nt + 2) // 2 <= pairs:
            nt += 1
        return nt

    rungs = {"single_launch": c["kSingleLaunchTiles"], "side_stream": last_within(c["kOneStreamMaxPairs"]),
             "sweep": last_within(c["kSweepMinPairs"]), "pair_waves": last_within(c["kPairSplitMax"])}
    for nt in range(1, c["kKSplitWaves"] + 1):
        if recip_ksplit(nt + 1, c) != recip_ksplit(nt, c):
            rungs[f"ksplit_{recip_ksplit(nt + 1, c)}"] = nt
    return {k: (nt, nt + 1) for k, nt in rungs.items()}


def three_body_ladder():
    """The grid-stride thresholds of kernels_three_body.hip as tile counts: {"full": nt, "delta": nt}, the last tile count whose tile
    triples (k_three_body) / tile pairs (k_three_body_delta) fit in kThreeBodyBlocks workgroups, one each; nt + 1 tiles stride."""
    blocks = ladder_constants()["kThreeBodyBlocks"]

    def last_within(count):
        nt = 1
        while count(nt + 1) <= blocks:
            nt += 1
        return nt

    return {"full": last_within(lambda nt: nt * (nt + 1) * (nt + 2) // 6), "delta": last_within(lambda nt: nt * (nt + 1) // 2)}


def rung_sizes(nt):
    """the two atom counts around a switch between nt and nt + 1 tiles: nt full tiles, and nt + 1 tiles whose last one holds one atom"""
    tile = ladder_constants()["kTile"]
    return (tile * nt, tile * nt + 1)
