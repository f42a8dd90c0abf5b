"""GPU (MI355X): the size-dependent launch paths of enqueue() (csrc/evaluate.cpp) against the oracle, on both sides of every switch.

enqueue() picks kernels and launch shapes by the size of the tile-pair table (nt = ceil(n / 64) tiles, nt (nt + 1) / 2 tile pairs):
the one-launch LJ evaluation up to kSingleLaunchTiles tiles, the number of k-slices of the reciprocal field kernel (recip_ksplit), the
side stream above kOneStreamMaxPairs tile pairs (not for a solve with kOneStreamMinInflight evaluations in flight), the pair sweep above
kSweepMinPairs (with k_pair_fused on the list of tile pairs that hold a kAtomFlagsMixing atom) and one wave per tile pair of k_pair_fused
above kPairSplitMax.  util.size_ladder() reads those constants out of the sources, so the rungs move with them; each rung evaluates a box
of nt full tiles and one of nt + 1 tiles whose last tile holds a single atom.

The boxes are heterogeneous like test_gpu_random's: molecules of 1-4 sites, 15 % frozen molecules, zero charges, polarizabilities,
epsilons and sigmas, unwrapped coordinates, one frozen framework molecule of a few hundred sites, and a handful of sigma < 0 / dispersion
atoms -- enough for a non-empty generic list on the sweep, few enough that it stays a small part of the table.  Every evaluation is
compared with the oracle by util.assert_matches_oracle (1e-9 per component with no floor, counts bit-exact, per-atom fields).  Run with
-s for the largest deviation per key and rung."""
import math
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import util
from mpmcxx_amd import energy

pytestmark = pytest.mark.gpu

E2R = 408.7816
N_FRAME = 320  # sites of the frozen framework molecule: five tiles' worth
LADDER = util.size_ladder()
CONST = util.ladder_constants()


def ladder_box(n, cell, seed, n_frame=N_FRAME):
    """n atoms at about 45 A^3 each: molecule centres (and the framework's sites) on a jittered cubic lattice of the cell's fractional
    coordinates, every molecule shifted by a random whole cell vector (unwrapped coordinates).  n_frame: sites of the frozen framework molecule."""
    rng = np.random.default_rng(seed)
    L = (45.0 * n) ** (1.0 / 3.0)
    if cell == "cubic":
        basis = np.diag([L, L, L])
    elif cell == "ortho":
        f = np.array([0.88, 1.0, 1.15])
        basis = np.diag(L * f / np.prod(f) ** (1.0 / 3.0))
    else:  # triclinic, unit determinant before scaling
        basis = L * np.array([[1.0, 0.0, 0.0], [0.17, 1.0, 0.0], [-0.12, 0.21, 1.0]])
    # molecule sizes in list order: mobile molecules of 1-4 sites, the framework somewhere in between
    sizes = rng.choice([1, 1, 1, 2, 3, 4], size=n)
    cs = np.cumsum(sizes)
    k = int(np.searchsorted(cs, n - n_frame))
    sizes = sizes[:k + 1].copy()
    sizes[-1] -= cs[k] - (n - n_frame)
    sizes = sizes[sizes > 0]
    at = int(rng.integers(1, len(sizes)))
    sizes = np.concatenate([sizes[:at], [n_frame], sizes[at:]])
    frame = np.zeros(len(sizes), dtype=bool)
    frame[at] = True
    # one lattice point per mobile molecule and per framework site
    n_pts = int((sizes[~frame]).size + n_frame)
    g = math.ceil(n_pts ** (1.0 / 3.0))
    sites = rng.permutation(g ** 3)[:n_pts]
    ijk = np.stack([sites // (g * g), (sites // g) % g, sites % g], axis=1).astype(np.float64)
    frac = (ijk + 0.5 + rng.uniform(-0.08, 0.08, size=ijk.shape)) / g
    mol = np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    # centre of every atom's molecule: its own lattice point for framework sites
    pt_of_mol = np.full(len(sizes), -1)
    pt_of_mol[~frame] = np.arange((~frame).sum())
    pt_of_atom = pt_of_mol[mol].copy()
    fr_atoms = np.arange(first[at], first[at] + n_frame)
    pt_of_atom[fr_atoms] = (~frame).sum() + np.arange(n_frame)
    pos = frac[pt_of_atom] @ basis
    rank = np.arange(n) - first[mol]  # position inside the molecule
    off = rng.normal(scale=0.45, size=(n, 3))
    off[(rank == 0) | np.isin(np.arange(n), fr_atoms)] = 0.0
    pos = pos + off + (rng.integers(-1, 2, size=(len(sizes), 3)) @ basis)[mol]
    # per-atom parameters: the mix of test_gpu_random.random_system
    q = np.where(rng.random(n) < 0.25, 0.0, rng.uniform(-0.9, 0.9, n) * E2R)
    al = np.where(rng.random(n) < 0.3, 0.0, rng.uniform(0.2, 1.5, n))
    ep = np.where(rng.random(n) < 0.15, 0.0, rng.uniform(5.0, 150.0, n))
    sg = np.where(rng.random(n) < 0.1, 0.0, rng.uniform(2.0, 3.4, n))
    disp = np.zeros(n, dtype=np.int32)
    mix = rng.choice(n, size=int(rng.integers(2, 7)), replace=False)  # a handful of atoms that change lj_mix
    sg[mix[0::2]] = -rng.uniform(2.0, 3.4, size=len(mix[0::2]))
    disp[mix[1::2]] = 1
    frozen = (rng.random(len(sizes)) < 0.15) | frame
    atoms = {"pos": pos, "charge": q, "polarizability": al, "epsilon": ep, "sigma": sg, "mol_id": mol, "frozen": frozen[mol].astype(np.int32),
             "has_disp": disp, "mass": rng.uniform(1.0, 40.0, n)}
    return atoms, basis


def options(*base, **kw):
    o = {"rd_only": 0, "rd_lrc": 1, "polarization": 0, "polar_iterative": 0, "polar_ewald": 0, "polar_max_iter": 10, "polar_gs": 0,
         "polar_rrms": 0, "ewald_kmax": 7, "polar_precision": 0.0, "polar_gamma": 1.0, "polar_damp": 0.0, "damp_type": "exponential",
         "ewald_alpha": None, "polar_ewald_alpha": None, "wolf": 0, "feynman_hibbs": 0, "feynman_hibbs_order": 0, "temperature": 0.0}
    for b in base + (kw,):
        o.update(b)
    return o


# four iterations: the AUTO solver takes the compact store from four fixed iterations on (choose_solver); the 8 000-atom rung runs two,
# with the solver named
POLAR = dict(polarization=1, polar_iterative=1, polar_ewald=1, polar_damp=2.1304, polar_max_iter=4)
# (rung, case, cell, options of the nt-tile box, options of the nt + 1-tile box); "solver" reaches the library only (the oracle ignores it)
CASES = [
    ("single_launch", "lj", "cubic", options(rd_only=1), options(rd_only=1)),
    # a solve that converges (10 iterations; at the usual damping of 2.1304 the random mix diverges to the 128-iteration limit here)
    ("side_stream", "precision", "cubic", options(POLAR, polar_precision=1e-4, polar_damp=1.0), options(POLAR, polar_precision=1e-4, polar_damp=1.0)),
    ("sweep", "polar", "ortho", options(POLAR), options(POLAR, polar_rrms=1)),  # (also the k-slice switch at 63 / 64 tiles)
    ("sweep", "es", "ortho", options(), options()),
    ("sweep", "gauss_seidel", "ortho", options(POLAR, polar_gs=1), options(POLAR, polar_gs=1, polar_rrms=1)),
    ("sweep", "triclinic", "triclinic", options(POLAR), options(POLAR)),
    ("pair_waves", "polar_compact", "ortho", options(POLAR, polar_max_iter=2, solver="compact"),
     options(POLAR, polar_max_iter=2, polar_rrms=1, solver="compact")),  # (also the k-slice switch at 127 / 128 tiles)
    ("pair_waves", "polar_matrix_free", "ortho", options(POLAR, polar_max_iter=2, solver="matrix_free"),
     options(POLAR, polar_max_iter=2, polar_rrms=1, solver="matrix_free")),
    ("pair_waves", "nopbc_field", "ortho", options(POLAR, polar_ewald=0, polar_max_iter=2), options(POLAR, polar_ewald=0, polar_max_iter=2)),
    ("pair_waves", "wolf", "ortho", options(wolf=1), options(wolf=1)),
    ("pair_waves", "feynman_hibbs4", "ortho", options(feynman_hibbs=1, feynman_hibbs_order=4, temperature=60.0),
     options(feynman_hibbs=1, feynman_hibbs_order=4, temperature=60.0)),
]
# every other k-slice switch: polarizable Ewald, polar_rrms on one side (the ones that fall on the sweep or pair-wave rung are crossed by
# their "polar" cases already)
for _rung in sorted(k for k in LADDER if k.startswith("ksplit_")):
    if LADDER[_rung] not in (LADDER["sweep"], LADDER["pair_waves"]):
        _it = 4 if LADDER[_rung][1] < 100 else 2
        CASES.append((_rung, "polar", "ortho", options(POLAR, polar_max_iter=_it), options(POLAR, polar_max_iter=_it, polar_rrms=1)))
PARAMS = [pytest.param(rung, side, case, cell, o[side], id=f"{rung}-{util.rung_sizes(LADDER[rung][0])[side]}-{case}")
          for rung, case, cell, *o in CASES for side in (0, 1)]


def box(n, cell):
    return ladder_box(n, cell, seed=1000 * n + ["cubic", "ortho", "triclinic"].index(cell))


def oracle_key(n, cell, opts):
    return (n, cell, tuple(sorted((k, v) for k, v in opts.items() if k != "solver")))


_refs = {}
_pool = None
_big = threading.BoundedSemaphore(2)  # oracles whose dense dipole matrix is larger than BIG_MATRIX_BYTES, at once
BIG_MATRIX_BYTES = 2 << 30


def oracle_job(n, cell, opts):
    import oracle as orc

    big = opts["polarization"] and (3 * n) ** 2 * 8 > BIG_MATRIX_BYTES
    if big:
        _big.acquire()
    try:
        return orc.OracleSystem(*box(n, cell), opts).energy()
    finally:
        if big:
            _big.release()


@pytest.fixture(scope="module", autouse=True)
def oracle_pool(request):
    """The oracle is serial and is what this file costs: every (box, options) of the selected tests is computed once, on a few threads
    (the oracle's C code holds no global state and ctypes lets go of the GIL), submitted in test order so that the GPU side rarely
    waits.  At most four at a time, and at most two of the polarizable ones above 2 GB: the oracle's dense dipole matrix of an 8 129-atom
    box is 4.8 GB."""
    global _pool
    import oracle as orc

    orc.lib()  # build / load once, before the threads
    _pool = ThreadPoolExecutor(max_workers=4)
    for item in request.session.items:
        if item.module is not request.module or "rung" not in getattr(getattr(item, "callspec", None), "params", {}):
            continue
        rung, side, cell, opts = (item.callspec.params[k] for k in ("rung", "side", "cell", "opts"))
        n = util.rung_sizes(LADDER[rung][0])[side]
        key = oracle_key(n, cell, opts)
        if key not in _refs:
            _refs[key] = _pool.submit(oracle_job, n, cell, opts)
    yield
    _pool.shutdown(wait=True, cancel_futures=True)
    if DEVIATIONS:
        print("\nlargest deviation from the oracle per rung and key (energies: relative; fields: max_i |d_i| / allowed_i, 1 = the bound):")
        for label, d in DEVIATIONS.items():
            print(f"  {label}: " + ", ".join(f"{k} {v:.1e}" for k, v in d.items()))


DEVIATIONS = {}


def compact_store_expected(opts):
    """choose_solver (evaluate.cpp): Gauss-Seidel and matrix_free recompute the tensors; AUTO stores them for a precision-terminated
    solve or more than three fixed iterations (the store fits the default budget at every rung)"""
    solver = opts.get("solver", "auto")
    if opts["polar_gs"] or solver == "matrix_free":
        return False
    return solver == "compact" or opts["polar_precision"] != 0.0 or opts["polar_max_iter"] > 3


def has_mixing_atom(atoms):
    return bool(np.any(atoms["sigma"] < 0) or np.any(atoms["has_disp"] != 0))


@pytest.mark.parametrize("rung, side, case, cell, opts", PARAMS)
def test_size_ladder_against_oracle(rung, side, case, cell, opts):
    nt = LADDER[rung][side]
    n = util.rung_sizes(LADDER[rung][0])[side]
    atoms, basis = box(n, cell)
    assert len(atoms["charge"]) == n and -(-n // CONST["kTile"]) == nt
    ref = _refs[oracle_key(n, cell, opts)].result()
    label = f"{rung} n={n} ({nt} tiles) {case}"
    polar = bool(opts["polarization"])
    S = energy.System(atoms, basis, opts)
    try:
        S.energy()
        obs = dict(S.observables)
        dev = DEVIATIONS.setdefault(label, {})
        util.assert_matches_oracle(obs, S.dipoles() if polar else None, ref, atoms, opts, label=label, deviations=dev)

        # ---- which path ran.  On the single_launch rung the tile count is the only evidence: last_pair_kernel() tells the sweep from
        # k_pair_fused, not the one-launch LJ kernel (32 tiles) from the general LJ path (33 tiles), and no accessor reports that choice
        pairs = nt * (nt + 1) // 2
        assert S.tile_stats()["tile_pairs"] == pairs, label
        in_sweep_domain = not (opts["rd_only"] or opts["wolf"] or opts["feynman_hibbs"] or (polar and not opts["polar_ewald"]))
        want = "sweep" if in_sweep_domain and pairs > CONST["kSweepMinPairs"] else "fused"
        assert S.last_pair_kernel() == want, (label, S.last_pair_kernel(), want)
        if want == "sweep" or rung == "single_launch":
            assert has_mixing_atom(atoms), label  # the generic list next to the sweep is not empty / the LJ kernels meet lj_mix's branches
        if polar:
            assert (S.memory_usage()[1] > 0) == compact_store_expected(opts), (label, S.memory_usage())  # the compact Thole store

        if rung == "side_stream":
            # the same evaluation with kOneStreamMinInflight evaluations in flight: a solve stays on one stream at any size.  The choice of
            # streams does not touch the arithmetic: bit-identical to the plain evaluation.  (energy() resets the hint; energy_async keeps it.)
            S.hint_in_flight(4)
            S.energy_async()
            S.energy_wait()
            hinted = dict(S.observables)
            for k, _ in util.ENERGY_KEYS:
                assert hinted[k] == obs[k], (label, "hinted", k, hinted[k], obs[k])
            for k in list(util.COUNT_KEYS) + ["n_es_in_cutoff", "polar_iterations", "iterator_failed", "dipole_rrms"]:
                assert hinted[k] == obs[k], (label, "hinted", k, hinted[k], obs[k])
            util.assert_matches_oracle(hinted, S.dipoles(), ref, atoms, opts, label=label + " hinted", deviations=dev)
    finally:
        S.close()


@pytest.mark.parametrize("case", ["one_atom", "one_lj_atom", "only_frozen_lj_atoms", "one_mobile_pair"])
def test_pair_lrc_of_an_empty_pair_set_is_exactly_zero(case):
    """Found by the floor-free comparison (test_gpu_random seeds 0, 11, 22 and Gauss-Seidel seed 0): the pair LRC is summed in O(N) from
    moments (kernels.hip k_atom_terms_*), and where no pair with eps_ij, sigma_ij != 0 is left -- one such atom, or all of them frozen --
    the moments cancelled only up to rounding (-5e-16 for one atom) where the reference's sum over no pairs is exactly 0."""
    rng = np.random.default_rng(5)
    n = 1 if case == "one_atom" else 6
    atoms = {"pos": rng.uniform(0.0, 12.0, size=(n, 3)), "charge": np.zeros(n), "polarizability": np.zeros(n), "epsilon": np.zeros(n),
             "sigma": np.full(n, 3.0), "mol_id": np.arange(n, dtype=np.int32), "frozen": np.zeros(n, dtype=np.int32),
             "has_disp": np.zeros(n, dtype=np.int32), "mass": np.ones(n)}
    lj = {"one_atom": [0], "one_lj_atom": [2], "only_frozen_lj_atoms": [1, 3, 4], "one_mobile_pair": [1, 3, 4]}[case]
    atoms["epsilon"][lj] = rng.uniform(20.0, 150.0, size=len(lj))
    atoms["sigma"][lj] = rng.uniform(2.0, 3.4, size=len(lj))
    if case == "only_frozen_lj_atoms":
        atoms["frozen"][lj] = 1
    if case == "one_mobile_pair":
        atoms["frozen"][[1, 3]] = 1  # frozen-frozen (1, 3) is excluded; (1, 4) and (3, 4) remain
    basis = np.diag([12.0, 13.0, 14.0])
    opts = options(rd_only=1)
    ref = util.oracle_energy(atoms, basis, opts)
    S = energy.System(atoms, basis, opts)
    try:
        S.energy()
        util.assert_matches_oracle(S.observables, None, ref, atoms, opts, label=case)
        assert (S.observables["lrc_pair"] == 0.0) == (case != "one_mobile_pair"), (case, S.observables["lrc_pair"])
    finally:
        S.close()
