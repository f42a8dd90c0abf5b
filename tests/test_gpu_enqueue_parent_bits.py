"""GPU (MI355X): enqueue() as a plan, the room it needs and a list of stages (csrc/evaluate.cpp) gives the bits and the launches of the
commit before it was split.

tests/golden/enqueue_parent.json holds, per case, what `record` returns with the PARENT commit's library on an MI355X.  Per evaluation:
every field of the result as a bit pattern (float.hex(); the counts, `polar_iterations` and `iterator_failed` as integers), the
launches per timing class, last_pair_kernel() and, for polarizable boxes, the sha256 of the bytes of mu, ef_static and ef_induced.
Every context is evaluated three times: the FIRST evaluation (the one that allocates: the split moved every allocation in front of the
first launch), a steady-state one, and one under profiling (the launch counts; a profiled context never takes the one-launch LJ path,
which is why the two before it are recorded as well).  Equality is exact.

Cases: the smallest boxes that reach each branch of the plan.
- both sides of the single_launch, side_stream and sweep rungs of tests/test_gpu_size_ladder.py, with that file's boxes and options, and
  the pair_waves rung's two polarizable cases (compact store, matrix-free); the side_stream boxes once more with four evaluations in flight
  (a solve then keeps to one stream).  No oracle runs here.
- ion216_polar (four tiles): the direct solve, the dense solver, a precision-terminated solve that reports rrms, Gauss-Seidel sweeps with
  `polar_palmo`, dipoles on demand (energy(), then dipoles()) alone and with a hint of four evaluations in flight.
- one live context per term: every component entry point followed by energy().
- the position-independent terms riding along: an Ewald box of more than kSingleLaunchTiles tiles whose atom list is set again with one
  molecule inserted.
- lj1000 with the one-launch path on and off.
Where the library can tell, `record` asserts that the intended branch ran (last_pair_kernel(), launches per class, the tensor bytes of
memory_usage(), direct_info(), the Palmo-Krimm correction): a case that silently took another path would test nothing.  Nothing reports the
choice of streams or the one-launch LJ path; those cases rest on the sizes of their boxes (util.size_ladder reads the thresholds from the
sources).

To regenerate the golden (a compiler or ROCm change that moves a last bit): build the library of the commit before "Split the evaluation's
enqueue" (python -c "from mpmcxx_amd import build; build.build_library()" in a checkout of it) and run, in this tree on the GPU,
    PYTHONPATH=. MPMC_ENERGY_LIB=/path/to/that/libmpmc_energy.so python tests/test_gpu_enqueue_parent_bits.py tests/golden/enqueue_parent.json
(energy.py loads the library the variable names instead of the tree's own)."""
import hashlib
import json
import os

import numpy as np
import pytest

import disp_expansion_ref as D
import rd_crystal_ref as R
import test_gpu_size_ladder as ladder
import three_body_ref as T
import util
from mpmcxx_amd import energy
from test_gpu_size_ladder import CASES as LADDER_CASES
from test_gpu_size_ladder import ladder_box, options

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(util.GOLDEN, "enqueue_parent.json")
LADDER = util.size_ladder()
CONST = util.ladder_constants()
RUNGS = {"single_launch": None, "side_stream": None, "sweep": None, "pair_waves": ("polar_compact", "polar_matrix_free")}  # None: every case of the rung


def bits(obs):
    return {k: (float(v).hex() if isinstance(v, float) else int(v)) for k, v in obs.items()}


def launches(S):
    return {k: v["launches"] for k, v in S.timings(reset=True).items()}


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def fields(S):
    return dict(zip(("mu", "ef_static", "ef_induced"), map(digest, S.dipoles())))


def evaluation(S, polar, run=None):
    """one evaluation (energy(), or `run`) of a context: result, launches since the last look, pair kernel, per-atom fields"""
    (run or S.energy)()
    rec = {"result": bits(S.observables), "launches": launches(S), "pair_kernel": S.last_pair_kernel()}
    if polar:
        rec["fields"] = fields(S)
    return rec


def three_evaluations(S, polar, run=None):
    rec = {"first": evaluation(S, polar, run), "steady": evaluation(S, polar, run)}
    S.set_profiling(True)
    S.timings(reset=True)
    rec["profiled"] = evaluation(S, polar, run)
    return rec


def polar_of(opts):
    return bool(opts.get("polarization")) and not opts.get("rd_only")


# ---- the size ladder ----------------------------------------------------------------------------------------------------------------
def ladder_case(rung, side, case, cell, opts):
    nt = LADDER[rung][side]
    n = util.rung_sizes(LADDER[rung][0])[side]
    atoms, basis = ladder.box(n, cell)
    polar = polar_of(opts)
    S = energy.System(atoms, basis, opts)
    try:
        rec = three_evaluations(S, polar)
        pairs = nt * (nt + 1) // 2
        assert S.tile_stats()["tile_pairs"] == pairs, (rung, side, case)
        in_sweep_domain = not (opts["rd_only"] or opts["wolf"] or opts["feynman_hibbs"] or (polar and not opts["polar_ewald"]))
        want = "sweep" if in_sweep_domain and pairs > CONST["kSweepMinPairs"] else "fused"
        assert rec["profiled"]["pair_kernel"] == want, (rung, side, case, rec["profiled"]["pair_kernel"], want)
        if want == "sweep":  # the generic list next to the sweep is not empty: two launches of the pair class
            assert ladder.has_mixing_atom(atoms) and rec["profiled"]["launches"]["pair"] == 2, (rung, side, case, rec["profiled"]["launches"])
        if polar:
            assert (S.memory_usage()[1] > 0) == ladder.compact_store_expected(opts), (rung, side, case, S.memory_usage())
            assert rec["profiled"]["launches"]["tensor"] == (1 if opts["polar_gs"] else 0), (rung, side, case, rec["profiled"]["launches"])
        if rung == "side_stream":  # four evaluations in flight: the solve keeps to one stream at either size (energy() resets the hint)
            def hinted():
                S.hint_in_flight(4)
                S.energy_async()
                S.energy_wait()

            rec["hinted"] = evaluation(S, polar, hinted)
        return rec
    finally:
        S.close()


CASES = {}
for _rung, _case, _cell, *_o in LADDER_CASES:
    if _rung in RUNGS and (RUNGS[_rung] is None or _case in RUNGS[_rung]):
        for _side in (0, 1):
            CASES[f"{_rung}-{util.rung_sizes(LADDER[_rung][0])[_side]}-{_case}"] = (
                lambda rung=_rung, side=_side, case=_case, cell=_cell, opts=_o[_side]: ladder_case(rung, side, case, cell, opts))


# ---- ion216_polar, four tiles -------------------------------------------------------------------------------------------------------------
def small_box(**extra):
    atoms, basis, opts = util.load_fixture("ion216_polar")
    return atoms, basis, dict(opts, **extra)


def small_direct():
    S = energy.System(*small_box(polar_iterative=0))
    try:
        rec = three_evaluations(S, True)
        info = S.direct_info()
        assert info["n_unknowns"] > 0 and info["status"] == 0 and info["factor_bytes"] > 0, info
        assert rec["profiled"]["launches"]["tensor"] == 1 and rec["profiled"]["result"]["polar_iterations"] == 0, rec["profiled"]
        rec["direct_info"] = bits(info)
        return rec
    finally:
        S.close()


def small_dense():
    S = energy.System(*small_box(solver="dense"))
    try:
        rec = three_evaluations(S, True)
        # k_dense_build, and nothing in the compact store
        assert rec["profiled"]["launches"]["tensor"] == 1 and S.memory_usage()[1] == 0, (rec["profiled"]["launches"], S.memory_usage())
        return rec
    finally:
        S.close()


def small_precision():
    S = energy.System(*small_box(polar_precision=1e-6, polar_max_iter=30, polar_rrms=1))
    try:
        rec = three_evaluations(S, True)
        r = rec["profiled"]["result"]
        # terminated by the precision (not by a count), rrms reported, the tensor store in use
        assert 0 < r["polar_iterations"] and r["iterator_failed"] == 0 and float.fromhex(r["dipole_rrms"]) > 0.0 and S.memory_usage()[1] > 0, r
        return rec
    finally:
        S.close()


def small_gs_palmo():
    S = energy.System(*small_box(polar_gs=1, polar_palmo=1))
    try:
        rec = three_evaluations(S, True)
        corr, change = S.palmo_info()
        assert corr != 0.0 and rec["profiled"]["launches"]["tensor"] == 1 and S.memory_usage()[1] == 0, (corr, rec["profiled"]["launches"])
        rec["palmo"] = {"correction": float(corr).hex(), "change": digest(change)}
        return rec
    finally:
        S.close()


def small_on_demand(hint):
    atoms, basis, opts = small_box()
    n_it = opts["polar_max_iter"]
    S = energy.System(atoms, basis, opts)
    S.set_dipoles_on_demand(True)

    def run():
        if hint:
            S.hint_in_flight(hint)
            S.energy_async()
            S.energy_wait()
        else:
            S.energy()

    def step():  # the evaluation, then the dipoles it left undone (finish_pending_dipoles)
        run()
        rec = {"result": bits(S.observables), "launches": launches(S), "pair_kernel": S.last_pair_kernel()}
        rec["fields"] = fields(S)
        rec["launches_of_the_dipoles"] = launches(S)
        return rec

    try:
        rec = {"first": step(), "steady": step()}
        S.set_profiling(True)
        S.timings(reset=True)
        rec["profiled"] = p = step()
        half = (n_it + 1) // 2
        assert p["launches"]["dipole_iter"] == half and p["launches_of_the_dipoles"]["dipole_iter"] == n_it - half, p
        assert p["result"]["polar_iterations"] == n_it, p["result"]
        return rec
    finally:
        S.close()


CASES.update({"ion216_direct": small_direct, "ion216_dense": small_dense, "ion216_precision_rrms": small_precision, "ion216_gs_palmo": small_gs_palmo,
              "ion216_on_demand": lambda: small_on_demand(0), "ion216_on_demand_in_flight": lambda: small_on_demand(4)})


# ---- one live context: every component entry point, each followed by energy() -------------------------------------------------------------
def live_sequence(box, pieces):
    atoms, basis, opts = box
    polar = polar_of(opts)
    S = energy.System(atoms, basis, opts)
    try:
        S.energy()
        S.set_profiling(True)
        S.timings(reset=True)
        rec = {}
        for name in pieces:
            v = getattr(S, name)()
            piece = {"value": digest(v) if isinstance(v, np.ndarray) else float(v).hex(), "launches": launches(S), "pair_kernel": S.last_pair_kernel()}
            rec[name] = {"piece": piece, "energy": evaluation(S, polar)}
        if "rd_crystal" in opts:
            info = S.rd_crystal_info()
            assert info["order"] == 2 and info["n_image_terms"] > 0, info
            rec["rd_crystal_info"] = bits(info)
        return rec
    finally:
        S.close()


PIECES = ["lj", "coulombic", "coulombic_real", "coulombic_reciprocal", "coulombic_self", "polar", "thole_field"]
CASES.update({"live_ion216_polar": lambda: live_sequence(util.load_fixture("ion216_polar"), PIECES),
              "live_ion216_polar_at": lambda: live_sequence(T.load("ion216_polar_at"), ["axilrod_teller"]),
              "live_ion216_polar_disp": lambda: live_sequence(D.load("ion216_polar_disp"), ["disp_expansion"]),
              "live_water64_polar_rc2": lambda: live_sequence(R.load("water64_polar_rc2"), ["lj"])})


# ---- the position-independent terms ride along with the evaluation behind an insertion ------------------------------------------------------
def static_ride():
    nt = CONST["kSingleLaunchTiles"] + 2
    n = CONST["kTile"] * nt - 7
    atoms, basis = ladder_box(n, "cubic", seed=77)
    opts = options()
    S = energy.System(atoms, basis, opts, max_atoms=n + CONST["kTile"])  # (room for the insertion: the context is not rebuilt)
    try:
        rec = {"before": evaluation(S, False)}
        more = {k: np.concatenate([v, v[-1:]]) for k, v in atoms.items()}
        more["pos"][-1] = 0.37 * basis.sum(axis=0)
        more["mol_id"][-1] = more["mol_id"].max() + 1
        more["frozen"][-1] = 0
        more["epsilon"][-1], more["sigma"][-1], more["charge"][-1] = 80.0, 3.1, 0.4 * ladder.E2R
        S.set_atoms(more)
        rec["after"] = evaluation(S, False)
        rec["again"] = evaluation(S, False)
        assert S.tile_stats()["tile_pairs"] == nt * (nt + 1) // 2
        b, a = rec["before"]["result"], rec["after"]["result"]
        assert a["lrc_pair"] != b["lrc_pair"] and a["es_self"] != b["es_self"] and a["n_pairs"] == b["n_pairs"] + n, (a, b)  # the new terms were adopted
        assert rec["again"]["result"] == a
        return rec
    finally:
        S.close()


# ---- the one-launch LJ evaluation, switched on and off ------------------------------------------------------------------------------------
def single_launch_switch():
    atoms, basis, opts = util.load_fixture("lj1000")
    rec = {}
    for on in (1, 0):
        S = energy.System(atoms, basis, opts)
        try:
            S.configure("single_launch", on)
            rec["on" if on else "off"] = three_evaluations(S, False)
        finally:
            S.close()
    assert rec["off"]["profiled"]["launches"]["pair"] == 1 and rec["off"]["profiled"]["launches"]["classes"] == 1, rec["off"]["profiled"]
    return rec


CASES.update({"static_terms_ride_along": static_ride, "lj1000_single_launch_switch": single_launch_switch})


def record(label):
    return json.loads(json.dumps(CASES[label]()))


def first_difference(got, want, path=""):
    if isinstance(got, dict) and isinstance(want, dict):
        for k in sorted(set(got) | set(want)):
            if got.get(k) != want.get(k):
                return first_difference(got.get(k), want.get(k), f"{path}/{k}")
    return path, got, want


@pytest.mark.parametrize("label", sorted(CASES))
def test_bits_and_launches_of_the_parent(label):
    with open(GOLDEN) as f:
        want = json.load(f)[label]
    got = record(label)
    assert got == want, (label,) + first_difference(got, want)  # (names what differs first: the whole record is long)


if __name__ == "__main__":  # regenerate the golden from the library MPMC_ENERGY_LIB names (see the module docstring)
    import sys

    with open(sys.argv[1], "w") as f:
        json.dump({k: record(k) for k in sorted(CASES)}, f, indent=0, sort_keys=True)
