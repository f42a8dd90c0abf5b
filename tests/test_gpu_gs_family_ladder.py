"""GPU (MI355X): the Gauss-Seidel family past 16 tiles and on ranked views whose tile pairs have classes.

Every other GPU test of `polar_gs_ranked`, of `polar_sor` / `polar_esor` under Gauss-Seidel and of `polar_wolf` / `polar_palmo` stops at
1000 atoms in a 40 A cube: 16 tiles, one trip of k_gr_rows' column loop (kRankWaves = 16 tiles per trip), no tile pair beyond the 20 A
cutoff and a ranked view with next to no far or common-image tile pairs.  The slab boxes of gen_box.slab_box reach all of that at 1089
atoms: a 25.2 x 25.2 x 82.8 A cell (cutoff 12.6 A, Thole far distance 14.1 A) filled layer by layer, so that the 18 tiles of the list
order are slabs about 5 A thick.
  planted     a handful of atoms 2.0 A from a neighbour: about 20 atoms have a rank, the ranked view is the list with those pulled to
              the front, and its tiles are still slabs -- the view has far, beyond-cutoff and common-image tile pairs (asserted through
              mpmc_debug_gs_ranked_pair_stats); also in a triclinic cell
  scrambled   nearly every atom has a rank: every tile of the view spans the cell
Yardsticks: the restatement's rank pass (rmin its double, rank_metric and order its integers: against_rank_pass) and its dense solve
tests/polar_gs_ranked_ref.py with the bounds of test_gpu_polar_gs_ranked.test_matrix_against_the_restatement (REF_REL_E, REF_REL_MU, the
rrms rule, equal iteration counts, the Palmo-Krimm correction at 1e-9 |U_pol|).  The two planted boxes are GS_RANKED_FIXTURES too:
test_gpu_polar_gs_ranked.test_golden holds the device to the reference's own results on them.  Run with -s for the measured deviations.

As measured on an MI355X (energy relative; mu and ef_induced as fractions of their bounds; ef_static 1.0e-4 of its bound at most):
  ranked, planted orthorhombic   ewald 1.1e-15 / 2.1e-3 / 1.5e-2 (tile_classes off 8.6e-16 / 1.6e-4 / 1.4e-4, uniform_images off as on)
                                 nopbc 6.9e-16 / 2.1e-3 / 1.3e-2   wolf 2.1e-16 / 1.3e-3 / 1.0e-2   rrms 1.1e-15, rrms itself 1.5e-13
                                 precision (7 iterations) 8.6e-16, rrms 3.2e-12   sor 1.3e-15   esor_palmo 6.5e-16, correction 1.8e-15 |U_pol|
  ranked, planted triclinic      ewald 9.7e-16 / 1.2e-3 / 1.0e-2 (tile_classes off 9.7e-16 / 4.8e-5 / 1.1e-4)   esor_palmo 1.9e-16, 4.5e-16 |U_pol|
  ranked, scrambled              ewald 6.9e-16 / 5.7e-5 / 5.9e-5   esor_palmo 4.1e-16 / 5.9e-5 / 1.2e-4, 1.7e-16 |U_pol|
  atom order, orthorhombic       gs 2.2e-16 / 2.8e-3 / 9.8e-3   esor + palmo 4.3e-16, 7.3e-16 |U_pol|   wolf + palmo 4.2e-16, 3.0e-16 |U_pol|
  atom order, triclinic          gs 7.8e-16 / 2.9e-3 / 9.2e-3   esor + palmo 7.8e-16, 1.3e-16 |U_pol|   wolf + palmo 2.2e-15, 3.6e-16 |U_pol|
  ranked against plain polar_gs  7.1e-5 (orthorhombic), 7.0e-5 (triclinic)
  ranked views, of 153 off-diagonal tile pairs: planted (both cells) 66 far, 66 beyond the cutoff, 120 with a common image, 28 of them not
  the zero image; scrambled 10 / 11 / 39 / 4.  Atom order: 76 far and 76 beyond the cutoff of 171.
(The far-field class drops the Thole damping beyond lambda r = 30: with the classes on, mu and ef_induced sit at 1e-3 to 1e-2 of their
1e-9 bounds instead of 1e-4.)
"""
import numpy as np
import pytest

import util
import polar_gs_ranked_ref as ref
from test_gpu_polar_gs_ranked import MATRIX, REF_REL_E, REF_REL_MU, REL, against_rank_pass
from test_polar_gs_ranked import planted_preconditions
from mpmcxx_amd import energy

pytestmark = pytest.mark.gpu

ORTHO, TRI, SCRAMBLED = "slab1089_planted", "slab1089_planted_tri", "slab1089_scrambled"
TRIP_SIZES = (1024, 1025, 1089, 2049)  # 16 full tiles: one trip; 17 tiles: one live wave in the second; 18; 33 tiles: three trips
NAMES = [ORTHO, TRI, SCRAMBLED] + [f"slab{n}_planted" for n in TRIP_SIZES if n != 1089]


@pytest.fixture(scope="module")
def slabs(tmp_path_factory):
    """{name: (atoms, basis, options)}, the options with sweeps in atom order (polar_gs).  The preconditions of every planted box are
    asserted here, on the CPU, before anything runs on the device."""
    d = tmp_path_factory.mktemp("gs_ladder")
    out = {name: util.load_generated(name, d) for name in NAMES}
    for name, (atoms, basis, o) in out.items():
        assert o["polar_gs"] == 1 and o["polar_max_iter"] == 3 and len(atoms["charge"]) == int(name[4:8])
        if "planted" in name:
            planted_preconditions(atoms, basis)
    return out


@pytest.fixture(scope="module")
def restated():
    """the restatement's solve of (box, options, sweep order), computed once per module"""
    kept = {}

    def get(key, atoms, basis, o, order=None):
        if key not in kept:
            kept[key] = ref.solve(atoms, basis, o, order=order)
        return kept[key]

    return get


def ranked(o, **kw):
    return dict(o, polar_gs=0, polar_gs_ranked=1, **kw)


def against_the_restatement(S, want, o, label):
    """test_gpu_polar_gs_ranked.test_matrix_against_the_restatement's comparison, bound for bound"""
    obs = S.observables
    mu, E0, F = S.dipoles()
    assert obs["polar_iterations"] == want["polar_iterations"] and obs["iterator_failed"] == want["iterator_failed"] == 0, label
    dev = abs(obs["polarization_energy"] - want["polarization_energy"]) / abs(want["polarization_energy"])
    lines = [f"energy {dev:.1e}"]
    fails = []
    if not dev <= REF_REL_E:
        fails.append(("energy", obs["polarization_energy"], want["polarization_energy"]))
    for k, got in (("ef_static", E0), ("mu", mu), ("ef_induced", F)):
        bad, ratio, _ = util.field_errors(got, want[k], REF_REL_MU, 1e-12)
        lines.append(f"{k} {ratio:.1e} of its bound")
        if bad.size:
            fails.append((k, ratio, bad[:5].tolist()))
    rr = want["dipole_rrms"]
    if rr:
        eps_mu = util.max_rel(np.asarray(mu).reshape(-1), want["mu"].reshape(-1))
        lines.append(f"rrms {abs(obs['dipole_rrms'] - rr) / rr:.1e}")
        if not abs(obs["dipole_rrms"] - rr) <= min(REL + 4.0 * eps_mu / rr, 1e-6) * rr:
            fails.append(("rrms", obs["dipole_rrms"], rr))
    elif obs["dipole_rrms"] != 0.0:
        fails.append(("rrms", obs["dipole_rrms"], 0.0))
    if o.get("polar_palmo"):
        corr = S.palmo_info()[0]
        lines.append(f"palmo {abs(corr - want['correction']) / abs(want['polarization_energy']):.1e} of U_pol")
        if not (abs(corr - want["correction"]) <= REL * abs(want["polarization_energy"]) and want["correction"] != 0.0):
            fails.append(("palmo", corr, want["correction"]))
    print(f"\n{label}: iterations {obs['polar_iterations']} " + " ".join(lines))
    assert not fails, (label, fails)
    assert not np.any(np.asarray(mu)[np.asarray(S.atoms["polarizability"]) == 0.0]), label


# ---- A. the rank pass and the sort past one trip of k_gr_rows ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", TRIP_SIZES)
def test_rank_pass_past_one_trip(slabs, n):
    atoms, basis, o = slabs[f"slab{n}_planted"]
    S = energy.System(atoms, basis, ranked(o, polar_max_iter=2))
    try:
        S.energy()
        info = against_rank_pass(S, atoms, basis, 1, f"n = {n}")
        assert info["max_rank"] >= 2 and info["n_moved"] > 0, info
        print(f"\nn = {n}: tiles {-(-n // 64)} rmin {info['rmin']!r} max_rank {info['max_rank']} n_moved {info['n_moved']}")
    finally:
        S.close()


def test_the_sort_over_three_trips(slabs):
    """mpmc_debug_gs_rank_order at n = 2049 (33 tiles: trips of 16, 16 and 1 column tiles, the last with one atom)"""
    n = 2049
    atoms, basis, o = slabs[f"slab{n}_planted"]
    S = energy.System(atoms, basis, ranked(o, polar_max_iter=2))
    try:
        S.energy()
        L = energy.lib()
        rng = np.random.default_rng(7)
        i = np.arange(n)
        sets = {"random below n": rng.integers(0, n, size=n), "all equal": np.full(n, 5), "ascending": i, "descending": i[::-1].copy(),
                "ties across the trips": i // 1024, "one large key in the last tile": np.where(i == n - 1, n - 1, 0)}
        for label, keys in sets.items():
            keys = np.ascontiguousarray(keys, dtype=np.int32)
            got = np.full(n, -1, dtype=np.int32)
            S._check(L.mpmc_debug_gs_rank_order(S.handle, energy._ip(keys), energy._ip(got)))
            assert np.array_equal(got, np.argsort(-keys.astype(np.int64), kind="stable")), (label, got[:8])
    finally:
        S.close()


# ---- B. ranked sweeps on views that have classes ----------------------------------------------------------------------------------------------
def view_stats(S, name):
    """the classes of the ranked view just swept; the conditions that keep the comparison from passing on a view of generic tile pairs"""
    st = S.gs_ranked_pair_stats()
    off = st["tile_pairs_off_diagonal"]
    print(f"\n{name}: ranked view, of {off} off-diagonal tile pairs: far {st['tile_pairs_far']} beyond the cutoff {st['tile_pairs_beyond_cutoff']} "
          f"common image {st['tile_pairs_common_image']} of those not the zero image {st['tile_pairs_shifted']}")
    assert st["tile_pairs"] == 171 and off == 153, st
    if name == ORTHO:
        assert 4 * st["tile_pairs_far"] >= off and 4 * st["tile_pairs_beyond_cutoff"] >= off, st
        assert st["tile_pairs_common_image"] > 0 and st["tile_pairs_shifted"] > 0, st
    elif name == TRI:
        assert st["tile_pairs_far"] > 0 and st["tile_pairs_beyond_cutoff"] > 0 and st["tile_pairs_common_image"] > 0, st
    return st


RANKED_CASES = [(ORTHO, case) for case in sorted(MATRIX)] + [(name, case) for name in (TRI, SCRAMBLED) for case in ("ewald", "esor_palmo")]


@pytest.mark.parametrize("name,case", RANKED_CASES)
def test_ranked_sweeps_against_the_restatement(slabs, restated, name, case):
    atoms, basis, base = slabs[name]
    o = ranked(base, polar_max_iter=3)
    o.update(MATRIX[case])
    want = restated((name, case, "ranked"), atoms, basis, o)
    # the `ewald` cases also with the view's classes, then its common images, switched off: the same restatement at the same bounds
    for switch in (None, "tile_classes", "uniform_images") if case == "ewald" else (None,):
        label = f"{name} {case}" + (f" {switch} off" if switch else "")
        S = energy.System(atoms, basis, o)
        try:
            if switch:
                S.configure(switch, 0)
            S.energy()
            against_the_restatement(S, want, o, label)
            against_rank_pass(S, atoms, basis, want["ranked_sweeps"], label)
            if case == "ewald":
                st = S.gs_ranked_pair_stats() if switch else view_stats(S, name)
                if switch == "tile_classes":
                    assert st["tile_pairs_far"] == st["tile_pairs_beyond_cutoff"] == st["tile_pairs_common_image"] == 0, st
                if switch == "uniform_images":
                    assert st["tile_pairs_common_image"] == 0 and (name == SCRAMBLED or st["tile_pairs_far"] > 0), st
        finally:
            S.close()


@pytest.mark.parametrize("name", [ORTHO, TRI])
def test_ranked_sweeps_are_not_plain_sweeps(slabs, name):
    """the device's own polar_gs energy is further from its ranked energy than 100 times the bound of the comparison above (the restatements
    differ by 2e-5): that comparison cannot be passed by sweeping in atom order"""
    atoms, basis, o = slabs[name]
    got = {}
    for key, opts in (("ranked", ranked(o)), ("plain", o)):
        S = energy.System(atoms, basis, opts)
        try:
            S.energy()
            got[key] = S.observables["polarization_energy"]
        finally:
            S.close()
    print(f"\n{name}: ranked {got['ranked']!r} polar_gs {got['plain']!r} rel {abs(got['ranked'] - got['plain']) / abs(got['plain']):.2e}")
    assert abs(got["ranked"] - got["plain"]) > 100.0 * REL * abs(got["plain"])


# ---- C. plain, relaxed and Wolf / Palmo-Krimm sweeps on a table with skipped tile pairs ------------------------------------------------------
ATOM_ORDER = {"gs": {}, "gs_esor_palmo": {"polar_esor": 1, "polar_gamma": 0.7, "polar_palmo": 1},
              "gs_wolf_palmo": {"polar_ewald": 0, "polar_wolf": 1, "polar_wolf_alpha": 0.13, "polar_palmo": 1}}


@pytest.mark.parametrize("case", sorted(ATOM_ORDER))
@pytest.mark.parametrize("name", [ORTHO, TRI])
def test_sweeps_in_atom_order_on_a_table_with_skipped_tile_pairs(slabs, restated, name, case):
    atoms, basis, base = slabs[name]
    o = dict(base, **ATOM_ORDER[case])
    n = len(atoms["charge"])
    want = restated((name, case, "atom order"), atoms, basis, o, order=np.arange(n))
    assert want["ranked_sweeps"] == 2 and want["polar_iterations"] == 3
    S = energy.System(atoms, basis, o)
    try:
        S.energy()
        st = S.pair_stats()
        print(f"\n{name} {case}: of {st['tile_pairs']} tile pairs: far {st['tile_pairs_far']} beyond the cutoff {st['tile_pairs_beyond_cutoff']}")
        assert st["tile_pairs"] == 171 and 4 * st["tile_pairs_far"] >= st["tile_pairs"] and 4 * st["tile_pairs_beyond_cutoff"] >= st["tile_pairs"], st
        assert S.polar_gs_ranked_info()["acted"] == 0
        against_the_restatement(S, want, o, f"{name} {case}")
    finally:
        S.close()
