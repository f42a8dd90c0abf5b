"""GPU (MI355X): the dipole-solve variants that came after the base path -- `polar_ewald_full` (kernels_ewald_full.hip), the Wolf static
field (kernels_wolf_field.hip), the relaxed Jacobi updates of `polar_sor` / `polar_esor` and `polar_zodid` -- at ragged sizes and on the
slab boxes.  Their own GPU test files run cubes of 2, 192, 216, 1000 and 4000 atoms in which nearly every atom is a polarizable ion.

Boxes and variants: tests/polar_ragged_boxes.py; their preconditions (conditioning, empty tile pairs, non-polarizable atoms in the last
tile) are asserted on the CPU by tests/test_polar_ragged_preconditions.py.
  ragged rungs  1, 2, 63, 64, 65, 128, 129 (the first size the spatial order permutes), 257 (k_pef_sf strides by 256), 512 and 513 atoms (nine
                tiles: a wave of k_pef_finish takes a second slot) of test_gpu_random's heterogeneous mix
  slab rungs    1089 atoms in 18 tiles: tile pairs beyond the cutoff (k_pef_fill's CLS_BEYOND_CUTOFF return and k_pef_contract's zero
                slots) under the spatial order and in list order, Thole far panels under the relaxed Jacobi update, the panel table built on
                the side stream, precision-terminated solves whose pass count must be the restatement's; list edits on one context, so
                that a cnt, store or part slot of the list before would be read (a fresh context's memory reads as zeros: a kernel that
                never wrote cnt on the beyond-cutoff return passed every test on fresh contexts)
Yardsticks: the numpy restatements polar_ewald_full_ref, polar_relax_ref and polar_wolf_ref with the bounds of each variant's own GPU test
file (imported below): the energy relative, the per-atom arrays within 1e-9 + margin of the array's largest component, every count exact;
the other energy components against the oracle with polarization off at util.REL_TOL.  A lone atom's field is the rounding residue of a
cancellation: test_gpu_random.check's absolute floors (1e-12 on the fields, 3 alpha 1e-24 on the energies).  Run with -s for the measured
deviations.

As measured on an MI355X (largest over the rungs: energy relative / ef_static / mu / ef_induced as fractions of their largest component):
  pef             1.3e-12 / 1.8e-12 / 3.8e-12 / 4.0e-12        pef_sor         2.5e-12 / 1.8e-12 / 6.3e-12 / 6.6e-12
  jac_sor         1.4e-11 / 1.8e-12 / 3.4e-11 / 3.5e-11        zodid           1.6e-14 / 1.8e-12 / 2.9e-12 / 0
  wolf_jac        2.2e-11 / 9.4e-14 / 2.0e-11 / 1.9e-11        wolf_gsp        4.6e-11 / 9.4e-14 / 3.9e-11 / 4.1e-11, correction 4.6e-11 |U_pol|
  pef_prec        1.1e-15 / 2.1e-15 / 2.4e-15 / 2.4e-15        pef_esor_prec   8.4e-16 / 2.1e-15 / 2.2e-15 / 2.9e-15
  jac_esor_prec   3.7e-15 / 2.1e-15 / 2.5e-13 / 1.1e-12
  (the fixed-count variants are largest at 128 atoms, ef_static at 65; on the slabs every variant sits at 1e-15 but for mu and ef_induced
  under Jacobi, 2e-13 and 1e-12 with the spatial order, 4e-13 and 2e-12 in list order).  Precision-terminated on the slabs, orthorhombic
  and triclinic: pef_prec 7 and 8 passes, pef_esor_prec 8 and 9, jac_esor_prec 8 and 9 iterations, as the restatement.  Tile stats of the
  slabs, of 171 tile pairs: 5 beyond the cutoff and 5 thole_far with the spatial order, 76 and 76 in list order.
"""
import numpy as np
import pytest

import util
import polar_ragged_boxes as B
import test_gpu_polar_ewald_full as PEF
import test_gpu_polar_relax as RX
import test_gpu_polar_wolf as PW
from test_polar_relax import WORST as RX_WORST
from mpmcxx_amd import energy

pytestmark = pytest.mark.gpu

REL = util.REL_TOL
ARRAYS = ("ef_static", "mu", "ef_induced")
# (energy, {array: bound as a fraction of its largest component}) per restatement: 1e-9 plus the restatement's own margin, as each file has it
BOUNDS = {"pef": (PEF.REF_REL_E, {k: PEF.REF_REL_F for k in ARRAYS}),
          "relax": (RX.REF_REL_E, {k: REL + 10.0 * RX_WORST[k] for k in ARRAYS}),
          "wolf": (PW.REF_REL, {k: PW.REF_REL for k in ARRAYS})}
OTHER_KEYS = [k for k, _ in util.ENERGY_KEYS if k not in ("energy", "polarization_energy")]
SEEN = {}  # variant -> {quantity: largest deviation over the comparisons of this module}, printed when the module is done


@pytest.fixture(scope="module", autouse=True)
def _need_device():
    if energy.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests need an MI355X")


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for variant in B.VARIANTS:  # (with -s: the record in the docstring)
        if variant in SEEN:
            print(f"\nlargest, {variant}: " + " ".join(f"{k} {v:.1e}" for k, v in SEEN[variant].items()))


def snapshot(S):
    return dict(S.observables), [x.copy() for x in S.dipoles()]


def same_bits(a, b):
    return a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))


def store_bytes(n):
    nt = -(-n // B.TILE)
    return nt * (nt + 1) // 2 * 64 * 64 * 16


def against_the_restatement(S, atoms, o, variant, want, label, pef_box=None, largest=None):
    """one evaluated System against the restatement's `want`; pef_box: {"n_real_pairs", "n_k"} of the box for the polar_ewald_full variants;
    largest: the longest list the context has held (its buffers only grow: store_bytes is what the device holds), the list itself if None"""
    fam = B.FAMILY[variant]
    rel_e, rel_f = BOUNDS[fam]
    n = len(atoms["charge"])
    alpha = np.asarray(atoms["polarizability"])
    lone = n == 1
    floor_f = 1e-12 if lone else 0.0
    floor_e = 3.0 * float(alpha.max()) * 1e-24 if lone else 0.0
    obs = S.observables
    mu, E0, F = S.dipoles()
    fails, devs = [], {}
    u = want["polarization_energy"]
    du = abs(obs["polarization_energy"] - u)
    devs["energy"] = du / abs(u) if u else du
    if not du <= rel_e * abs(u) + floor_e:
        fails.append(("polarization_energy", obs["polarization_energy"], u))
    for k, got in zip(ARRAYS, (E0, mu, F)):
        top = float(np.abs(want[k]).max())
        d = float(np.abs(got - want[k]).max())
        devs[k] = d / top if top else d
        if not d <= rel_f[k] * top + floor_f:
            fails.append((k, d, top))
    # counts
    assert obs["iterator_failed"] == want["iterator_failed"] == 0, (label, obs["iterator_failed"], want["iterator_failed"])
    assert obs["polar_iterations"] == want["polar_iterations"], (label, obs["polar_iterations"], want["polar_iterations"])
    counts = f"iterations {obs['polar_iterations']}"
    if o.get("polar_ewald_full"):
        info = S.ewald_full_info()
        assert info["passes"] == want["passes"], (label, info, want["passes"])
        if not o.get("polar_precision"):
            assert info["passes"] == o["polar_max_iter"] + 1, (label, info)
        assert info["n_real_pairs"] == pef_box["n_real_pairs"] and info["n_k"] == pef_box["n_k"] == B.N_K[o["ewald_kmax"]], (label, info, pef_box)
        assert info["store_bytes"] == store_bytes(largest or n), (label, info)
        counts = f"passes {info['passes']} real pairs {info['n_real_pairs']} k vectors {info['n_k']}"
    if o.get("polar_palmo"):
        corr = S.palmo_info()[0]
        devs["palmo"] = abs(corr - want["correction"]) / abs(u) if u else abs(corr - want["correction"])
        if lone:  # (one atom has nothing to sweep against: the correction is zero to the bit on both sides)
            assert corr == want["correction"] == 0.0, (label, corr, want["correction"])
        elif not (abs(corr - want["correction"]) <= REL * abs(u) and want["correction"] != 0.0 and corr != 0.0):
            fails.append(("palmo", corr, want["correction"]))
    print(f"\n{label}: {counts} " + " ".join(f"{k} {v:.1e}" for k, v in devs.items()))
    if not fails and not lone:  # (a lone atom's deviations are rounding residues over rounding residues: no record)
        seen = SEEN.setdefault(variant, {})
        for k, v in devs.items():
            seen[k] = max(seen.get(k, 0.0), v)
    assert not fails, (label, fails)
    assert not np.any(np.asarray(mu)[alpha == 0.0]), f"{label}: a dipole on an atom with alpha == 0"
    return floor_e


def against_the_oracle_without_polarization(S, ref, want_u, floor_e, label):
    """every component but the polarization energy at util.REL_TOL with no floor, the pair counts exactly; the total is their sum with the
    polarization energy, each part within REL_TOL of its yardstick"""
    obs = S.observables
    bad = util.component_errors(obs, ref, OTHER_KEYS, REL)
    assert not bad, f"{label}: against the oracle without polarization: " + "; ".join(bad)
    for k in util.COUNT_KEYS + ["n_es_in_cutoff"]:
        assert int(obs[k]) == int(ref[k]), (label, k, obs[k], ref[k])
    assert abs(obs["energy"] - (ref["energy"] + want_u)) <= REL * (abs(ref["energy"]) + abs(want_u)) + floor_e, (label, obs["energy"], ref["energy"], want_u)


def pef_box_of(rung):
    want = B.restated(rung, "pef")
    return {"n_real_pairs": want["n_real_pairs"], "n_k": want["n_k"]}


def evaluate(rung, variant, label, check=None, configure=()):
    """one context, one energy(), held to the restatement and to the oracle; check(S): what the caller asserts on the live context"""
    atoms, basis, _ = B.box(rung)
    o = B.options(rung, variant)
    want = B.restated(rung, variant)
    pef_box = pef_box_of(rung) if o.get("polar_ewald_full") else None
    S = energy.System(atoms, basis, o)
    try:
        for key, value in configure:
            S.configure(key, value)
        S.energy()
        floor_e = against_the_restatement(S, atoms, o, variant, want, label, pef_box)
        against_the_oracle_without_polarization(S, B.oracle_without_polarization(rung), want["polarization_energy"], floor_e, label)
        return check(S) if check else None
    finally:
        S.close()


# ---- A. one test per (rung, variant) --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,variant", [c for c in B.CASES if c[0] in B.RAGGED])
def test_ragged_rung(n, variant):
    evaluate(n, variant, f"n = {n} {variant}")


@pytest.mark.parametrize("name,variant", [c for c in B.CASES if c[0] in B.SLABS])
def test_slab_rung(name, variant):
    """with the spatial order (the default): under `pef` the table has tile pairs beyond the cutoff, which k_pef_fill returns from early"""

    def check(S):
        st = S.tile_stats()
        print(f"{name} {variant}: tile stats {st}")
        if variant == "pef":
            assert st["tile_pairs"] == 171 and st["beyond_cutoff"] > 0, st

    evaluate(name, variant, f"{name} {variant}", check)


# ---- B. the slab rungs: list order, the side stream, repeats ----------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["pef", "jac_sor"])
@pytest.mark.parametrize("name", B.SLABS)
def test_slab_rung_in_list_order(name, variant):
    """spatial_sort = 0: the tiles are the slabs of the list, 98 off-diagonal tile pairs of 171 hold no pair inside the polar_ewald_full
    predicate (test_polar_ragged_preconditions); jac_sor's AUTO solver is the compact store with panels at six iterations"""

    def check(S):
        st = S.tile_stats()
        print(f"{name} {variant} in list order: tile stats {st}")
        assert st["tile_pairs"] == 171 and st["beyond_cutoff"] > 0, st
        if variant == "jac_sor":
            assert st["thole_far"] > 0 and S.polar_relax_info()["store_filled"] == 1, (st, S.polar_relax_info())

    energy.configure("spatial_sort", 0)  # (for the contexts created from here on)
    try:
        evaluate(name, variant, f"{name} {variant} in list order", check)
    finally:
        energy.configure("spatial_sort", 1)


@pytest.mark.parametrize("name", B.SLABS)
def test_panel_table_on_the_side_stream(name):
    """side_stream = 1 builds the panel table of the relaxed Jacobi solve on the side stream at 18 tiles; the choice of streams does not
    touch the arithmetic (plan_evaluation): the bits of the run without the switch"""
    got = []
    for mode in ((), (("side_stream", 1),)):
        got.append(evaluate(name, "jac_sor", f"{name} jac_sor side_stream {dict(mode).get('side_stream', 'by size')}", snapshot, configure=mode))
    assert same_bits(got[0], got[1])


@pytest.mark.parametrize("variant", ["pef", "jac_sor"])
@pytest.mark.parametrize("name", B.SLABS)
def test_a_second_evaluation_gives_the_same_bits(name, variant):
    atoms, basis, _ = B.box(name)
    S = energy.System(atoms, basis, B.options(name, variant))
    try:
        S.energy()
        first = snapshot(S), S.ewald_full_info() if variant == "pef" else None
        S.energy()
        assert same_bits(first[0], snapshot(S)) and first[1] == (S.ewald_full_info() if variant == "pef" else None)
    finally:
        S.close()


@pytest.mark.parametrize("name", B.SLABS)
def test_slab_in_list_order_after_a_list_that_filled_every_tile_pair(name):
    """One context in list order under `pef`: first the slab's molecules in a shuffled order, so that every tile spans the cell, no tile
    pair lies beyond the cutoff and every cnt and store slot is written; then the slab's own list, whose 76 tile pairs beyond the cutoff
    must read as empty although their slots hold the shuffled list's counts and factors.  Nothing is sorted, so the second result is a fresh
    context's to the bit, and it is held to the restatement as above."""
    atoms, basis, _ = B.box(name)
    o = B.options(name, "pef")
    mols = util.molecules(atoms)
    order = np.concatenate([np.arange(*mols[m]) for m in np.random.default_rng(11).permutation(len(mols))])
    shuffled = {k: np.array(v[order]) for k, v in atoms.items()}
    energy.configure("spatial_sort", 0)
    try:
        S, F = energy.System(shuffled, basis, o), energy.System(atoms, basis, o)
    finally:
        energy.configure("spatial_sort", 1)
    try:
        S.energy()
        assert S.tile_stats()["beyond_cutoff"] == 0 and S.ewald_full_info()["n_real_pairs"] == pef_box_of(name)["n_real_pairs"], S.tile_stats()
        S.set_atoms(atoms)
        S.energy()
        F.energy()
        assert S.tile_stats()["beyond_cutoff"] > 0 and S.tile_stats() == F.tile_stats(), (S.tile_stats(), F.tile_stats())
        against_the_restatement(S, atoms, o, "pef", B.restated(name, "pef"), f"{name} pef in list order after the shuffled list", pef_box_of(name))
        assert same_bits(snapshot(S), snapshot(F)) and S.ewald_full_info() == F.ewald_full_info(), "against a fresh context"
    finally:
        S.close(), F.close()


# ---- C. list edits on one context ------------------------------------------------------------------------------------------------------------
def test_list_edits_under_polar_ewald_full():
    """set_atoms through 63, 65 and 63 atoms (prefixes of the 65-atom rung), then 128, 129 and 128 (prefixes of the 129-atom rung) on ONE
    context: a store, cnt or part slot that survives a shrink would be read by the next evaluation.  Up to 128 atoms nothing is sorted, so
    each result is a fresh context's to the bit; at 129 the carried order may differ from a fresh sort, so from the first 129-atom list on
    each result is held to the restatement at the bounds above."""
    small, sbasis, _ = B.box(65)
    big, bbasis, _ = B.box(129)
    o65, o129 = B.options(65, "pef"), B.options(129, "pef")
    S = energy.System(B.prefix(small, 63), sbasis, o65)
    largest = 0
    try:
        for step, m in enumerate((63, 65, 63)):
            atoms = B.prefix(small, m)
            if step:
                S.set_atoms(atoms)
            S.energy()
            F = energy.System(atoms, sbasis, o65)
            try:
                F.energy()
                assert same_bits(snapshot(S), snapshot(F)), f"step {step}: {m} atoms against a fresh context"
                largest = max(largest, m)  # (the store only grows: after the shrink it is still the 65-atom list's)
                assert S.ewald_full_info() == dict(F.ewald_full_info(), store_bytes=store_bytes(largest)), (step, S.ewald_full_info(), F.ewald_full_info())
            finally:
                F.close()
        S.set_box(bbasis)
        S.set_options(o129)
        kept = {}
        for step, m in enumerate((128, 129, 128)):
            atoms = B.prefix(big, m)
            S.set_atoms(atoms)
            S.energy()
            if m not in kept:
                E0 = B.static_field(atoms, bbasis, o129)
                kept[m] = B.solve("pef", atoms, bbasis, o129, E0)
            want = kept[m]
            largest = max(largest, m)
            against_the_restatement(S, atoms, o129, "pef", want, f"list edit {step}: {m} atoms", {"n_real_pairs": want["n_real_pairs"], "n_k": want["n_k"]}, largest)
    finally:
        S.close()
