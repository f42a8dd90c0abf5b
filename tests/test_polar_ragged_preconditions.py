"""CPU: the preconditions of tests/test_gpu_polar_ragged_ladder.py.  Conditions on its inputs (tests/polar_ragged_boxes.py), checked
with the numpy restatements alone, before any device runs.

  conditioning       every (box, variant) of the ladder: the restatement's own static field E0, perturbed by a relative 1e-13 of seeded
                     normal noise, moves mu and ef_induced by at most CAP * 1e-13 of their largest component and polarization_energy by at
                     most CAP * 1e-13 relative, and the pass / iteration count by nothing.  A comparison at 1e-9 of a solve that amplified
                     rounding a million times would say nothing; at this damping the random mix does so from about ten Jacobi iterations
                     on, which is why the ladder's counts are three to six.  Run with -s for the measured factors.
  empty tile pairs   each slab rung in list order has off-diagonal tile pairs without a pair inside the polar_ewald_full predicate
                     (99 of 171 tile pairs on both cells, 98 of the 99 off the diagonal): k_pef_contract's zero-publishing branch
  non-polarizable    every ragged rung from 63 atoms on has alpha == 0 and alpha != 0 atoms in its last tile; where that tile holds one
                     atom it is the kind polar_ragged_boxes.LONE_ATOM_POLARIZABLE says and the tile in front of it has both
"""
import numpy as np
import pytest

import polar_ragged_boxes as B

EPS = 1e-13
CAP = 100.0  # the issue's cap on the amplification; a seed that broke it would be replaced, the cap stays


@pytest.mark.parametrize("rung,variant", B.CASES)
def test_conditioning(rung, variant):
    atoms, basis, _ = B.box(rung)
    o = B.options(rung, variant)
    E0 = B.field_of(rung, variant)
    base = B.restated(rung, variant)
    noise = np.random.default_rng(977).normal(size=E0.shape)
    moved = B.solve(variant, atoms, basis, o, E0 * (1.0 + EPS * noise))
    factors = {}
    for k in ("mu", "ef_induced"):
        top = float(np.abs(base[k]).max())
        d = float(np.abs(moved[k] - base[k]).max())
        factors[k] = d / (EPS * top) if top else (0.0 if d == 0.0 else float("inf"))
    u = base["polarization_energy"]
    du = abs(moved["polarization_energy"] - u)
    factors["energy"] = du / (EPS * abs(u)) if u else (0.0 if du == 0.0 else float("inf"))
    print(f"\n{rung} {variant}: " + " ".join(f"{k} {v:.2f}" for k, v in factors.items()))
    for k in ("polar_iterations", "passes", "iterator_failed"):
        assert moved.get(k) == base.get(k), (rung, variant, k, moved.get(k), base.get(k))
    assert base["iterator_failed"] == 0 and np.isfinite(u), (rung, variant)
    assert max(factors.values()) <= CAP, (rung, variant, factors)


@pytest.mark.parametrize("name", B.SLABS)
def test_slab_has_empty_tile_pairs_in_list_order(name):
    atoms, basis, _ = B.box(name)
    pairs, empty, off = B.empty_tile_pairs(B.predicate(atoms, basis, B.options(name, "pef")))
    print(f"\n{name}: {empty} of {pairs} tile pairs hold no pair inside the predicate, {off} of them off the diagonal")
    assert pairs == 171 and off >= 1, (name, pairs, empty, off)


@pytest.mark.parametrize("n", [n for n in B.RAGGED if n >= 63])
def test_last_tile_has_both_kinds_of_atoms(n):
    al = B.box(n)[0]["polarizability"]
    first = B.TILE * ((n - 1) // B.TILE)
    last = al[first:]
    if last.size == 1:  # one atom cannot be both: it is the kind the ladder wants at this size, and the tile in front of it has both
        assert (last[0] != 0.0) == B.LONE_ATOM_POLARIZABLE[n], (n, last)
        last = al[first - B.TILE:first]
    assert np.any(last == 0.0) and np.any(last != 0.0), (n, last)


@pytest.mark.parametrize("n", [n for n in B.RAGGED if n <= 2])
def test_smallest_rungs_are_polarizable(n):
    assert np.all(B.box(n)[0]["polarizability"] != 0.0)
