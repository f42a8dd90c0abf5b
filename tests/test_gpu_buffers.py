"""The device-memory accounting of a context (mpmc_memory_usage) depends on where the context stands, not on how it got there.

Every buffer of a context grows on demand and never shrinks, and each is sized by a quantity that only rises along the sequence below
(capacity, tile count, k-vector count, number of polarizable atoms).  A context that is driven through growing sizes therefore ends
with every buffer at the size its last step needs, which is what a fresh context allocates when it is taken to that step directly:
the two must report the same bytes, and -- every kernel reading only what this evaluation wrote -- the same energies to the bit.

One buffer is sized beyond what the call at hand needs in a way that depends on the call: the field scratch of a polarizable trial move
is allocated for the longest move (MPMC_TRIAL_MAX_ATOMS atoms) at the tile count of the moment, so a one-atom move at 10 tiles fits the
scratch a one-atom move at 7 tiles left behind, and the grown context would keep the smaller one (measured: 18 432 bytes,
3 tiles x 256 x 3 doubles, fewer than the fresh context; the sizing is older than the buffer type, and DESIGN.md section 2 records it).  The quantity that sizes this buffer is the tile count times the move length, and the sequence has to be monotone in it as in the
others: the last stage therefore moves LONG_MOVE atoms at once, more than the scratch left behind holds.

No atom carries a flag that changes the LJ mixing (sigma < 0, dispersion coefficients), so the list of tile pairs left to the generic
pair kernel, whose size depends on where such atoms sit, is never allocated."""
import struct

import numpy as np
import pytest

import util
from mpmcxx_amd import energy

pytestmark = pytest.mark.gpu

N_SMALL, N_MIDDLE, N_FINAL = 192, 448, 620  # 3, 7 and 10 tiles of 64 atoms
CAPACITY_GROWN = N_MIDDLE + N_MIDDLE // 4 + 64  # what a context of N_SMALL atoms grows to when it is handed N_MIDDLE (context.cpp grow_capacity)
LONG_MOVE = 200  # atoms of the last stage's trial moves: 10 tiles x 200 > 7 tiles x MPMC_TRIAL_MAX_ATOMS (256)


def bits(x):
    return struct.pack("<d", x).hex()


def drive(S, atoms, opts, m=1):
    """one box through every path that owns growable buffers: the compact solver (tensor store, panel table, structure-factor partials),
    an accepted and a rejected trial move of m atoms (trial structure factors, field scratch), Gauss-Seidel sweeps (block store), the direct solve
    (factor, vectors, list), the compact solver again.  Returns the energies as bit patterns and the memory report after the first
    compact evaluation and at the end."""
    out = []
    S.set_options(dict(opts, solver="compact"))
    S.set_atoms(atoms)
    out.append(("compact", bits(S.energy())))
    mem_compact = S.memory_usage()
    out.append(("trial accepted", bits(S.trial_energy(5, util.moved(atoms, 5, m, seed=1)))))
    assert not S.last_trial_was_full()
    S.accept()
    out.append(("trial rejected", bits(S.trial_energy(100, util.moved(atoms, 100, m, seed=2, sigma=0.1)))))
    assert not S.last_trial_was_full()
    S.reject()
    S.set_options(dict(opts, solver="compact", polar_gs=1))
    out.append(("gauss-seidel", bits(S.energy())))
    S.set_options(dict(opts, solver="compact", polar_iterative=0))
    out.append(("direct", bits(S.energy())))
    assert S.direct_info()["status"] == 0
    S.set_options(dict(opts, solver="compact"))
    out.append(("compact again", bits(S.energy())))
    return out, mem_compact, S.memory_usage()


def test_memory_accounting_is_path_independent():
    atoms, basis, opts = util.load_fixture("ion1000_polar")
    assert not np.any(atoms["sigma"] < 0) and not np.any(atoms["has_disp"])  # no special-flag atoms: no generic tile-pair list
    cut = lambda n: {k: v[:n].copy() for k, v in atoms.items()}
    low, high = dict(opts, ewald_kmax=4), dict(opts, ewald_kmax=7)

    grown = energy.System(cut(N_SMALL), basis, dict(low, solver="compact"), max_atoms=N_SMALL)
    fresh = None
    try:
        drive(grown, cut(N_SMALL), low)
        small_total = grown.memory_usage()[0]
        drive(grown, cut(N_MIDDLE), low)  # more atoms than the capacity: the context is rebuilt with room for CAPACITY_GROWN
        middle_total = grown.memory_usage()[0]
        got = drive(grown, cut(N_FINAL), high, LONG_MOVE)  # inside that capacity: more tiles and more k vectors, every table grows in place
        assert small_total < middle_total < got[2][0], (small_total, middle_total, got[2])

        fresh = energy.System(cut(N_FINAL), basis, dict(high, solver="compact"), max_atoms=CAPACITY_GROWN)
        want = drive(fresh, cut(N_FINAL), high, LONG_MOVE)
        print("grown:", got)
        print("fresh:", want)
        assert got[0] == want[0], "energies differ between the grown and the fresh context"
        assert got[1][1] == want[1][1] > 0, ("tensor store after the compact evaluation", got[1], want[1])
        assert got[2] == want[2] and want[2][1] > 0, ("memory_usage (total, tensor store) at the end", got[2], want[2])
    finally:
        grown.close()
        if fresh is not None:
            fresh.close()
