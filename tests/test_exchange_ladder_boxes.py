"""CPU: the start boxes of test_gpu_exchange_ladder and test_gpu_exchange_chain hide nothing behind ill-conditioned components, and the step
generator of the long chain does what that test needs.

Those tests compare per component and relative, with no floor anywhere.  That is only meaningful where every compared component of the
box is well-conditioned: the oracle evaluates each start configuration (up to the sweep rung; the pair_waves box is held to the fresh
context mostly) twice, on the list as given and with the molecules listed in reverse order -- the same physics and counts, another
summation order -- and every compared component must agree within 1e-10 and be non-zero unless its term is off.  The seeds in those files
were chosen for that.  Largest order drift of a component per box (this file, -s prints them):
    single_launch  2048 atoms, cubic, rd_only            3.8e-14 (lj_pairs)
    side_stream    3456 atoms, triclinic, Ewald + FH 2   9.1e-14 (lrc_pair)
    sweep          4032 atoms, ortho, Ewald              9.2e-14 (lrc_pair)
    framework       640 atoms, ortho, Ewald              2.1e-14 (rd_energy)
    resort          512 atoms, triclinic, Ewald          3.6e-14 (coulombic_energy)
    chain           190 atoms, ortho, Ewald              6.4e-15 (rd_energy); the list the chain ends on: 1.6e-14 (energy)
"""
import numpy as np
import pytest

import test_gpu_exchange_chain as chain
import test_gpu_exchange_ladder as xl
import test_gpu_size_ladder as ladder
import util

BOXES = {rung: (lambda rung=rung: xl.start_box(rung)) for rung in xl.RUNGS if rung != "pair_waves"}
BOXES["framework"] = lambda: ladder.ladder_box(*xl.FRAMEWORK_BOX) + (ladder.options(),)
BOXES["resort"] = lambda: ladder.ladder_box(*xl.RESORT_BOX) + (ladder.options(),)
BOXES["chain"] = lambda: chain.chain_box() + (chain.OPTS,)


def reversed_molecules(atoms):
    order = np.concatenate([np.arange(a, b) for a, b in reversed(util.molecules(atoms))])
    return {k: np.asarray(v)[order] for k, v in atoms.items()}


def compared_keys(opts):
    keys = [k for k, _ in util.ENERGY_KEYS if k != "polarization_energy"]
    if opts["rd_only"]:
        keys = [k for k in keys if k not in ("coulombic_energy", "es_real", "es_recip", "es_self")]
    if opts["wolf"]:
        keys = [k for k in keys if k not in ("es_real", "es_recip", "es_self")]
    return keys


@pytest.mark.parametrize("name", list(BOXES))
def test_no_compared_component_is_ill_conditioned(name):
    from oracle import OracleSystem

    atoms, basis, opts = BOXES[name]()
    a = OracleSystem(atoms, basis, opts).energy(want_atoms=False)
    b = OracleSystem(reversed_molecules(atoms), basis, opts).energy(want_atoms=False)
    worst = (0.0, None)
    for k in compared_keys(opts):
        assert a[k] != 0.0, (name, k)
        d = abs(a[k] - b[k]) / abs(a[k])
        worst = max(worst, (d, k))
        assert d <= 1e-10, (name, k, a[k], b[k], d)
    for k in util.COUNT_KEYS + ([] if opts["rd_only"] or opts["wolf"] else ["n_es_in_cutoff"]):
        assert a[k] == b[k], (name, k)
    assert a["polarization_energy"] == 0.0
    # the classes the position-independent counts and the LRC gate tell apart are all there
    assert np.any(atoms["sigma"] < 0) and np.any(atoms["has_disp"] != 0) and np.any(atoms["epsilon"] == 0) and np.any(atoms["sigma"] == 0)
    assert np.any(atoms["charge"] == 0) and np.any(atoms["frozen"] != 0) and np.any(atoms["frozen"] == 0)
    print(f"\n{name}: n = {len(atoms['pos'])}, largest order drift {worst[0]:.1e} ({worst[1]})")


def test_chain_generator_reaches_the_resummation_and_keeps_its_band():
    resum = util.xch_resum()
    atoms, basis = chain.chain_box()
    assert atoms["epsilon"][-1] == 0.0 and atoms["charge"][-1] == 0.0  # silent in the host sums
    assert abs(len(atoms["pos"]) - 3 * 64) <= 4                        # around the three-tile edge
    exchanges, kinds, sizes = 0, {"insert": 0, "remove": 0, "move": 0}, []
    last_at_resum = None
    steps = 0
    for kind, args, trial in chain.chain_steps(atoms, basis):
        if kind != "move" and exchanges == resum:  # the list the re-summing trial sums over
            last_at_resum = {k: atoms[k][-1] for k in ("epsilon", "sigma", "charge", "frozen")}
        if kind == "remove":
            a, m = args
            assert m <= 4 and a + m < len(atoms["pos"]) and (a, a + m) in util.molecules(atoms)
        if kind == "insert":
            assert len(args[1]["pos"]) <= 4 and (args[0] < len(atoms["pos"]) or exchanges == chain.LOUD_AT_EXCHANGE)
        atoms = trial
        exchanges += kind != "move"
        kinds[kind] += 1
        sizes.append(len(atoms["pos"]))
        steps += 1
        assert chain.N_BAND[0] <= sizes[-1] <= chain.N_BAND[1], (steps, sizes[-1])
    assert steps == chain.STEPS and kind != "move"
    assert exchanges >= resum + 2, (exchanges, kinds)
    assert min(kinds.values()) > 0, kinds
    assert min(sizes) <= 192 < max(sizes) and max(sizes) > 256  # both sides of the three- and of the four-tile edge
    # the atom the re-summation ends on has a share in every host sum
    assert last_at_resum and last_at_resum["epsilon"] > 0 and last_at_resum["sigma"] > 0 and last_at_resum["charge"] != 0 and not last_at_resum["frozen"]
    # the list the chain ends on is as well-conditioned as the one it starts from
    from oracle import OracleSystem

    a = OracleSystem(atoms, basis, chain.OPTS).energy(want_atoms=False)
    b = OracleSystem(reversed_molecules(atoms), basis, chain.OPTS).energy(want_atoms=False)
    worst = max((abs(a[k] - b[k]) / abs(a[k]), k) for k in compared_keys(chain.OPTS))
    assert worst[0] <= 1e-10 and all(a[k] != 0.0 for k in compared_keys(chain.OPTS)), worst
    print(f"\nchain: {kinds}, n in [{min(sizes)}, {max(sizes)}]; end of chain: order drift {worst[0]:.1e} ({worst[1]}), "
          f"energy {a['energy']:.6g}, lj_pairs {a['lj_pairs']:.6g}, coulombic_energy {a['coulombic_energy']:.6g}")
