"""numpy restatement of the reference's cavity-bias grid (System::cavity_update_grid, update_cavity_probability, update_cavity_volume,
is_point_empty: src/System.Cavity.cpp:15-188) and of the ENSEMBLE_UVT branch of System::boltzmann_factor (src/System.MonteCarlo.cpp:1358-1422),
the comparison partner of tests/test_cavity.py and tests/test_gpu_cavity.py.

float64 throughout, one rounded operation per reference operation, in the reference's operand order; distances are compared as the reference
compares them, `sqrt(r) < radius`, not through a threshold on r.  The loops over sphere centres and darts are Python loops; the loop over the
atoms (respectively the empty centres) of one of them is a numpy vector, element by element the same IEEE operations (numpy's sqrt of a
float64 is the correctly rounded one, as math.sqrt's: test_cavity.py checks the two against each other).  The wrapped atom positions are an
input: the tests take them from System.update_com."""
import math

import numpy as np

ATM2REDUCED = 0.0073389366
DARTSCALE = 0.1
INSERT, REMOVE, DISPLACE = 0, 1, 2


def num_darts(volume):
    return int(volume * DARTSCALE)


def grid_point(basis, G, i, j, k):
    """one sphere centre with Python floats (cavity_update_grid :44-58)"""
    comp = [float(i + 1) / float(G + 1), float(j + 1) / float(G + 1), float(k + 1) / float(G + 1)]
    v = [0.0, 0.0, 0.0]
    for p in range(3):
        v[p] = 0.0
        for q in range(3):
            v[p] += float(basis[q][p]) * comp[q]
    for p in range(3):
        for q in range(3):
            v[p] -= 0.5 * float(basis[q][p])
    return v


def grid_points(basis, G):
    """(G^3, 3) sphere centres in enumeration order (i outermost, k innermost): the same operations as grid_point, a vector over the centres"""
    basis = np.asarray(basis, dtype=np.float64)
    idx = np.arange(G, dtype=np.float64)
    c = (idx + 1.0) / float(G + 1)
    comp = [a.reshape(-1) for a in np.meshgrid(c, c, c, indexing="ij")]
    out = np.zeros((G ** 3, 3))
    for p in range(3):
        v = np.zeros(G ** 3)
        for q in range(3):
            v = v + basis[q][p] * comp[q]
        for q in range(3):
            v = v - 0.5 * basis[q][p]
        out[:, p] = v
    return out


def occupancy(grid, wrapped_pos, radius):
    """atoms inside the sphere of every centre (a count), :61-74"""
    w = np.asarray(wrapped_pos, dtype=np.float64)
    occ = np.zeros(len(grid), dtype=np.int32)
    for g in range(len(grid)):
        r = np.zeros(len(w))
        for p in range(3):
            d = grid[g, p] - w[:, p]
            r = r + d * d
        occ[g] = int(np.count_nonzero(np.sqrt(r) < radius))
    return occ


def dart_positions(basis, dart_frac):
    """update_cavity_volume :142-148"""
    basis = np.asarray(basis, dtype=np.float64)
    f = np.asarray(dart_frac, dtype=np.float64).reshape(-1, 3)
    pos = np.zeros((len(f), 3))
    for p in range(3):
        v = np.zeros(len(f))
        for q in range(3):
            v = v + basis[q][p] * f[:, q]
        pos[:, p] = v
    return pos


def dart_hits(grid, open_index, darts, radius):
    """per dart: inside some empty sphere (is_point_empty :165-188; pow(d, 2) is d * d exactly)"""
    og = grid[open_index]
    hit = np.zeros(len(darts), dtype=bool)
    for t in range(len(darts)):
        if len(og) == 0:
            break
        r = np.zeros(len(og))
        for p in range(3):
            d = darts[t, p] - og[:, p]
            r = r + d * d
        hit[t] = bool(np.any(np.sqrt(r) < radius))
    return hit


def update(basis, volume, wrapped_pos, G, radius, dart_frac):
    """one cavity_update_grid: everything mpmc_cavity_update and mpmc_cavity_get return"""
    grid = grid_points(basis, G)
    occ = occupancy(grid, wrapped_pos, radius)
    open_index = np.flatnonzero(occ == 0).astype(np.int32)
    n_open, total = int(len(open_index)), G ** 3
    f = np.zeros((0, 3)) if dart_frac is None else np.asarray(dart_frac, dtype=np.float64).reshape(-1, 3)
    hit = dart_hits(grid, open_index, dart_positions(basis, f), radius)
    hits, n_darts = int(np.count_nonzero(hit)), int(len(f))
    with np.errstate(invalid="ignore", divide="ignore"):
        fraction = np.float64(hits) / np.float64(n_darts)  # (0 darts: 0 / 0, NaN, as in the reference)
    return {"grid": grid, "occupancy": occ, "open_index": open_index, "total_points": total, "cavities_open": n_open, "n_darts": n_darts, "hits": hits,
            "hit": hit, "probability": float(n_open) / float(total), "cavity_volume": float(fraction * np.float64(volume))}


def insertion_index(cavities_open, u):
    """random_index of make_move (src/System.MonteCarlo.cpp:759); rint rounds half to even, as Python's round does"""
    return (cavities_open - 1) - int(round(float(cavities_open - 1) * u))


def uvt_boltzmann_factor(movetype, biased, temperature, fugacity, volume, N, init_energy, final_energy, sorbate_count, cavity_volume, avg_probability):
    delta_energy = final_energy - init_energy
    if biased:
        if movetype == INSERT:
            return (cavity_volume * avg_probability * fugacity * ATM2REDUCED / (temperature * N)) * math.exp(-delta_energy / temperature) * float(sorbate_count)
        if movetype == REMOVE:
            return (temperature * (N + 1.0)) / (cavity_volume * avg_probability * fugacity * ATM2REDUCED) * math.exp(-delta_energy / temperature) / float(sorbate_count)
    else:
        if movetype == INSERT:
            return volume * fugacity * ATM2REDUCED / (temperature * float(N)) * math.exp(-delta_energy / temperature) * float(sorbate_count)
        if movetype == REMOVE:
            return temperature * (float(N) + 1.0) / (volume * fugacity * ATM2REDUCED) * math.exp(-delta_energy / temperature) / float(sorbate_count)
    if movetype == DISPLACE:
        return math.exp(-delta_energy / temperature)
    raise ValueError(movetype)


def mt19937_uniforms(count, seed=5489):
    """`count` draws of std::uniform_real_distribution<double>(0, 1) from a std::mt19937 seeded with `seed` (5489: default constructed), as
    libstdc++ makes them: two 32-bit outputs per double, (lo + hi * 2^32) / 2^64 with the sum rounded to double, 1.0 replaced by the double below"""
    import random

    mt = [0] * 624
    mt[0] = seed & 0xFFFFFFFF
    for i in range(1, 624):
        mt[i] = (1812433253 * (mt[i - 1] ^ (mt[i - 1] >> 30)) + i) & 0xFFFFFFFF
    r = random.Random()
    r.setstate((3, tuple(mt) + (624,), None))
    out = np.zeros(count)
    for t in range(count):
        lo, hi = r.getrandbits(32), r.getrandbits(32)
        s = float(lo) + float(hi) * 4294967296.0
        v = s / 18446744073709551616.0
        out[t] = v if v < 1.0 else math.nextafter(1.0, 0.0)
    return out
