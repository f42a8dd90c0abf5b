"""numpy restatement of `polar_gs_ranked`: the rank pass at the end of System::pairs() (src/System.cpp:1001-1029), the bubble sort of
update_ranking (src/System.Energy.cpp:3631-3656) and the sweeps of thole_iterative (:3450-3543) in that order.  The yardstick of
tests/test_polar_gs_ranked.py (which holds it to the GS_RANKED_FIXTURES goldens) and of tests/test_gpu_polar_gs_ranked.py.

The contract, in the order the reference runs it:
  rank pass    over all pairs of atoms with polarizability != 0 (same-molecule and frozen pairs too): rmin = the smallest rimg (1e40 when
               there is no such pair); rank_metric[i] = the pairs that contain i and have r <= rmin * 1.5, r the UNWRAPPED distance.
               minimum_image (:1202-1262) in its own operation order, nothing fused: rmin is the reference's double.
  order        identity for iteration 1; behind every iteration that is followed by another the bubble sort = the stable descending
               order of rank_metric, so iterations 2, 3, ... sweep in that order
  sweeps       polar_relax_ref.solve's loop (start vector, rrms, precision test, failure at 128, blend, Palmo-Krimm) with the atoms
               taken in the sweep order
"""
import os

import numpy as np

import polar_relax_ref as rx
import polar_wolf_ref as pw
from oracle import pbc_update
from polar_direct_ref import amatrix

MAXVALUE = 1.0e40


def golden(name):
    """the reference's results of one GS_RANKED_FIXTURES box (tests/golden/polar_gs_ranked.json, .npz: gen_box.keep_gs_ranked_golden)"""
    from mpmcxx_amd import gen_box

    return gen_box.gs_ranked_golden(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"), name)


def pair_distances(pos, basis):
    """(r, rimg) [n, n] of minimum_image: d = pos_i - pos_j, img[p] = rint(sum_q R[q][p] d[q]), di[p] = d[p] - sum_q B[q][p] img[q], the
    sums from q = 0 on, r = sqrt(sum_p d[p] d[p]), rimg likewise of di (r itself where rimg is NaN)"""
    R, _, _ = pbc_update(basis)
    R, B = np.asarray(R, dtype=np.float64).reshape(3, 3), np.asarray(basis, dtype=np.float64).reshape(3, 3)
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    d = [pos[:, None, p] - pos[None, :, p] for p in range(3)]
    img = [np.rint((R[0][p] * d[0] + R[1][p] * d[1]) + R[2][p] * d[2]) for p in range(3)]
    di = [d[p] - ((B[0][p] * img[0] + B[1][p] * img[1]) + B[2][p] * img[2]) for p in range(3)]
    r = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    ri = np.sqrt((di[0] * di[0] + di[1] * di[1]) + di[2] * di[2])
    return r, np.where(np.isnan(ri), r, ri)


def rank_pass(atoms, basis):
    """(rmin, rank_metric int32 [n], order int32 [n]): order[p] = the atom swept p-th from iteration 2 on"""
    alpha = np.asarray(atoms["polarizability"], dtype=np.float64)
    n = alpha.size
    r, ri = pair_distances(atoms["pos"], basis)
    pair = (alpha[:, None] != 0.0) & (alpha[None, :] != 0.0) & ~np.eye(n, dtype=bool)
    rmin = float(ri[pair].min()) if pair.any() else MAXVALUE
    rank = (pair & (r <= rmin * 1.5)).sum(axis=1).astype(np.int32)
    return rmin, rank, np.argsort(-rank.astype(np.int64), kind="stable").astype(np.int32)


def bubble_order(rank):
    """update_ranking itself, line by line (the cases small enough for it): must equal rank_pass's stable descending order"""
    order = list(range(len(rank)))
    for _ in range(len(order)):
        done = True
        for j in range(len(order) - 1):
            if rank[order[j]] < rank[order[j + 1]]:
                order[j], order[j + 1] = order[j + 1], order[j]
                done = False
        if done:
            break
    return np.asarray(order, dtype=np.int32)


def solve(atoms, basis, opts, E0=None, order=None):
    """polar_relax_ref.solve for sweeps, with the sweep order of iterations 2, 3, ... (None: the rank pass's; the identity gives
    polar_gs).  Returns its dict and "rmin", "rank_metric", "order", "ranked_sweeps"."""
    n = int(np.asarray(atoms["pos"]).reshape(-1, 3).shape[0])
    rmin, rank, ranked = rank_pass(atoms, basis)
    order = ranked if order is None else np.asarray(order)
    E0 = rx.static_field(atoms, basis, opts) if E0 is None else E0
    E0 = np.asarray(E0, dtype=np.float64).reshape(n, 3)
    alpha = np.asarray(atoms["polarizability"], dtype=np.float64)
    scheme = rx._onoff(opts.get("polar_sor")) or rx._onoff(opts.get("polar_esor"))
    start_gamma = 1.0 if scheme else float(opts.get("polar_gamma", 1.0))
    energy = lambda mu: float(-0.5 * (mu.astype(np.longdouble) * E0.astype(np.longdouble)).sum())
    A, idx = amatrix(atoms, basis, opts)
    place = {int(a): k for k, a in enumerate(idx)}  # atom -> its block of the restricted system
    sweep = [place[int(a)] for a in order if int(a) in place]  # (contract_dipoles skips the atoms that are not polarizable, :3573)
    al = np.repeat(alpha[idx], 3)
    Aoff = A - np.diag(1.0 / al) if idx.size else A
    e0 = E0[idx].reshape(-1)
    palmo = rx._onoff(opts.get("polar_palmo"))
    prec = float(opts.get("polar_precision") or 0.0)
    want_rrms = rx._onoff(opts.get("polar_rrms")) or prec > 0
    max_iter = int(opts.get("polar_max_iter", 10))
    x = al * e0 * start_gamma
    ind, change = np.zeros_like(x), np.zeros_like(x)
    it, failed, rrms, contractions, ranked_sweeps = 0, 0, 0.0, 0, 0
    while True:
        it += 1
        if it >= rx.MAX_ITERATION_COUNT and prec:
            x, failed = al * e0, 1
            change = np.zeros_like(x)
            break
        old = x.copy()
        for b in (range(idx.size) if it == 1 else sweep):  # one atom at a time with the dipoles swept so far
            k = 3 * b
            ind[k:k + 3] = -(Aoff[k:k + 3] @ x)
            x[k:k + 3] = al[k:k + 3] * (e0[k:k + 3] + ind[k:k + 3])
        new = x.copy()
        ranked_sweeps += 1 if it > 1 else 0
        contractions += 1
        if want_rrms:
            rrms = rx._rrms(new, old, n)
        done = (it == max_iter) if prec == 0.0 else not np.any((new - old) ** 2 > (prec * rx.DEBYE2SKA) ** 2)
        if done and palmo:  # in front of the blend: the swept dipoles
            change = -(Aoff @ new) - ind
            contractions += 1
        x = rx.blend(rx.weights(opts, it), new, old)
        if done:
            break
    mu = pw._scatter(x, idx, n)
    corr = float(-0.5 * (x.astype(np.longdouble) * change.astype(np.longdouble)).sum())
    return {"ef_static": E0, "mu": mu, "ef_induced": pw._scatter(ind, idx, n), "polarization_energy": energy(mu) + corr, "correction": corr,
            "polar_iterations": it, "iterator_failed": failed, "dipole_rrms": rrms, "contractions": contractions, "rmin": rmin, "rank_metric": rank,
            "order": ranked, "ranked_sweeps": ranked_sweeps}
