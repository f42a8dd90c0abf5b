"""CPU (numpy): the polarization energy of n Jacobi iterations from the moments of the first ceil(n/2) dipole differences.

With mu_0 = alpha E0, mu_(k+1) = alpha (E0 - T mu_k), d_0 = mu_0 and d_k = mu_k - mu_(k-1) = (-alpha T)^k alpha E0 (T symmetric, alpha
diagonal): E0 . mu_n = sum_{k=0..n} m_k with m_2a = <d_a, d_a>_{1/alpha}, m_2a+1 = <d_a, d_a+1>_{1/alpha}; for a = 0 the weight d_0 / alpha
is E0 itself, atoms with alpha = 0 drop out (the kernel: k_polar_moments, csrc/kernels.hip).

Tolerance: none guessed.  `moment_error_bound` follows the rounding of both sides through the recursion:
  - the computed mu_k carries e_k <= |alpha| |T| e_(k-1) + (L + 3) eps mubar_k, L = 3N the length of a row of T (a dot product of L terms, one
    addition, one multiplication), mubar_k the same recursion on absolute values;
  - the computed d_k carries f_k <= e_k + e_(k-1) + eps (|mu_k| + |mu_(k-1)|);
  - a moment is a dot product of L terms (three roundings more per term for the weight and the product) of perturbed vectors:
    |dm_(a+b)| <= sum_i (f_a |d_b| + |d_a| f_b + f_a f_b)_i / alpha_i + (L + 3) eps sum_i |d_a d_b|_i / alpha_i;
  - the n + 1 moments are added in sequence: n eps sum_k |m_k|;
  - the plain side: sum_i |E0_i| e_n,i + (L + 1) eps sum_i |E0 mu_n|_i.
Run with -s for the measured deviation next to its bound."""
import numpy as np
import pytest

EPS = np.finfo(float).eps
N_ATOMS = 40


def random_system(seed, n_atoms=N_ATOMS):
    """symmetric T with zero diagonal 3 x 3 blocks, scaled so that the iteration contracts; diagonal alpha with zeros; a static field"""
    rng = np.random.default_rng(seed)
    L = 3 * n_atoms
    T = rng.normal(size=(L, L))
    T = 0.5 * (T + T.T)
    for i in range(n_atoms):
        T[3 * i:3 * i + 3, 3 * i:3 * i + 3] = 0.0
    alpha_atom = rng.uniform(0.5, 2.0, n_atoms)
    alpha_atom[rng.choice(n_atoms, n_atoms // 5, replace=False)] = 0.0
    alpha = np.repeat(alpha_atom, 3)
    T *= 0.6 / np.abs(np.linalg.eigvals(alpha[:, None] * T)).max()
    return T, alpha, rng.normal(size=L)


def plain_energy(T, alpha, E0, n):
    mu = alpha * E0
    for _ in range(n):
        mu = alpha * (E0 + (-(T @ mu)))
    return -0.5 * float(E0 @ mu), mu


def dipole_differences(T, alpha, E0, count):
    """d_0 .. d_count the way the update kernels record them: new_mu - mu_old of the plain iteration"""
    mu = alpha * E0
    d = [mu.copy()]
    for _ in range(count):
        new = alpha * (E0 + (-(T @ mu)))
        d.append(new - mu)
        mu = new
    return d


def moment_energy(d, alpha, E0, n):
    """(-1/2 sum m_k, the moments) in the kernel's order: ascending k, the weight of a = 0 is E0, alpha = 0 skipped"""
    live = alpha != 0.0
    m = []
    for k in range(n + 1):
        a, b = k // 2, (k + 1) // 2
        w = E0[live] if a == 0 else d[a][live] / alpha[live]
        m.append(float(np.sum(w * d[b][live])))
    u = 0.0
    for v in m:
        u += v
    return -0.5 * u, m


def moment_error_bound(T, alpha, E0, n):
    """|moment energy - plain energy| <= this, by the derivation in the module docstring"""
    L = E0.size
    aT, aE, aa = np.abs(T), np.abs(E0), np.abs(alpha)
    live = alpha != 0.0
    mubar = [aa * aE]
    e = [EPS * mubar[0]]
    mus = [alpha * E0]
    for _ in range(n):
        mubar.append(aa * (aE + aT @ mubar[-1]))
        e.append(aa * (aT @ e[-1]) + (L + 3) * EPS * mubar[-1])
        mus.append(alpha * (E0 + (-(T @ mus[-1]))))
    half = (n + 1) // 2
    d = dipole_differences(T, alpha, E0, half)
    f = [e[0]] + [e[k] + e[k - 1] + EPS * (np.abs(mus[k]) + np.abs(mus[k - 1])) for k in range(1, half + 1)]
    inv = np.zeros(L)
    inv[live] = 1.0 / aa[live]
    total, sum_abs_m = 0.0, 0.0
    for k in range(n + 1):
        a, b = k // 2, (k + 1) // 2
        da, db = np.abs(d[a]), np.abs(d[b])
        total += float(np.sum((f[a] * db + da * f[b] + f[a] * f[b]) * inv)) + (L + 3) * EPS * float(np.sum(da * db * inv))
        sum_abs_m += abs(float(np.sum(d[a] * d[b] * inv)))
    total += n * EPS * sum_abs_m
    total += float(np.sum(aE * e[n])) + (L + 1) * EPS * float(np.sum(aE * np.abs(mus[n])))
    return 0.5 * total, sum_abs_m


@pytest.mark.parametrize("n", range(1, 12))
def test_moment_sum_equals_plain_recursion(n):
    for seed in (1, 2, 3):
        T, alpha, E0 = random_system(seed)
        u_plain, _ = plain_energy(T, alpha, E0, n)
        d = dipole_differences(T, alpha, E0, (n + 1) // 2)
        u_mom, m = moment_energy(d, alpha, E0, n)
        bound, sum_abs_m = moment_error_bound(T, alpha, E0, n)
        print(f"n={n} seed={seed}: |moments - plain| {abs(u_mom - u_plain):.2e}, bound {bound:.2e} (rel {bound / abs(u_plain):.1e}), sum|m_k| {sum_abs_m:.3e}")
        assert len(m) == n + 1 and len(d) == (n + 1) // 2 + 1
        assert abs(u_mom - u_plain) <= bound, (n, seed, u_mom, u_plain, abs(u_mom - u_plain), bound)


def test_atoms_without_polarizability_drop_out():
    T, alpha, E0 = random_system(7)
    d = dipole_differences(T, alpha, E0, 5)
    assert all(not np.any(v[alpha == 0.0]) for v in d)
    u10, _ = moment_energy(d, alpha, E0, 10)
    E0_other = E0.copy()
    E0_other[alpha == 0.0] += 3.0  # the field on an atom that cannot polarize changes nothing
    d2 = dipole_differences(T, alpha, E0_other, 5)
    assert moment_energy(d2, alpha, E0_other, 10)[0] == u10


def test_odd_and_even_counts_need_the_same_ring():
    """n = 2h - 1 and n = 2h read d_0 .. d_h: the ring holds ceil(n/2) + 1 vectors"""
    T, alpha, E0 = random_system(11)
    for n in (1, 2, 3, 10):
        h = (n + 1) // 2
        d = dipole_differences(T, alpha, E0, h)
        _, m = moment_energy(d, alpha, E0, n)
        used = {k // 2 for k in range(n + 1)} | {(k + 1) // 2 for k in range(n + 1)}
        assert max(used) == h and len(m) == n + 1
