"""The identity behind the deferred last Jacobi sweep, on a dozen sites in dense numpy: with
mu_0 = alpha E, mu_{k+1} = alpha (E - T mu_k) and T symmetric,
    -1/2 sum mu_n.E  =  -1/2 sum mu_0.E + 1/2 (T mu_0).mu_{n-1},
so the energy of an n-sweep solve needs the dipoles of sweep n - 1 and the first sweep's sums only."""
import numpy as np
import pytest


def _case(seed, nsite=12):
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0.0, 9.0, size=(nsite, 3))
    alpha = rng.uniform(0.3, 1.5, size=nsite)
    alpha[3] = 0.0  # a site without polarizability keeps mu = 0 and drops out of both sides
    T = np.zeros((3 * nsite, 3 * nsite))
    for i in range(nsite):
        for j in range(i + 1, nsite):
            d = pos[i] - pos[j]
            r = np.linalg.norm(d)
            blk = np.eye(3) / r**3 - 3.0 * np.outer(d, d) / r**5  # c3 I - 3 c5 d d^T, stored once per unordered pair
            T[3 * i:3 * i + 3, 3 * j:3 * j + 3] = blk
            T[3 * j:3 * j + 3, 3 * i:3 * i + 3] = blk
    E = rng.normal(size=3 * nsite)
    return T, np.repeat(alpha, 3), E


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("n", [2, 3, 4, 5, 6])
def test_energy_from_sweep_n_minus_1(seed, n):
    T, a, E = _case(seed)
    assert np.array_equal(T, T.T)
    mu0 = a * E
    mu = [mu0]
    for _ in range(n):
        mu.append(a * (E - T @ mu[-1]))
    direct = -0.5 * np.dot(mu[n], E)
    deferred = -0.5 * np.dot(mu0, E) + 0.5 * np.dot(T @ mu0, mu[n - 1])
    assert abs(deferred - direct) <= 1e-14 * abs(direct), (deferred, direct)
    assert abs(direct - (-0.5 * np.dot(mu[n - 1], E))) > 1e-6 * abs(direct)  # (the last sweep does change the energy)
