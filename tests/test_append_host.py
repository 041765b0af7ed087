"""The bordered update behind omb_gp_append, restated in numpy and checked against a full refactorisation.

Conditioning a fitted state (X, ℓ, σ_f², α, L⁻¹) of n points on one more observation (x, y) at noise σ_n²:
    k = K(X, x),  μ = kᵀα,  v = L⁻¹k,  δ² = σ_f² + σ_n² + 1e-8 − vᵀv,  w = L⁻ᵀv,  ζ = (y − μ)/δ
    L⁻¹' = [[L⁻¹, 0], [−wᵀ/δ, 1/δ]],   α' = [α − w·ζ/δ ; ζ/δ],   X' = [X ; x].
``bordered_append`` below is that update; the GPU tests (tests/test_gpu_append.py) take their cases, the oracle
states and the sequential predictive moments from this module.

The guard here proves that the cases are ones where the update itself is accurate: after q appended points the
restated posterior stays within ONE TENTH of the project's posterior tolerance (1e-6 relative, floors 1e-7·σ_f for μ
and 1e-9·σ_f² for σ²) of oracle.gp.ExactGP refactorised on all n + q points.  Measured: at most 1.2e-5 of
the tolerance (printed per case).
"""
import functools

import numpy as np
import pytest
from scipy import linalg

from oracle import gp as ogp

VARIANCE = 1.7
N_EVAL = 256
# (n, d, q, noise, kernel)
HOST_CASES = [(15, 2, 3, 0.0, "matern52"), (63, 6, 3, 0.0, "matern52"), (127, 6, 2, 1e-4, "rbf"),
              (200, 30, 8, 0.0, "matern52"), (1023, 6, 2, 0.0, "matern52")]
# the smallest state, and one whose mat-vecs span many workgroups and row chunks (the GPU tests run these too)
EDGE_CASES = [(1, 1, 2, 0.0, "matern52"), (2050, 5, 2, 1e-4, "matern52")]


@functools.lru_cache(maxsize=None)
def make_case(n, d, q, noise, kernel):
    """X (n + q, d) uniform in the unit box, y, ℓ ∈ [0.3, 1]·√d, and N_EVAL evaluation points."""
    rng = np.random.default_rng(100000 * q + 100 * n + d)
    X = rng.uniform(0.0, 1.0, (n + q, d))
    ls = rng.uniform(0.3, 1.0, d) * np.sqrt(d)
    w = rng.normal(size=d) / np.sqrt(d)
    y = np.sin(3.0 * X @ w) + 0.5 * np.cos(2.0 * X.sum(1) / np.sqrt(d))
    Xc = rng.uniform(0.0, 1.0, (N_EVAL, d))
    for a in (X, y, ls, Xc):
        a.setflags(write=False)
    return X, y, ls, Xc


@functools.lru_cache(maxsize=None)
def oracle_gp(n, d, q, noise, kernel, m):
    """ExactGP refactorised on the first m points of the case."""
    X, y, ls, _ = make_case(n, d, q, noise, kernel)
    return ogp.ExactGP(X[:m], y[:m], ls, VARIANCE, kernel=kernel, noise=noise)


@functools.lru_cache(maxsize=None)
def oracle_refit(n, d, q, noise, kernel):
    """(μ, latent σ²) of the full refit on n + q points at the case's evaluation points."""
    g = oracle_gp(n, d, q, noise, kernel, n + q)
    mu, var = g.predict(make_case(n, d, q, noise, kernel)[3])
    return mu[:, 0], var[:, 0] - noise


@functools.lru_cache(maxsize=None)
def oracle_sequential(n, d, q, noise, kernel):
    """Point j's predictive mean and δ² = latent σ² + σ_n² + 1e-8 under the refit on the n + j points before it."""
    X = make_case(n, d, q, noise, kernel)[0]
    mus, d2 = [], []
    for j in range(q):
        mu, var = oracle_gp(n, d, q, noise, kernel, n + j).predict(X[n + j][None, :])
        mus.append(mu[0, 0])
        d2.append(var[0, 0] + 1e-8)          # predict's variance carries σ_n² already
    return np.array(mus), np.array(d2)


def bordered_append(X, ls, variance, kernel, alpha, Linv, x, y, noise):
    """One point: the state of n + 1 points, the point's predictive mean and its δ².  y None: the believer."""
    k = ogp.KERNELS[kernel](X, x[None, :], ls, variance)[:, 0]
    mu = k @ alpha
    v = Linv @ k
    d2 = variance + noise + 1e-8 - v @ v
    if not (d2 > 0.0 and np.isfinite(d2)):
        raise linalg.LinAlgError("delta^2 <= 0")
    delta = np.sqrt(d2)
    w = Linv.T @ v
    zeta = ((mu if y is None else y) - mu) / delta
    n = len(alpha)
    Lnew = np.zeros((n + 1, n + 1))
    Lnew[:n, :n] = Linv
    Lnew[n, :n] = -w / delta
    Lnew[n, n] = 1.0 / delta
    return np.vstack((X, x)), np.append(alpha - w * zeta / delta, zeta / delta), Lnew, mu, d2


def restated_posterior(X, ls, variance, kernel, alpha, Linv, Xc):
    Kx = ogp.KERNELS[kernel](X, Xc, ls, variance)
    return Kx.T @ alpha, variance - np.square(Linv @ Kx).sum(0)


def tolerance_ratio(mu, var, mu_ref, var_ref, variance):
    """Largest |error| / (project tolerance) over μ and σ²: ≤ 1 passes assert_allclose at the project's bar."""
    rm = np.abs(mu - mu_ref) / (1e-7 * np.sqrt(variance) + 1e-6 * np.abs(mu_ref))
    rv = np.abs(var - var_ref) / (1e-9 * variance + 1e-6 * np.abs(var_ref))
    return float(max(rm.max(), rv.max()))


@pytest.mark.parametrize("n,d,q,noise,kernel", HOST_CASES + EDGE_CASES)
def test_bordered_update_matches_refactorisation(n, d, q, noise, kernel):
    X, y, ls, Xc = make_case(n, d, q, noise, kernel)
    g = oracle_gp(n, d, q, noise, kernel, n)
    Xa, alpha = X[:n], g.alpha[:, 0]
    Linv = linalg.solve_triangular(g.L, np.eye(n), lower=True)
    seq_mu, seq_d2 = oracle_sequential(n, d, q, noise, kernel)
    for j in range(q):
        Xa, alpha, Linv, mu, d2 = bordered_append(Xa, ls, VARIANCE, kernel, alpha, Linv, X[n + j], y[n + j], noise)
        assert abs(mu - seq_mu[j]) <= 0.1 * (1e-7 * np.sqrt(VARIANCE) + 1e-6 * abs(seq_mu[j]))
        assert abs(d2 - seq_d2[j]) <= 0.1 * (1e-9 * VARIANCE + 1e-6 * abs(seq_d2[j]))
    assert np.array_equal(Xa, X) and np.all(np.triu(Linv, 1) == 0.0)
    mu, var = restated_posterior(Xa, ls, VARIANCE, kernel, alpha, Linv, Xc)
    mu_ref, var_ref = oracle_refit(n, d, q, noise, kernel)
    ratio = tolerance_ratio(mu, var, mu_ref, var_ref, VARIANCE)
    print(f"n={n} d={d} q={q} noise={noise:g} {kernel}: worst error = {ratio:.2e} of the project tolerance")
    assert ratio <= 0.1


def test_believer_keeps_the_mean():
    """y = μ: ζ = 0, the old α entries keep their bits and the new one is exactly 0."""
    n, d, q, noise, kernel = HOST_CASES[1]
    X, y, ls, Xc = make_case(n, d, q, noise, kernel)
    g = oracle_gp(n, d, q, noise, kernel, n)
    Linv = linalg.solve_triangular(g.L, np.eye(n), lower=True)
    mu0, var0 = restated_posterior(X[:n], ls, VARIANCE, kernel, g.alpha[:, 0], Linv, Xc)
    Xa, alpha, Lnew, _, _ = bordered_append(X[:n], ls, VARIANCE, kernel, g.alpha[:, 0], Linv, X[n], None, noise)
    assert np.array_equal(alpha[:n], g.alpha[:, 0]) and alpha[n] == 0.0
    mu1, var1 = restated_posterior(Xa, ls, VARIANCE, kernel, alpha, Lnew, Xc)
    assert np.abs(mu1 - mu0).max() <= 1e-12 * np.sqrt(VARIANCE) and np.all(var1 <= var0 + 1e-12 * VARIANCE)


def test_signature_table_types_omb_gp_append():
    import ctypes

    from optimobo_amd import _lib
    res, args = _lib.SIGNATURES["omb_gp_append"]
    p, i, dbl = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    assert res is i and args == [p, i, i, p, p, dbl, p, p]
