"""Restatement of the posterior sample paths, on the bits handed to the device (helper, no tests).

An installed state is (X, ℓ, σ_f², α, L⁻¹) in fp64 — what ``set_gp`` uploads — and a batch of paths is (ω̃, b, w, z,
σ_n²) as handed to ``paths_set``.  The contract of omb_paths_set / omb_paths_eval on them:

    φ_i(x) = sqrt(2σ_f²/m)·cos(ω̃_i·(x/ℓ) + b_i)          U = Φ(X) w + sqrt(σ_n² + 1e-8)·z
    V = α − L⁻ᵀ(L⁻¹ U)   (tril(L⁻¹))                     f_s(x) = φ(x)ᵀ w_s + k(x, X) V_s

``reference`` evaluates it in np.longdouble, ``restatement`` in plain fp64 numpy (the yardstick for what an honest
fp64 evaluation achieves); both also return the term sum Σ_i |φ_i w_is| + Σ_j |k_j V_js| that errors are measured
in (DESIGN §20's convention).  ``path_moments`` gives the closed-form mean and variance of f_s(x) over w and z next
to the exact posterior variance.
"""
import functools

import numpy as np

from _posterior_xp import LD, _kernel_ld, _r2_ld


def make_state(n, d, kernel, seed, noise=0.0, obj=0):
    """A well-conditioned GPState on n uniform points of [0, 1]^d."""
    from optimobo_amd.gp import GPState
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 1.0, (n, d))
    ls = rng.uniform(0.3, 1.2, d) * np.sqrt(d)
    y = np.sin(3.0 * X).sum(1) if obj % 2 == 0 else np.cos(2.0 * X).prod(1) + 0.3 * X[:, 0]
    return GPState(X, y, ls, float(np.var(y) + 0.1) if n > 1 else 1.0, kernel=kernel, noise=noise)


def _bits(state):
    return (np.asarray(state.X, np.float64), np.asarray(state.lengthscale, np.float64).reshape(-1),
            float(state.variance), np.asarray(state.alpha, np.float64).reshape(-1),
            np.tril(np.asarray(state.Linv, np.float64)))


def _features_ld(Xq, ls, variance, omega, phase):
    """Φ (N, m) in np.longdouble, the argument summed one input dimension at a time."""
    arg = np.zeros((Xq.shape[0], omega.shape[0]), LD) + phase.astype(LD)[None, :]
    for j in range(Xq.shape[1]):
        arg += (Xq[:, j].astype(LD) / LD(ls[j]))[:, None] * omega[:, j].astype(LD)[None, :]
    return np.sqrt(LD(2) * LD(variance) / LD(omega.shape[0])) * np.cos(arg)


def reference(state, kernel, omega, phase, w, z, noise, Xc):
    """f (S, N), term sum T (S, N), V (n, S), all np.longdouble."""
    X, ls, var, alpha, Linv = _bits(state)
    omega, phase, w = (np.asarray(a, np.float64) for a in (omega, phase, w))
    Xc = np.asarray(Xc, np.float64)
    wl = w.astype(LD)
    U = _features_ld(X, ls, var, omega, phase) @ wl
    if z is not None:
        U = U + np.sqrt(LD(noise) + LD(1e-8)) * np.asarray(z, np.float64).astype(LD)
    Ll = Linv.astype(LD)
    V = alpha.astype(LD)[:, None] - Ll.T @ (Ll @ U)
    Phi = _features_ld(Xc, ls, var, omega, phase)
    K = _kernel_ld(_r2_ld(X, Xc, ls), var, kernel)          # (n, N)
    f = (Phi @ wl).T + V.T @ K
    T = (np.abs(Phi) @ np.abs(wl)).T + np.abs(V).T @ np.abs(K)
    return f, T, V


def _kernel64(X, Xc, ls, variance, kernel):
    a, b = Xc / ls, X / ls
    r2 = -2.0 * (b @ a.T) + (np.sum(np.square(b), 1)[:, None] + np.sum(np.square(a), 1)[None, :])
    r = np.sqrt(np.clip(r2, 0.0, np.inf))
    if kernel == "matern52":
        return variance * (1.0 + np.sqrt(5.0) * r + 5.0 / 3.0 * r ** 2) * np.exp(-np.sqrt(5.0) * r)
    return variance * np.exp(-0.5 * r ** 2)


def _features64(Xq, ls, variance, omega, phase):
    return np.sqrt(2.0 * variance / omega.shape[0]) * np.cos((Xq / ls) @ omega.T + phase[None, :])


def restatement(state, kernel, omega, phase, w, z, noise, Xc):
    """f (S, N) and V (n, S) by the same formula in plain fp64 numpy."""
    X, ls, var, alpha, Linv = _bits(state)
    omega, phase, w = (np.asarray(a, np.float64) for a in (omega, phase, w))
    Xc = np.asarray(Xc, np.float64)
    U = _features64(X, ls, var, omega, phase) @ w
    if z is not None:
        U = U + np.sqrt(noise + 1e-8) * np.asarray(z, np.float64)
    V = alpha[:, None] - Linv.T @ (Linv @ U)
    f = (_features64(Xc, ls, var, omega, phase) @ w).T + V.T @ _kernel64(X, Xc, ls, var, kernel)
    return f, V


def normalised(result, ref, T):
    """|result − reference| / term sum, as float64 (an entry whose term sum is 0 is exactly 0 in every evaluation)."""
    e = np.abs(np.asarray(result, np.float64).astype(LD) - ref)
    return np.asarray(np.where(T > 0, e / np.where(T > 0, T, 1), e), np.float64)


@functools.lru_cache(maxsize=None)
def statistics_case():
    """The statistics tests' fixed draws: a Matern-5/2 state (n = 130, d = 6), 64 candidates and 16 batches of
    S = 16 paths on m = 1024 features each → (state, Xc, [(omega, phase, w, z)] · 16)."""
    from optimobo_amd.paths import draw_path_inputs
    st = make_state(130, 6, "matern52", seed=2024)
    Xc = np.random.default_rng(77).uniform(0.0, 1.0, (64, 6))
    Xc.setflags(write=False)
    draws = [draw_path_inputs("matern52", 130, 6, 16, 1024, np.random.default_rng(500 + g), np.zeros(6), np.ones(6),
                              st.lengthscale) for g in range(16)]
    return st, Xc, draws


def path_moments(state, kernel, omega, phase, noise, Xc):
    """Closed form over w ~ N(0, I), z ~ N(0, I), in fp64: the mean μ(x) = k(x, X) α of a path, its variance
    ‖φ(x) − Φ(X)ᵀ K_y⁻¹ k‖² + (σ_n² + 1e-8)·‖K_y⁻¹ k‖², and the exact posterior variance σ_f² − kᵀ K_y⁻¹ k."""
    X, ls, var, alpha, Linv = _bits(state)
    omega, phase = np.asarray(omega, np.float64), np.asarray(phase, np.float64)
    Xc = np.asarray(Xc, np.float64)
    K = _kernel64(X, Xc, ls, var, kernel)                   # (n, N)
    A = Linv.T @ (Linv @ K)                                 # K_y⁻¹ k
    resid = _features64(Xc, ls, var, omega, phase).T - _features64(X, ls, var, omega, phase).T @ A   # (m, N)
    pathvar = np.sum(resid * resid, 0) + (noise + 1e-8) * np.sum(A * A, 0)
    return alpha @ K, pathvar, var - np.sum(K * A, 0)
