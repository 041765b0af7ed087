"""Host side of the posterior sample paths (omb_paths_set / omb_paths_eval): the random draws.  numpy only.

A path is f_s(x) = φ(x)ᵀ w_s + k(x, X) v_s with φ_i(x) = sqrt(2σ_f²/m)·cos(ω̃_i·(x/ℓ) + b_i), m random Fourier
features of the prior (Rahimi & Recht 2007), and v_s = α − K_y⁻¹(Φ(X) w_s + ε_s) the pathwise update (Wilson et al.
2020).  This module draws ω̃, b, w and the standard normals z behind ε; the device does the rest.
"""
import numpy as np

# the device cosine's argument range (include/optimobo_hip.h)
MAX_ARGUMENT = float(1 << 20)


def spectral_frequencies(kernel, m, d, rng):
    """(m, d) frequencies ω̃ of the unit-lengthscale kernel, acting on x/ℓ.

    RBF: ω̃ = g, g ~ N(0, I).  Matern-5/2: ω̃ = g·sqrt(5/u), u ~ χ²₅ per row — the spectral density of Matern-ν
    is a multivariate Student-t with 2ν degrees of freedom."""
    g = rng.standard_normal((int(m), int(d)))
    if kernel == "rbf":
        return g
    if kernel == "matern52":
        u = rng.chisquare(5.0, size=int(m))
        return g * np.sqrt(5.0 / u)[:, None]
    raise ValueError(f"unknown kernel {kernel!r} (matern52 or rbf)")


def worst_argument(omega, lower, upper, lengthscale):
    """Per frequency row, the largest |ω̃·(x/ℓ) + b| over the box: Σ_j |ω̃_ij|·max(|lo_j|, |hi_j|)/ℓ_j + 2π."""
    reach = np.maximum(np.abs(np.asarray(lower, np.float64)), np.abs(np.asarray(upper, np.float64)))
    reach = reach.reshape(-1) / np.asarray(lengthscale, np.float64).reshape(-1)
    return np.abs(omega) @ reach + 2.0 * np.pi


def feature_lengthscale(lengthscale, lower, upper):
    """The lengthscale the features are drawn for: ℓ_j, but no smaller than 100·d·2^-20 of the box's reach
    max(|lo_j|, |hi_j|).  Below that floor (a degenerate fit: ℓ = 1e-16 happens in near-singular runs) almost no
    frequency keeps ω̃_j·x_j/ℓ_j inside the device cosine's 2^20 range, and nothing a candidate set of 2^16 … 2^20
    points could resolve is lost: the prior part of a path is then as smooth as the floor allows — white noise at the
    candidates' spacing — while the update term keeps the fitted kernel."""
    ls = np.asarray(lengthscale, np.float64).reshape(-1)
    reach = np.maximum(np.abs(np.asarray(lower, np.float64)), np.abs(np.asarray(upper, np.float64))).reshape(-1)
    return np.maximum(ls, 100.0 * ls.size * reach / MAX_ARGUMENT)


def draw_path_inputs(kernel, n, d, S, m, rng, lower=None, upper=None, lengthscale=None):
    """The draws of S paths over n training points in d dimensions with m features → omega (m, d), phase (m,)
    ~ U[0, 2π), w (m, S), z (n, S), drawn in that order so that a seed pins a batch.

    With bounds (and the lengthscale, default 1) any frequency row whose worst-case argument over the box exceeds
    2^20 — the device cosine's stated range — is drawn again, after the four arrays, until none is left; the
    probability is below 1e-9 per row for a sane lengthscale."""
    omega = spectral_frequencies(kernel, m, d, rng)
    phase = rng.uniform(0.0, 2.0 * np.pi, size=int(m))
    w = rng.standard_normal((int(m), int(S)))
    z = rng.standard_normal((int(n), int(S)))
    if lower is not None and upper is not None:
        ls = np.ones(d) if lengthscale is None else np.broadcast_to(np.asarray(lengthscale, np.float64), (d,))
        for _ in range(1000):
            bad = np.flatnonzero(~(worst_argument(omega, lower, upper, ls) <= MAX_ARGUMENT))
            if bad.size == 0:
                break
            omega[bad] = spectral_frequencies(kernel, bad.size, d, rng)
        else:
            raise ValueError("draw_path_inputs: the lengthscale is so small against the box that no frequency keeps "
                             "its argument within 2^20")
    return omega, phase, w, z
