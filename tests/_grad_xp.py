"""Extended-precision reference of the posterior gradients' contract, on the bits handed to the device (helper, no
tests).  It sits on tests/_posterior_xp.py: the same installed states (X, ℓ, σ_f², α, L⁻¹), the same 44 candidates,
the same case table.

The contract of omb_posterior_grad on an installed state (include/optimobo_hip.h):

    diff_ij = x_j − X_ij          s_ij = diff_ij/ℓ_j²          r²_i = Σ_j (diff_ij/ℓ_j)²
    g_i = −(5/3)σ_f²(1 + √5 r_i)e^{−√5 r_i}  (Matern-5/2)   or   −k_i  (RBF)
    V = tril(L⁻¹)K*               W = tril(L⁻¹)ᵀV
    ∂μ/∂x_j = Σ_i α_i g_i s_ij    ∂σ²/∂x_j = −2 Σ_i W_i g_i s_ij

``reference_grad`` evaluates it in np.longdouble.  ``restatement_grad`` is plain fp64 numpy, the yardstick for what
an honest fp64 evaluation reaches: K* for W as GPy writes it (expanded-norm r² clipped at 0, as
``_posterior_xp.restatement``), w = tril(Linv).T @ (tril(Linv) @ k), and g, s from differences of the ℓ-scaled
coordinates x/ℓ − X/ℓ, which is how the device forms them.

Rounding scales (``scales_grad``), entry-wise and to first order, in units of u = 2⁻⁵³.  An entry of either gradient
is Σ_i c_i g_i s_ij with c = α or −2W.  Its error sources:

  s   one rounding of each scaled coordinate x_j/ℓ_j, X_ij/ℓ_j before the difference:
          δs_ij ≤ u·E^s_ij,   E^s_ij = (|x_j| + |X_ij|)/ℓ_j²
  g   the same roundings move r²_i = Σ_j (x_j/ℓ_j − X_ij/ℓ_j)² by
          δr²_i ≤ u·ρ_i,      ρ_i = 2 Σ_j |diff_ij/ℓ_j|·(|x_j| + |X_ij|)/ℓ_j,
      and g follows with max |∂g/∂r²| = C_g·σ_f²: C_g = 25/6 for Matern-5/2 (∂g/∂r² = (25/6)σ_f²e^{−√5 r}), 1/2 for
      RBF (∂k/∂r² = −k/2); with g's own rounding
          δg_i ≤ u·E^g_i,     E^g_i = C_g σ_f² ρ_i + |g_i|
  W   K* as GPy writes it is off by u·D (D of ``_posterior_xp._linv_abs_d``: the expanded norm's cancellation through
      max |∂k/∂r²|, plus |K*|), and that error and the two products' own roundings go through |L⁻¹| twice:
          δW_i ≤ u·E^W_i,     E^W = |L⁻¹|ᵀ(|L⁻¹|·D) + |L⁻¹|ᵀ|V|           (|L⁻¹||K*| ≤ |L⁻¹|·D is inside the first)
  Σ   the products and the sum: the plain term magnitudes |c_i||g_i||s_ij|.

With E^t_ij = |g_i|E^s_ij + E^g_i|s_ij| + |g_i||s_ij| the error of a term g_i s_ij itself:

    S_∂μ,j  = Σ_i |α_i|·E^t_ij
    S_∂σ²,j = 2 Σ_i (E^W_i·|g_i||s_ij| + |W_i|·E^t_ij)

A global constant in S is immaterial: the bar is relative to the restatement measured in the same S, and only the
shape of S across entries matters.  That bar is per candidate group: near the data the true |∂σ²/∂x| is anywhere from
1e-4 to 1e5 of u·S, while an honest evaluation stays below one u·S, so "a few roundings of the worst case" would let a
wrong gradient pass.

Far and ray candidates (the last 8): kernel values underflow, the normalised measure says nothing there, and
``check_far`` holds them in absolute terms instead.
"""
import functools

import numpy as np

import _posterior_xp as xp
from _posterior_xp import CASES, GROUPS, KERNELS, LD, U, _linv_abs_d, candidates, late_run_state  # noqa: F401

C_G = {"matern52": 25.0 / 6.0, "rbf": 0.5}           # max |∂g/∂r²| / σ_f²
NEAR = [g for g in GROUPS if g[0] not in ("far", "ray")]
N_NEAR = 36


class Grad:
    """∂μ, ∂σ² (N, d) in np.longdouble with what the bars are stated in: W (n, N), the plain term sums
    am = Σ_i |α_i g_i s_ij|, av = 2 Σ_i |W_i g_i s_ij|, avk = 2 Σ_i (|L⁻¹|ᵀ|L⁻¹||K*|)_i |g_i s_ij| (the term sum of
    ∂σ² before W's own cancellation) and smax = max_i |s_ij|."""
    __slots__ = ("dmu", "dvar", "W", "am", "av", "avk", "smax", "g", "s")


# ----------------------------------------------------------------------------- the contract
def _terms_ld(state, Xc, kernel, K):
    X = np.asarray(state.X, np.float64).astype(LD)
    ls = np.asarray(state.lengthscale, np.float64).astype(LD)
    diff = np.asarray(Xc, np.float64).astype(LD)[None, :, :] - X[:, None, :]          # (n, N, d): x_j − X_ij
    t = diff / ls
    r2 = np.sum(t * t, axis=2)
    if kernel == "matern52":
        r, s5 = np.sqrt(r2), np.sqrt(LD(5))
        g = -(LD(5) / LD(3)) * LD(state.variance) * (1 + s5 * r) * np.exp(-s5 * r)
    else:
        g = -K
    return g, diff / (ls * ls), t


def reference_grad(state, Xc, kernel, ref=None):
    """The contract in np.longdouble; ``ref`` = _posterior_xp.reference(state, Xc, kernel) if already at hand."""
    _, _, K, V = ref if ref is not None else xp.reference(state, Xc, kernel)
    g, s, _ = _terms_ld(state, Xc, kernel, K)
    L = np.tril(np.asarray(state.Linv, np.float64)).astype(LD)
    alpha = np.asarray(state.alpha, np.float64).reshape(-1).astype(LD)
    out = Grad()
    out.W = L.T @ V
    out.g, out.s = g, s
    tm = (alpha[:, None] * g)[:, :, None] * s
    tv = -2 * (out.W * g)[:, :, None] * s
    out.dmu, out.dvar = tm.sum(0), tv.sum(0)
    out.am, out.av = np.abs(tm).sum(0), np.abs(tv).sum(0)
    Wk = np.abs(L).T @ (np.abs(L) @ np.abs(K))
    out.avk = 2 * ((Wk * np.abs(g))[:, :, None] * np.abs(s)).sum(0)
    out.smax = np.abs(s).max(0)
    return out


def restatement_grad(state, Xc, kernel):
    """∂μ, ∂σ² (N, d) in fp64 numpy: GPy's K* for w, direct differences of the scaled coordinates for g and s."""
    X = np.asarray(state.X, np.float64)
    ls = np.asarray(state.lengthscale, np.float64)
    var = float(state.variance)
    a, b = np.asarray(Xc, np.float64) / ls, X / ls
    r2 = -2.0 * (b @ a.T) + (np.sum(np.square(b), 1)[:, None] + np.sum(np.square(a), 1)[None, :])
    r = np.sqrt(np.clip(r2, 0.0, np.inf))
    if kernel == "matern52":
        Kx = var * (1.0 + np.sqrt(5.0) * r + 5.0 / 3.0 * r ** 2) * np.exp(-np.sqrt(5.0) * r)
    else:
        Kx = var * np.exp(-0.5 * r ** 2)
    Lt = np.tril(np.asarray(state.Linv, np.float64))
    w = Lt.T @ (Lt @ Kx)
    df = a[None, :, :] - b[:, None, :]
    rd2 = np.sum(df * df, axis=2)
    if kernel == "matern52":
        rd = np.sqrt(rd2)
        g = -(5.0 / 3.0 * var) * (1.0 + np.sqrt(5.0) * rd) * np.exp(-(np.sqrt(5.0) * rd))
    else:
        g = -(var * np.exp(-0.5 * rd2))
    alpha = np.asarray(state.alpha, np.float64).reshape(-1)
    dmu = ((alpha[:, None] * g)[:, :, None] * df).sum(0) / ls
    dvar = -2.0 * (((w * g)[:, :, None] * df).sum(0) / ls)
    return dmu, dvar


def scales_grad(state, Xc, kernel, ref, rg):
    """S_∂μ, S_∂σ² (N, d) of the header."""
    _, _, K, V = ref
    X = np.abs(np.asarray(state.X, np.float64)).astype(LD)
    x = np.abs(np.asarray(Xc, np.float64)).astype(LD)
    ls = np.asarray(state.lengthscale, np.float64).astype(LD)
    mag = x[None, :, :] + X[:, None, :]                                # |x_j| + |X_ij|
    g, s = np.abs(rg.g), np.abs(rg.s)
    rho = 2 * np.sum(s * mag, axis=2)                                  # |diff/ℓ|·mag/ℓ = |s|·mag
    Eg = LD(C_G[kernel]) * LD(state.variance) * rho + g
    Et = g[:, :, None] * (mag / (ls * ls)) + Eg[:, :, None] * s + g[:, :, None] * s
    alpha = np.abs(np.asarray(state.alpha, np.float64).reshape(-1)).astype(LD)
    s_mu = np.tensordot(alpha, Et, axes=(0, 0))
    _, LD_D = _linv_abs_d(state, Xc, kernel, K)
    La = np.abs(np.tril(np.asarray(state.Linv, np.float64))).astype(LD)
    EW = La.T @ (LD_D + np.abs(V))
    s_var = 2 * (((EW * g)[:, :, None] * s).sum(0) + (np.abs(rg.W)[:, :, None] * Et).sum(0))
    return s_mu, s_var


def normalised(result, ref, S):
    """e = |result − reference| / (u·S) as float64; where S is 0 an exact result is 0 and any other is inf."""
    diff = np.abs(np.asarray(result, np.float64).astype(LD) - ref)
    pos = S > 0
    e = np.where(pos, diff / np.where(pos, LD(U) * S, LD(1)), np.where(diff == 0, LD(0), LD(np.inf)))
    return np.asarray(e, np.float64)


def by_group(e, groups=GROUPS, rows=0):
    """Worst e of every candidate group; ``rows`` shifts the group bounds (a second candidate set stacked below)."""
    return {name: float(np.max(e[rows + lo:rows + hi])) for name, lo, hi in groups}


# ----------------------------------------------------------------------------- far and ray rows
def far_tolerances(state, rg, rows):
    """(tol_∂μ, tol_∂σ²) (len(rows), d) for candidates whose kernel values underflow: an absolute 1e-290 of the
    largest coefficient, plus the relative error an fp64 exp(−√5 r) has at that depth — |x|·(d + 8)·u from r², |x| ≤
    895 before k is 0, twice for the polynomial and the sum (test_gpu_posterior_xp.check_moments' term for μ) — of
    the term sums Σ_i |α_i g_i s_ij| and 2 Σ_i (|L⁻¹|ᵀ|L⁻¹||K*|)_i |g_i s_ij|."""
    d = state.X.shape[1]
    rel = LD(2.0 * 895.0 * (d + 8) * U)
    sum_alpha = LD(np.abs(np.asarray(state.alpha, np.float64)).sum())
    tol_mu = LD(1e-290) * sum_alpha * rg.smax[rows] + rel * rg.am[rows]
    tol_var = LD(1e-290) * LD(state.variance) * rg.smax[rows] + rel * rg.avk[rows]
    return tol_mu, tol_var


def check_far(label, state, kernel, dmu, dvar, rg, rows):
    """Device rows ``rows`` (far or ray candidates) of one objective against the reference."""
    dm, dv = np.asarray(dmu, np.float64)[rows], np.asarray(dvar, np.float64)[rows]
    assert np.all(np.isfinite(dm)) and np.all(np.isfinite(dv)), label
    if kernel == "rbf":                                   # every term is exactly 0
        assert np.all(dm == 0.0) and np.all(dv == 0.0), (label, dm, dv)
        return
    tol_mu, tol_var = far_tolerances(state, rg, rows)
    assert np.all(np.abs(dm.astype(LD) - rg.dmu[rows]) <= tol_mu), (label, dm, rg.dmu[rows])
    assert np.all(np.abs(dv.astype(LD) - rg.dvar[rows]) <= tol_var), (label, dv, rg.dvar[rows])


# ----------------------------------------------------------------------------- the table
@functools.lru_cache(maxsize=None)
def case(n, d, kernel, obj=0):
    """(state, Xc, posterior reference, Grad, (S_∂μ, S_∂σ²)) of one case, computed once and shared read-only."""
    st, Xc, ref, _ = xp.case(n, d, kernel, obj)
    rg = reference_grad(st, Xc, kernel, ref)
    return st, Xc, ref, rg, scales_grad(st, Xc, kernel, ref, rg)


@functools.lru_cache(maxsize=None)
def restatement_error(n, d, kernel, obj=0):
    """group → (worst e_∂μ, worst e_∂σ²) of the fp64 restatement on one case."""
    st, Xc, _, rg, (s_mu, s_var) = case(n, d, kernel, obj)
    dm, dv = restatement_grad(st, Xc, kernel)
    em, ev = normalised(dm, rg.dmu, s_mu).max(1), normalised(dv, rg.dvar, s_var).max(1)
    gm, gv = by_group(em), by_group(ev)
    return {name: (gm[name], gv[name]) for name, _, _ in GROUPS}


@functools.lru_cache(maxsize=None)
def bar():
    """group → (T_∂μ, T_∂σ²): 4 × the restatement's worst normalised error of that group over the whole table
    (objective 0); the near groups only."""
    errs = [restatement_error(n, d, k) for n, d in CASES for k in KERNELS]
    return {name: (4.0 * max(e[name][0] for e in errs), 4.0 * max(e[name][1] for e in errs)) for name, _, _ in NEAR}


@functools.lru_cache(maxsize=None)
def case_bar(n, d):
    """group → (T_∂μ, T_∂σ²) of one shape: the same rule taken over the shape's own four cases (both kernels, both
    objectives).  S_∂σ² carries the worst case of the expanded norm's cancellation through |L⁻¹| twice, which an honest
    evaluation stays three to seven orders below at n_var ≤ 30, so the table's ∂σ² bar — set by the wide shapes — is
    that far above what the restatement reaches on the others; the shape's own bar is not."""
    errs = [restatement_error(n, d, k, o) for k in KERNELS for o in (0, 1)]
    return {name: (4.0 * max(e[name][0] for e in errs), 4.0 * max(e[name][1] for e in errs)) for name, _, _ in NEAR}


ceiling = xp.ceiling
