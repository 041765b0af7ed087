"""Restatement of the sample paths' gradient and of the sampled-front improvement's gradient, on the bits handed to
the device (helper, no tests; builds on tests/_paths_reference.py and tests/_nehvi_reference.py).

    ∂f_s/∂x_j = −(1/ℓ_j) Σ_i w_is·sqrt(2σ_f²/m)·ω̃_ij·sin(ω̃_i·(x/ℓ) + b_i)  +  Σ_r V_rs·g_r·(x_j − X_rj)/ℓ_j²
    g_r = −(5/3)σ_f²(1 + √5 r)e^{−√5 r} (Matern-5/2)  or  −k_r (RBF)

``path_gradient`` evaluates it in np.longdouble or in plain fp64 numpy (``dtype``), the difference x_j − X_rj formed
first in both, and returns next to it the term sum per dimension, Σ_i |feature term| + Σ_r |update term|, that errors
are measured in.

    ∂t_s/∂y_j = −Σ_b 1[lo_bj < y_j < hi_bj] Π_{l≠j} (hi_bl − max(y_l, lo_bl))⁺      (strict: 0 on a grid coordinate)
    ∂t_s/∂x   = Σ_j ∂t_s/∂y_j · dy[j, s],  j ascending;      ∂α/∂x = ((…(0 + ∂t_0) + …) + ∂t_{S−1}) / S

``hvi_gradient`` evaluates that over packed lists in either precision, in the kernel's order (slices of 1024 boxes
from the list's own start summed from 0 in list order, added in slice order), with the term sum
Σ_s Σ_j Σ_b |box term|·|dy| / S (per path: without the mean).
"""
import numpy as np

import _paths_reference as pr
from _posterior_xp import LD

SLICE = 1024


def _V(state, omega, phase, w, z, noise, dtype):
    X, ls, var, alpha, Linv = pr._bits(state)
    if dtype is LD:
        U = pr._features_ld(X, ls, var, omega, phase) @ w.astype(LD)
        if z is not None:
            U = U + np.sqrt(LD(noise) + LD(1e-8)) * np.asarray(z, np.float64).astype(LD)
        Ll = Linv.astype(LD)
        return alpha.astype(LD)[:, None] - Ll.T @ (Ll @ U)
    U = pr._features64(X, ls, var, omega, phase) @ w
    if z is not None:
        U = U + np.sqrt(noise + 1e-8) * np.asarray(z, np.float64)
    return alpha[:, None] - Linv.T @ (Linv @ U)


def path_gradient(state, kernel, omega, phase, w, z, noise, Xc, dtype=LD):
    """(grad (S, d, N), term sum T (S, d, N)) in ``dtype`` (np.longdouble or np.float64)."""
    X, ls, var, _, _ = pr._bits(state)
    omega, phase, w = (np.asarray(a, np.float64) for a in (omega, phase, w))
    Xc = np.asarray(Xc, np.float64)
    t = dtype
    V = _V(state, omega, phase, w, z, noise, dtype).astype(t)            # (n, S)
    m, d = omega.shape
    lsd, om, wd = ls.astype(t), omega.astype(t), w.astype(t)
    xs = Xc.astype(t) / lsd[None, :]
    arg = np.zeros((Xc.shape[0], m), t) + phase.astype(t)[None, :]
    for j in range(d):
        arg += xs[:, j][:, None] * om[:, j][None, :]
    sn = np.sqrt(t(2) * t(var) / t(m)) * np.sin(arg)                     # (N, m)
    diff = [(Xc[:, j].astype(t)[None, :] - X[:, j].astype(t)[:, None]) / lsd[j] for j in range(d)]   # (n, N) each
    r2 = np.zeros((X.shape[0], Xc.shape[0]), t)
    for df in diff:
        r2 += df * df
    if kernel == "matern52":
        r, s5 = np.sqrt(r2), np.sqrt(t(5))
        g = -(t(5) / t(3)) * t(var) * (1 + s5 * r) * np.exp(-s5 * r)
    else:
        g = -t(var) * np.exp(-r2 / 2)
    S, N = w.shape[1], Xc.shape[0]
    grad, T = np.zeros((S, d, N), t), np.zeros((S, d, N), t)
    aw, aV = np.abs(wd), np.abs(V)
    for j in range(d):
        A = sn * om[:, j][None, :]                                       # (N, m)
        B = g * diff[j] / lsd[j]                                         # (n, N)
        grad[:, j, :] = -(A @ wd).T / lsd[j] + V.T @ B
        T[:, j, :] = (np.abs(A) @ aw).T / lsd[j] + aV.T @ np.abs(B)
    return grad, T


def normalised(result, ref, T):
    return pr.normalised(result, ref, T)


def _dt_path(y, coords, boxes, dtype):
    """(t (N,), dt (k, N), |dt| sum (k, N)) of the points y (k, N) over one grid and list."""
    y = np.asarray(y, dtype)
    g = np.asarray(coords, dtype)
    boxes = np.asarray(boxes, np.int64)
    k, N = y.shape
    zero, one = dtype(0.0), dtype(1.0)
    total, dtot, atot = np.zeros(N, dtype), np.zeros((k, N), dtype), np.zeros((k, N), dtype)
    with np.errstate(invalid="ignore"):
        for b0 in range(0, len(boxes), SLICE):
            bl = boxes[b0:b0 + SLICE]
            ts, ins = [], []
            for j in range(k):
                lo = g[j, bl[:, 2 * j]][:, None]
                hi = g[j, bl[:, 2 * j + 1]][:, None]
                ts.append(np.maximum(hi - np.maximum(y[j][None, :], lo), zero))
                ins.append((lo < y[j][None, :]) & (y[j][None, :] < hi))
            prod = ts[0]
            for j in range(1, k):
                prod = prod * ts[j]
            total = total + np.cumsum(prod, axis=0, dtype=dtype)[-1]
            # Π_{l≠j} t_l = (t_0 ⋯ t_{j−1})·(t_{j+1} ⋯ t_{k−1}), as the kernel forms it
            suf = [None] * k
            suf[k - 1] = np.full_like(ts[0], one)
            for j in range(k - 2, -1, -1):
                suf[j] = ts[j + 1] * suf[j + 1]
            pre = np.full_like(ts[0], one)
            for j in range(k):
                term = np.where(ins[j], pre * suf[j], zero)
                s = np.cumsum(term, axis=0, dtype=dtype)[-1]
                dtot[j] = dtot[j] - s
                atot[j] = atot[j] + s
                pre = pre * ts[j]
    return total, dtot, atot


def hvi_gradient(y, dy, coords, box_off, boxes, dtype=LD):
    """y (k, S, N), dy (k, S, d, N) → dict(v (N,), g (N, d), t (S, N), tg (S, N, d), Tg (N, d), Ttg (S, N, d)) in
    ``dtype``; Tg / Ttg are the term sums of g / tg.  A NaN t_s makes its tg NaN, a NaN v every entry of g."""
    y = np.asarray(y, np.float64)
    dy = np.asarray(dy, np.float64)
    k, S, N = y.shape
    d = dy.shape[2]
    t = np.zeros((S, N), dtype)
    tg, Ttg = np.zeros((S, N, d), dtype), np.zeros((S, N, d), dtype)
    with np.errstate(invalid="ignore"):
        for s in range(S):
            ts, dts, ats = _dt_path(y[:, s, :], coords[s], boxes[box_off[s]:box_off[s + 1]], dtype)
            nan = np.isnan(y[:, s, :]).any(0)
            t[s] = np.where(nan, dtype(np.nan), ts)
            acc, aacc = np.zeros((N, d), dtype), np.zeros((N, d), dtype)
            for j in range(k):
                acc = acc + dts[j][:, None] * dy[j, s].astype(dtype).T
                aacc = aacc + ats[j][:, None] * np.abs(dy[j, s].astype(dtype).T)
            tg[s] = np.where(nan[:, None], dtype(np.nan), acc)
            Ttg[s] = aacc
        v, g, Tg = np.zeros(N, dtype), np.zeros((N, d), dtype), np.zeros((N, d), dtype)
        for s in range(S):
            v = v + t[s]
            g = g + tg[s]
            Tg = Tg + Ttg[s]
        v, g, Tg = v / dtype(S), g / dtype(S), Tg / dtype(S)
        g = np.where(np.isnan(v)[:, None], dtype(np.nan), g)
    return dict(v=v, g=g, t=t, tg=tg, Tg=Tg, Ttg=Ttg)
