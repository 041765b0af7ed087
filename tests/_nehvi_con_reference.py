"""numpy restatement of omb_hvi_paths_con and the inputs its tests share.

    ω(g)  = 1[g ≤ 0] (eta = 0);  1/(1 + e^{g/η}) for g ≤ 0, e^{−g/η}/(1 + e^{−g/η}) for g > 0 (eta > 0)
    w_s   = ((1·ω(g_0s))·ω(g_1s))·…          u_s = t_s·w_s, exactly 0 where w_s == 0
    α     = ((…((0 + u_0) + u_1) + …) + u_{S−1}) / S
    violation (eta = 0): u_s = −((0 + max(g_0s, 0)) + max(g_1s, 0) + …) where w_s == 0

written once over a ``dtype``: ``np.float64`` performs the kernel's operations in the kernel's order (t_s is
``_nehvi_reference.path_values``, or the device's own t_s handed in), ``np.longdouble`` is the reference both are
measured against.  A NaN among the k + c values of path s makes u_s NaN.
"""
import numpy as np

import _nehvi_reference as R

from optimobo_amd import pareto


def omega(g, eta, dtype=np.float64):
    g = np.asarray(g, dtype)
    if eta == 0:
        return np.where(g <= 0, dtype(1.0), dtype(0.0))
    with np.errstate(invalid="ignore", under="ignore"):
        neg = g <= 0
        e = np.exp(np.where(neg, g, -g) / dtype(eta))
        return np.where(neg, dtype(1.0) / (dtype(1.0) + e), e / (dtype(1.0) + e))


def weights(G, eta, dtype=np.float64):
    """w (S, N) of the constraint path values G (c, S, N), multiplied in constraint order from 1."""
    G = np.asarray(G, dtype)
    w = np.ones(G.shape[1:], dtype)
    for g in G:
        w = w * omega(g, eta, dtype)
    return w


def total_violation(G, dtype=np.float64):
    G = np.asarray(G, dtype)
    v = np.zeros(G.shape[1:], dtype)
    with np.errstate(invalid="ignore"):
        for g in G:
            v = v + np.maximum(g, dtype(0.0))
    return v


def u_paths(ts, y, G, eta=0.0, violation=False, dtype=np.float64):
    """u (S, N) from the per-path improvements ts (S, N), the objectives' path values y (k, S, N) (their NaNs count)
    and the constraints' G (c, S, N)."""
    ts = np.asarray(ts, dtype)
    G = np.asarray(G, dtype).reshape((-1,) + ts.shape)
    w = weights(G, eta, dtype)
    with np.errstate(invalid="ignore"):
        u = ts * w
    u = np.where(w == 0, -total_violation(G, dtype) if violation else dtype(0.0), u)
    nan = np.isnan(np.asarray(y, np.float64)).any(axis=0) | np.isnan(np.asarray(G, np.float64)).any(axis=0)
    return np.where(nan, dtype(np.nan), u)


def mean_in_order(u, dtype=np.float64):
    total = np.zeros(u.shape[1], dtype)
    for row in np.asarray(u, dtype):
        total = total + row
    return total / dtype(len(u))


def alpha(y, n_con, coords, box_off, boxes, eta=0.0, violation=False, dtype=np.float64, ts=None):
    """(α (N,), u (S, N)) of y (k + n_con, S, N); ``ts``: the per-path improvements to use in place of the numpy
    ones (the device's own, for the bitwise comparison at k ≥ 2, where the kernel's one fma is not numpy's)."""
    y = np.asarray(y)
    k = y.shape[0] - n_con
    if ts is None:
        with np.errstate(invalid="ignore"):
            ts = R.path_values(y[:k], coords, box_off, boxes, dtype)
    u = u_paths(ts, y[:k], y[k:], eta, violation, dtype)
    return mean_in_order(u, dtype), u


# ------------------------------------------------------------------------------------------------ shared inputs
def constraint_values(c, S, N, rng):
    """G (c, S, N) ~ N(shift, 1) with the shift that leaves half of the (candidate, path) pairs feasible under all c
    constraints; asserted: 20–80 % of the pairs are feasible and (S ≥ 2) some candidate is feasible in some paths
    and not in others."""
    from scipy.stats import norm
    G = rng.normal(size=(c, S, N)) - norm.ppf(0.5 ** (1.0 / c))
    check_mix(G)
    return G


def check_mix(G):
    feas = np.all(np.asarray(G) <= 0, axis=0)                    # (S, N)
    assert 0.2 <= feas.mean() <= 0.8, feas.mean()
    if feas.shape[0] > 1:
        per = feas.sum(axis=0)
        assert np.any((per > 0) & (per < feas.shape[0]))
    return feas


_CACHE = {}


def case(k, c, S, N=1000):
    """(packed lists, y (k + c, S, N)) of one (k, c, S), built once: at k ≥ 2 fronts of unequal sizes, an empty one
    and (k = 2) one list past 1024 boxes; at k = 1 thresholds."""
    key = (k, c, S, N)
    if key not in _CACHE:
        rng = np.random.default_rng(100000 * k + 1000 * c + S)
        if k == 1:
            # thresholds in the upper half of the values' range: most paths leave something to improve on
            packed = pareto.pack_box_lists(pareto.threshold_lists(rng.uniform(0.0, 1.5, size=S)))
            f = rng.normal(size=(1, S, N)) * 1.5
        else:
            big = {2: 1100, 3: 60}.get(k, 20)
            sizes = ([big, 0, 7, 3] + list(rng.integers(1, 12, size=16)))[:S]
            _, packed = R.lists_for(k, sizes, rng)
            f = R.candidates(k, S, N, rng)
        y = np.concatenate([f, constraint_values(c, S, N, rng)]) if c else f
        _CACHE[key] = (packed, y)
    return _CACHE[key]
