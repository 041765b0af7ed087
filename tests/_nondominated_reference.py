"""Host references of the non-dominated filter (omb_nondominated), minimisation, rows are points.

``definition``  the contract itself: ``pareto.nondominated_mask`` (the O(N²) le / lt broadcast) with the NaN rows
                cleared — a NaN row dominates nobody there already, since every comparison with it is false.
``sweep_2d``    an exact O(N log N) sort-and-sweep for two objectives that keeps duplicates, for sizes the O(N²) form
                cannot reach.  NaN-free input.
"""
import numpy as np

from optimobo_amd import pareto


def definition(Y):
    Y = np.asarray(Y, np.float64)
    Y = Y[:, None] if Y.ndim == 1 else Y
    return pareto.nondominated_mask(Y) & ~np.isnan(Y).any(axis=1)


def sweep_2d(Y):
    """mask (N,) of the rows of Y (N, 2) that no row dominates.  Sorted by (y1, y2), a row is dominated exactly when
    a row with a strictly smaller y1 has y2' ≤ y2, or a row with the same y1 has y2' < y2: the first is a running
    minimum over the groups of equal y1 before it, the second the group's own minimum."""
    Y = np.asarray(Y, np.float64).reshape(-1, 2)
    n = len(Y)
    mask = np.zeros(n, bool)
    if n == 0:
        return mask
    a, b = Y[:, 0] + 0.0, Y[:, 1] + 0.0                 # −0.0 + 0.0 = +0.0: one key for both zeros
    order = np.lexsort((b, a))
    a, b = a[order], b[order]
    start = np.flatnonzero(np.concatenate(([True], a[1:] != a[:-1])))      # first row of each group of equal y1
    group_min = b[start]                                                   # sorted by y2 within the group
    before = np.concatenate(([np.inf], np.minimum.accumulate(group_min)[:-1]))   # min y2 over smaller y1
    gid = np.cumsum(np.concatenate(([0], (a[1:] != a[:-1]).astype(np.int64))))
    keep = (b == group_min[gid]) & ((gid == 0) | (b < before[gid]))      # the first group has nothing before it
    mask[order] = keep
    return mask


# ---- the inputs of tests/test_nondominated_host.py and tests/test_gpu_nondominated.py, rows are points
def iid(rng, N, k):
    return rng.normal(size=(N, k))


def ties(rng, N, k):
    """Integers in [0, 4): heavy ties and duplicates."""
    return rng.integers(0, 4, size=(N, k)).astype(np.float64)


def antichain(N, k):
    """(i, N − 1 − i, 0, …): every point kept."""
    Y = np.zeros((N, k))
    Y[:, 0] = np.arange(N)
    if k > 1:
        Y[:, 1] = N - 1 - np.arange(N)
    return Y


def chain(N, k, duplicate=False):
    """y_i = (N − i)·1: the only survivor is the last index — a dominator in the last tile, every other point dominated
    from another tile only.  ``duplicate``: the winner stands at index 0 as well (first and last tile)."""
    Y = np.repeat((N - np.arange(N, dtype=np.float64))[:, None], k, axis=1)
    if duplicate:
        Y[0] = Y[-1]
    return Y
