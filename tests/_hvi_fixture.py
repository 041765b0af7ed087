"""Shared inputs and host references of the hypervolume-improvement tests (test_hvi_host.py, test_gpu_hvi.py,
test_gpu_thompson_batch.py).

A case is (k, P, seed): the front F is P points |N(0, 1)|^k normalised to unit length (drawn from
``default_rng(seed)``), the reference point r = 1.2·1, and 64 points F[rng.integers(0, P, 64)] + 0.15·N(0, 1) whose
rows 0..3 are F[0], r, r + 1 (each with HVI exactly 0) and F.min(0) − 0.1 (the largest value).  ``fixture`` builds a
case once per process; nothing changes what it returns."""
import functools

import numpy as np

from optimobo_amd import pareto

# (k, P, seed): boxes and the share of the 64 points with HVI > 0, as observed on the CPU
CASES = [(2, 1, 0), (2, 9, 1), (3, 12, 2), (4, 20, 3), (5, 12, 4), (8, 6, 5)]
BIG_CASE = (6, 30, 6)      # ≈ 8·10^4 boxes: the list cannot sit in LDS


def lo_hi(coords, boxes):
    k = coords.shape[0]
    lo = np.stack([coords[j][boxes[:, 2 * j]] for j in range(k)], 1)
    hi = np.stack([coords[j][boxes[:, 2 * j + 1]] for j in range(k)], 1)
    return lo, hi


def hvi_numpy(Y, coords, boxes, chunk=4096):
    """HVI(y) = Σ_b Π_j (hi_bj − max(y_j, lo_bj))⁺ for the rows of Y (N, k), boxes in list order."""
    Y = np.atleast_2d(np.asarray(Y, np.float64))
    lo, hi = lo_hi(coords, boxes)
    total = np.zeros(len(Y))
    for s in range(0, len(lo), chunk):
        t = np.clip(hi[None, s:s + chunk] - np.maximum(Y[:, None, :], lo[None, s:s + chunk]), 0.0, None)
        total += t.prod(axis=2).sum(axis=1)
    return total


@functools.lru_cache(maxsize=None)
def fixture(k, P, seed):
    """dict(F, r, Y (64, k), coords, boxes, ref (64,) = hvi_numpy(Y)); the arrays are read-only."""
    rng = np.random.default_rng(seed)
    F = np.abs(rng.standard_normal((P, k)))
    F /= np.linalg.norm(F, axis=1, keepdims=True)
    r = np.full(k, 1.2)
    Y = F[rng.integers(0, P, 64)] + 0.15 * rng.standard_normal((64, k))
    Y[0], Y[1], Y[2], Y[3] = F[0], r, r + 1.0, F.min(0) - 0.1
    coords, _, boxes = pareto.box_decomposition(F, r)
    ref = hvi_numpy(Y, coords, boxes)
    out = dict(F=F, r=r, Y=Y, coords=coords, boxes=boxes, ref=ref)
    for v in out.values():
        v.setflags(write=False)
    return out


def rtol(k, B):
    """(B + 3k)·2^-52: B − 1 additions and, per box, k subtractions and k − 1 products, every term ≥ 0."""
    return (B + 3 * k) * 2.0 ** -52
