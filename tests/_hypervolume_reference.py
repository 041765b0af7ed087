"""Host references of the exact hypervolume (omb_hypervolume / omb_hypervolume_contrib), minimisation, rows
are points.

``hv_grid(P, r, dtype)``  the grid-sweep formula itself, restated in numpy: the rows with every coordinate finite and
below r are kept; objectives 0..k-3 are cut at the kept rows' distinct values u_j (then r_j); a cell c has weight
Π_j (u_j[c_j + 1] − u_j[c_j]), multiplied left to right; the rows with rank_j ≤ c_j for every grid objective, walked in
(y_{k-2}, y_{k-1}) order with ymin = r_{k-1}, add (r_{k-2} − y_{k-2})·(ymin − y_{k-1}) whenever y_{k-1} < ymin; the
cells' w·A are added one after another.  With ``np.longdouble`` it is the reference of the GPU tests (64-bit
significand: its own rounding is 2^-11 of an fp64 ulp per operation); with ``np.float64`` it is the plain restatement,
which differs from the kernel only in the order the cells are added in.  ``pareto.hypervolume`` — a recursive sweep of
the last objective over non-dominated prefixes — is the independent algorithm both are checked against
(tests/test_hypervolume_host.py).

``contributions(P, r, dtype)``  HV(P) − HV(P without row i) for every row, by recomputing.

The inputs of the tests are built here too, from seeds."""
import itertools

import numpy as np

LD = np.longdouble


def kept_rows(P, r):
    r = np.asarray(r, np.float64)
    P = np.asarray(P, np.float64).reshape(-1, r.size)
    with np.errstate(invalid="ignore"):
        return np.all(np.isfinite(P) & (P < r), axis=1)


def hv_grid(P, r, dtype=LD):
    r64 = np.asarray(r, np.float64)
    k = r64.size
    P = np.asarray(P, np.float64).reshape(-1, k)
    P = P[kept_rows(P, r64)].astype(dtype)
    r = r64.astype(dtype)
    n = len(P)
    if n == 0:
        return dtype(0)
    if k == 1:
        return r[0] - P[:, 0].min()
    P = P[np.lexsort((P[:, k - 1], P[:, k - 2]))]
    g = k - 2
    grids = [np.unique(P[:, j]) for j in range(g)]
    ranks = np.stack([np.searchsorted(grids[j], P[:, j]) for j in range(g)], axis=1) if g else np.zeros((n, 0), int)
    widths = [np.diff(np.concatenate((grids[j], r[j:j + 1]))) for j in range(g)]
    shape = [len(u) for u in grids]
    cells = np.array(list(itertools.product(*map(range, shape))), dtype=int).reshape(int(np.prod(shape)), g)
    w = np.ones(len(cells), dtype)
    for j in range(g):
        w = widths[j][cells[:, j]] if j == 0 else w * widths[j][cells[:, j]]
    ymin = np.full(len(cells), r[k - 1], dtype)
    A = np.zeros(len(cells), dtype)
    for i in range(n):                               # the walk, every cell at once
        q = np.all(ranks[i] <= cells, axis=1) & (P[i, k - 1] < ymin)
        A[q] += (r[k - 2] - P[i, k - 2]) * (ymin[q] - P[i, k - 1])
        ymin[q] = P[i, k - 1]
    return np.cumsum(w * A)[-1]                      # one cell after another


def contributions(P, r, dtype=LD, rows=None):
    """HV(P) − HV(P without row i) for the rows ``rows`` (default: all) → (hv, array)."""
    P = np.asarray(P, np.float64)
    hv = hv_grid(P, r, dtype)
    rows = range(len(P)) if rows is None else rows
    return hv, np.array([hv - hv_grid(np.delete(P, i, axis=0), r, dtype) for i in rows], dtype)


# ---- the inputs of tests/test_hypervolume_host.py and tests/test_gpu_hypervolume.py
def sphere(rng, n, k):
    """n points of the positive unit sphere: a non-dominated front (reference point 1.1)."""
    X = np.abs(rng.normal(size=(n, k))) + 1e-3
    return X / np.linalg.norm(X, axis=1, keepdims=True)


def lattice(rng, n, k, levels=4):
    """n points with integer coordinates in [0, levels): heavy ties in every objective, duplicates and dominated rows
    (reference point ``levels``)."""
    return rng.integers(0, levels, size=(n, k)).astype(np.float64)


def dressed(rng, kind, n, k):
    """(P (N, k), r (k,)) with exactly n kept rows, in shuffled order: the ``kind`` points, of which (n ≥ 8) two are
    exact duplicates of others and two are dominated by others, and dropped rows around them — one coordinate equal
    to r_j, one above it, a NaN, a +inf and a −inf row."""
    r = np.full(k, 1.1 if kind == "sphere" else 4.0)
    make = sphere if kind == "sphere" else lattice
    extra = 4 if n >= 8 else 0
    core = make(rng, n - extra, k)
    rows = [core]
    if extra:
        rows.append(core[:2])                                                # duplicates
        dom = core[2:4].copy()
        dom[:, rng.integers(0, k)] += 0.05 if kind == "sphere" else 0.0      # dominated (lattice: a third duplicate pair)
        dom[1] = np.minimum(core[3] + (0.02 if kind == "sphere" else 1.0), r - 0.05)
        rows.append(dom)
    base = core[0] if n - extra > 0 else np.full(k, 0.5)
    bad = np.tile(base, (5, 1))
    bad[0, 0] = r[0]
    bad[1, k - 1] = r[k - 1] + 0.25
    bad[2, k // 2] = np.nan
    bad[3, 0] = np.inf
    bad[4, k - 1] = -np.inf
    rows.append(bad)
    P = np.vstack(rows)
    P = P[rng.permutation(len(P))]
    assert kept_rows(P, r).sum() == n
    return P, r
