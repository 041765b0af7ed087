"""Per-iteration host geometry for the acquisition kernels (pymoo/pygmo-free).

These run once per BO iteration on at most a few thousand objective vectors (SURVEY.md §8f
row 3), so they are host numpy; the per-candidate work they feed runs on the GPU.

* ``calc_pf``   — first non-dominated front, as util_functions.py:64-77 gets it from
                  pygmo.fast_non_dominated_sorting (row order kept, duplicates kept).
* ``stripes_2d``— the PF sorted by f2 ascending, the order EHVI_2D_aux walks
                  (util_functions.py:98-101); this is what omb_ehvi2d takes.
* ``decompose_into_cells`` — emo.py:55-152's 2-D cell list in closed form, reference-exact
                  including the lower-bound quirk (lower f2 of cells j ≥ 1 = max(I0, I1)).
* ``hypervolume`` — exact dominated volume (pymoo HV at optimisers.py:216-220; pygmo at
                  util_functions.py:198-199): sweep in 2-D, z-slab sweep in 3-D, WFG beyond.
* ``cached_samples`` / ``cache_stats`` — optimisers.py:121-141 and the np.cov constants EHVI
                  needs (util_functions.py:163).
"""
import numpy as np
from scipy.stats import norm, qmc

MAX_OBJ = 8          # OMB_MAX_OBJ (include/optimobo_hip.h)


def nondominated_mask(Y, block=2048):
    """mask[i] = no row of Y Pareto-dominates row i (minimisation)."""
    Y = np.asarray(Y, np.float64)
    n = len(Y)
    mask = np.ones(n, bool)
    for s in range(0, n, block):
        B = Y[s:s + block]                                         # candidates to test
        le = np.all(Y[:, None, :] <= B[None, :, :], axis=2)       # Y[a] <= B[b]
        lt = np.any(Y[:, None, :] < B[None, :, :], axis=2)
        mask[s:s + block] = ~np.any(le & lt, axis=0)
    return mask


def calc_pf(Y):
    Y = np.asarray(Y, np.float64)
    if len(Y) < 2:
        return Y
    return Y[nondominated_mask(Y)]


def stripes_2d(pf):
    pf = np.asarray(pf, np.float64).reshape(-1, 2)
    return np.ascontiguousarray(pf[np.argsort(pf[:, 1], kind="stable")])


def decompose_into_cells(pf, ideal_point, max_point):
    pf = np.asarray(pf, np.float64).reshape(-1, 2)
    ideal = np.asarray(ideal_point, np.float64)
    mx = np.asarray(max_point, np.float64)
    p = pf[np.argsort(pf[:, 0], kind="stable")]
    P = len(p)
    up = np.empty((P + 1, 2))
    lo = np.empty((P + 1, 2))
    up[0] = (p[0, 0], max(p[0, 1], mx[1]))
    lo[0] = ideal
    up[1:P, 0] = p[1:, 0]
    up[1:P, 1] = p[:-1, 1]
    up[P] = (max(p[-1, 0], mx[0]), p[-1, 1])
    lo[1:, 0] = np.maximum(p[:, 0], ideal[0])
    lo[1:, 1] = max(ideal[0], ideal[1])
    return np.ascontiguousarray(np.stack([up, lo], axis=1))


def hypervolume(points, ref):
    P = np.asarray(points, np.float64)
    r = np.asarray(ref, np.float64)
    if P.size == 0:
        return 0.0
    P = P[np.all(P < r, axis=1)]
    if len(P) == 0:
        return 0.0
    P = calc_pf(P)
    k = P.shape[1]
    if k == 1:
        return float(r[0] - P[:, 0].min())
    if k == 2:
        P = P[np.argsort(P[:, 0], kind="stable")]
        f2 = np.minimum.accumulate(P[:, 1])
        prev = np.concatenate(([r[1]], f2[:-1]))
        return float(np.sum((r[0] - P[:, 0]) * np.clip(prev - f2, 0.0, None)))
    # sweep the last objective: each slab between consecutive levels is a (k-1)-D volume
    order = np.argsort(P[:, -1], kind="stable")
    P = P[order]
    levels = np.append(P[:, -1], r[-1])
    total = 0.0
    for i in range(len(P)):
        h = levels[i + 1] - levels[i]
        if h > 0:
            total += hypervolume(P[: i + 1, :-1], r[:-1]) * h
    return float(total)


class _BoxBudget(Exception):
    pass


def _front_ranks(F):
    """Distinct non-dominated rows of an integer point set, in np.unique's (canonical) row order."""
    F = np.unique(F, axis=0)
    if len(F) < 2:
        return F
    le = np.all(F[:, None, :] <= F[None, :, :], axis=2)
    np.fill_diagonal(le, False)                       # rows are distinct: a ≤ b with a ≠ b is dominance
    return F[~le.any(axis=0)]


def _boxes_3d_ranks(F, top, budget):
    """box_decomposition's 3-D slab sweep on grid ranks: F (n, 3) distinct non-dominated rows."""
    order = np.argsort(F[:, 2], kind="stable")
    pts = F[order].tolist()
    t0, t1, t2 = top
    rows = []
    stair = []                                        # 2-D front of the points below the slab, x ascending
    i, n = 0, len(pts)
    z = 0
    while True:
        z_next = pts[i][2] if i < n else t2
        x_lo, y_hi = 0, t1
        for x, y in stair:
            rows.append((x_lo, x, 0, y_hi, z, z_next))
            x_lo, y_hi = x, y
        rows.append((x_lo, t0, 0, y_hi, z, z_next))
        if len(rows) > budget:
            raise _BoxBudget
        if i >= n:
            break
        z = z_next
        while i < n and pts[i][2] == z:               # the level's points enter the staircase
            x, y = pts[i][0], pts[i][1]
            i += 1
            if any(a <= x and b <= y for a, b in stair):
                continue
            stair = [(a, b) for a, b in stair if not (x <= a and y <= b)]
            stair.append((x, y))
            stair.sort()
    return np.asarray(rows, np.uint16)


def _boxes_ranks(F, top, budget, memo):
    """Boxes (B, 2d) of grid ranks covering what the front F (n, d) leaves non-dominated in [0, top].

    Recursion over the last objective: between two consecutive levels of it the region is the (d−1)-D region
    of the points at or below the lower level (their projected front), times the level interval.  F holds
    distinct non-dominated rows, so the projected front changes at every level and no two slabs merge.
    Sub-fronts recur across slabs; memo keeps their boxes.  budget: boxes this call may return.
    """
    d = F.shape[1]
    key = (d, F.tobytes())
    hit = memo.get(key)
    if hit is not None:
        if len(hit) > budget:
            raise _BoxBudget
        return hit
    if d == 3:
        out = _boxes_3d_ranks(F, top[:3], budget)
        memo[key] = out
        return out
    if len(F) == 0:
        return np.array([[0, t] for t in top[:d]], np.uint16).reshape(1, 2 * d)
    levels = np.unique(F[:, -1])
    parts = [np.array([[0, t] for t in top[:d - 1]] + [[0, levels[0]]], np.uint16).reshape(1, 2 * d)]
    count = 1
    front = np.zeros((0, d - 1), F.dtype)
    for a, z in enumerate(levels):
        front = _front_ranks(np.vstack((front, F[F[:, -1] == z, :-1])))
        sub = _boxes_ranks(front, top, budget - count, memo)
        count += len(sub)
        if count > budget:
            raise _BoxBudget
        zz = np.empty((len(sub), 2), np.uint16)
        zz[:, 0] = z
        zz[:, 1] = levels[a + 1] if a + 1 < len(levels) else top[d - 1]
        parts.append(np.hstack((sub, zz)))
    out = np.concatenate(parts)
    memo[key] = out
    return out


class BoxBudgetError(ValueError):
    """box_decomposition: the front needs more than max_boxes boxes (a ValueError, as it always was; callers that
    fall back on it alone — the drivers' Thompson batches — catch this class)."""


def _box_decomposition_kd(pf, ref, max_boxes):
    k = ref.size
    pts = pf[np.all(pf < ref, axis=1)] if pf.size else np.zeros((0, k))
    pts = calc_pf(pts) if len(pts) > 1 else pts
    grids = [np.concatenate(([-np.inf], np.unique(pts[:, j]), [ref[j]])) for j in range(k)]
    C = max(len(g) for g in grids)
    if C > 65535:
        raise ValueError("box_decomposition: front too large for 16-bit grid indices")
    top = [len(g) - 1 for g in grids]
    ranks = np.stack([np.searchsorted(grids[j], pts[:, j]) for j in range(k)], axis=1).astype(np.int32)
    ranks = _front_ranks(ranks.reshape(-1, k))
    try:
        boxes = _boxes_ranks(ranks, top, int(max_boxes), {})
    except _BoxBudget:
        raise BoxBudgetError(f"box_decomposition: a front of {len(ranks)} points in k={k} objectives needs more "
                             f"than max_boxes={int(max_boxes)} boxes") from None
    coords = np.stack([np.concatenate((g, np.full(C - len(g), g[-1]))) for g in grids])
    return (np.ascontiguousarray(coords), np.array([len(g) for g in grids], np.int32), np.ascontiguousarray(boxes))


def box_decomposition(pf, ref, max_boxes=1 << 20):
    """Disjoint boxes covering the part of (−∞, ref] the front does not dominate (2 ≤ k ≤ 8).

    Input of omb_ehvi_boxes[_k] (the exact "textbook" EHVI): HVI(y) = Σ_b Π_j (hi_bj − max(y_j, lo_bj))⁺.
    Returns (coords (k, C) f64 — per objective the sorted grid [−∞, front values…, ref_j] padded
    with ref_j —, ncoord (k,) int32, boxes (B, 2k) uint16 = [lo_idx_0, hi_idx_0, lo_idx_1, …]).
    3-D: one slab per distinct f3 level; inside a slab the 2-D staircase of the points below it.
    k ≥ 4: the same sweep by recursion over the last objective (_boxes_ranks), on grid ranks, so the
    boxes are exact; their number grows like P^(k/2)…P^(k−1), and a ValueError is raised
    as soon as the count passes max_boxes (k ≥ 4 only; the k ≤ 3 lists are at most P² boxes).
    """
    pf = np.asarray(pf, np.float64)
    ref = np.asarray(ref, np.float64)
    k = ref.size
    if 4 <= k <= MAX_OBJ:
        return _box_decomposition_kd(pf.reshape(-1, k), ref, max_boxes)
    if k not in (2, 3):
        raise NotImplementedError(f"box_decomposition: 2 to {MAX_OBJ} objectives")
    pts = pf[np.all(pf < ref, axis=1)] if pf.size else np.zeros((0, k))
    pts = calc_pf(pts) if len(pts) > 1 else pts
    grids = [np.concatenate(([-np.inf], np.unique(pts[:, j]), [ref[j]])) for j in range(k)]

    def staircase(P2):
        """(x_lo, x_hi, y_hi) of the 2-D non-dominated stripes below ref[:2]."""
        if len(P2) == 0:
            return [(-np.inf, ref[0], ref[1])]
        F = calc_pf(P2)
        F = F[np.argsort(F[:, 0], kind="stable")]
        xb = np.concatenate(([-np.inf], F[:, 0], [ref[0]]))
        yt = np.concatenate(([ref[1]], F[:, 1]))
        return [(xb[i], xb[i + 1], yt[i]) for i in range(len(F) + 1) if xb[i + 1] > xb[i]]

    rows = []
    if k == 2:
        for xl, xh, yh in staircase(pts):
            rows.append((xl, xh, -np.inf, yh))
    else:
        z_levels = grids[2]                      # −∞, distinct f3 values, ref_3
        for a in range(len(z_levels) - 1):
            below = pts[pts[:, 2] <= z_levels[a], :2]
            for xl, xh, yh in staircase(below):
                rows.append((xl, xh, -np.inf, yh, z_levels[a], z_levels[a + 1]))
    vals = np.asarray(rows, np.float64).reshape(-1, 2 * k)
    idx = np.empty(vals.shape, np.int64)
    for j in range(k):
        for s in (0, 1):
            idx[:, 2 * j + s] = np.searchsorted(grids[j], vals[:, 2 * j + s])
    C = max(len(g) for g in grids)
    coords = np.stack([np.concatenate((g, np.full(C - len(g), g[-1]))) for g in grids])
    if C > 65535:
        raise ValueError("box_decomposition: front too large for 16-bit grid indices")
    return (np.ascontiguousarray(coords), np.array([len(g) for g in grids], np.int32),
            np.ascontiguousarray(idx.astype(np.uint16)))


def threshold_lists(b):
    """One objective's "decompositions": for every sampled best value b_s the grid [−∞, b_s] and the single box
    (0, 1), whose improvement is (b_s − y)⁺ — the input of ``pack_box_lists`` for the noisy EI."""
    b = np.asarray(b, np.float64).reshape(-1)
    return [(np.array([[-np.inf, v]]), np.array([2], np.int32), np.array([[0, 1]], np.uint16)) for v in b]


def feasible_fronts(F, G, max_point, max_boxes=1 << 20):
    """Every path's own feasible front: F (k, S, n) the objectives' and G (c, S, n) the constraint models' path values
    at the same n rows (g ≤ 0 feasible).  Per path s the rows with every G[:, s] ≤ 0, then ``calc_pf`` and
    ``box_decomposition(PF_s, max_point, max_boxes)``; a path with no feasible row gets the empty front's single box.
    k = 1 (``max_point`` None): ``threshold_lists`` of the smallest feasible value, and of the path's largest value
    over all rows where none is feasible (nothing known to beat: a feasible candidate improves on the worst seen).
    → (fronts, decompositions): S arrays (P_s, k) (k = 1: b (S,)) and the input of ``pack_box_lists``."""
    F = np.asarray(F, np.float64)
    G = np.asarray(G, np.float64)
    if F.ndim != 3 or G.ndim != 3 or G.shape[1:] != F.shape[1:]:
        raise ValueError(f"feasible_fronts: F {F.shape} and G {G.shape} are not (k, S, n) and (c, S, n)")
    k, S, _ = F.shape
    if (k == 1) != (max_point is None):
        raise ValueError("feasible_fronts: one objective takes max_point=None, several need the reference point")
    feas = np.all(G <= 0.0, axis=0)                                  # (S, n); a NaN is infeasible
    if k == 1:
        b = np.array([F[0, s, feas[s]].min() if feas[s].any() else F[0, s].max() for s in range(S)])
        return b, threshold_lists(b)
    fronts = [calc_pf(np.ascontiguousarray(F[:, s, feas[s]].T)) if feas[s].any() else np.zeros((0, k))
              for s in range(S)]
    return fronts, [box_decomposition(pf, max_point, max_boxes=max_boxes) for pf in fronts]


def pack_box_lists(decomps):
    """S ``box_decomposition`` results (or ``threshold_lists``) of the same k as one input of omb_hvi_paths:
    (coords (S, k, C) f64, box_off (S + 1,) int32, boxes (ΣB, 2k) uint16).  C is the largest grid; a shorter grid is
    padded with its last coordinate, as ``box_decomposition`` pads within one grid.  List s is rows
    box_off[s]..box_off[s + 1] of boxes; an empty front still has one box (the whole of (−∞, ref])."""
    decomps = list(decomps)
    if not decomps:
        raise ValueError("pack_box_lists: no decompositions")
    k = decomps[0][0].shape[0]
    if any(d[0].ndim != 2 or d[0].shape[0] != k or d[2].ndim != 2 or d[2].shape[1] != 2 * k for d in decomps):
        raise ValueError("pack_box_lists: the decompositions disagree on the number of objectives")
    if any(len(d[2]) < 1 for d in decomps):
        raise ValueError("pack_box_lists: an empty box list")
    C = max(d[0].shape[1] for d in decomps)
    coords = np.empty((len(decomps), k, C), np.float64)
    for s, d in enumerate(decomps):
        c = d[0].shape[1]
        coords[s, :, :c] = d[0]
        coords[s, :, c:] = d[0][:, -1:]
    box_off = np.zeros(len(decomps) + 1, np.int64)
    np.cumsum([len(d[2]) for d in decomps], out=box_off[1:])
    if box_off[-1] > np.iinfo(np.int32).max:
        raise ValueError("pack_box_lists: more than 2^31 boxes")
    boxes = np.ascontiguousarray(np.concatenate([np.asarray(d[2], np.uint16) for d in decomps]))
    return coords, box_off.astype(np.int32), boxes


def cached_samples(k, sample_exponent, seed=None):
    s = qmc.Sobol(d=k, scramble=True, seed=seed).random_base2(m=sample_exponent)
    return np.ascontiguousarray(np.column_stack([norm.ppf(s[:, i]) for i in range(k)]))


def cache_stats(cache):
    c = np.cov(cache[:, 0], cache[:, 1])
    return float(c[0, 0]), float(c[0, 1])
