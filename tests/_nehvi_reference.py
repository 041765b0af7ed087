"""numpy restatement of omb_hvi_paths and the inputs the noisy-EHVI tests share.

    t_s(y)  = Σ_{b in list s} Π_j (hi_bj − max(y_j, lo_bj))⁺
    α(y)    = ((…((0 + t_0) + t_1) + …) + t_{S−1}) / S

written twice: ``dtype=np.float64`` in the kernel's order (slices of 1024 boxes counted from the list's own start, each
summed from 0 in list order, the slices added in slice order, the paths in path order; the product over objectives
0..k−2 first, then the last factor — without the kernel's one fused multiply-add, which numpy does not have) and
``dtype=np.longdouble``, the reference both are measured against.  ``np.maximum`` propagates NaN, as the kernel does.
"""
import numpy as np

from optimobo_amd import pareto

SLICE = 1024


def t_path(y, coords, boxes, dtype=np.float64):
    """t_s of the points y (k, N) over one grid coords (k, C) and list boxes (B, 2k) → (N,)."""
    y = np.asarray(y, dtype)
    g = np.asarray(coords, dtype)
    boxes = np.asarray(boxes, np.int64)
    k, N = y.shape
    zero = dtype(0.0)
    total = np.zeros(N, dtype)
    with np.errstate(invalid="ignore"):
        for b0 in range(0, len(boxes), SLICE):
            bl = boxes[b0:b0 + SLICE]
            prod = None
            for j in range(k):
                lo = g[j, bl[:, 2 * j]][:, None]
                hi = g[j, bl[:, 2 * j + 1]][:, None]
                t = np.maximum(hi - np.maximum(y[j][None, :], lo), zero)
                prod = t if prod is None else prod * t
            # cumsum adds in list order from the first term (0 + x = x exactly); ufunc.reduce would add pairwise
            total = total + np.cumsum(prod, axis=0, dtype=dtype)[-1]
    return total


def path_values(y, coords, box_off, boxes, dtype=np.float64):
    """(S, N): t_s of y (k, S, N) over list s."""
    S = len(box_off) - 1
    return np.stack([t_path(np.asarray(y)[:, s, :], coords[s], boxes[box_off[s]:box_off[s + 1]], dtype)
                     for s in range(S)])


def alpha(y, coords, box_off, boxes, dtype=np.float64):
    """α of y (k, S, N) → (N,)."""
    ts = path_values(y, coords, box_off, boxes, dtype)
    total = np.zeros(ts.shape[1], dtype)
    for t in ts:
        total = total + t
    return total / dtype(len(ts))


def mean_in_order(ts):
    """((0 + t_0) + t_1 + …) / S over the rows of ts (S, N) in fp64: what omb_hvi_paths does with its t_s."""
    total = np.zeros(ts.shape[1])
    for t in ts:
        total = total + t
    return total / float(len(ts))


# ------------------------------------------------------------------------------------------------ shared inputs
def front(k, P, rng, scale=1.0):
    """P mutually non-dominated points in (0, scale)^k: on the simplex Σ_j f_j = 1, scaled."""
    if P == 0:
        return np.zeros((0, k))
    return scale * rng.dirichlet(np.ones(k), size=P)


def lists_for(k, sizes, rng, ref=1.1):
    """One box list per entry of ``sizes`` (front sizes; 0 is the empty front) for k ≥ 2 objectives, reference point
    ref·1, packed: (fronts, (coords, box_off, boxes))."""
    r = np.full(k, ref)
    fronts = [front(k, P, rng) for P in sizes]
    return fronts, pareto.pack_box_lists([pareto.box_decomposition(f, r) for f in fronts])


def thresholds_for(S, rng):
    b = rng.normal(size=S)
    return b, pareto.pack_box_lists(pareto.threshold_lists(b))


def candidates(k, S, N, rng, lo=-0.2, hi=1.3):
    """Path values (k, S, N): most inside the fronts' range, some past the reference point."""
    return rng.uniform(lo, hi, size=(k, S, N))


# ------------------------------------------------------------------------------------------------ the estimator
def ehvi_boxes(mu, var, coords, boxes):
    """The exact EHVI Σ_b Π_j σ_j [h((hi − μ_j)/σ_j) − h((lo − μ_j)/σ_j)], h(t) = tΦ(t) + φ(t), of the moments
    mu, var (k, N) over one box decomposition, in fp64 (scipy's Φ, φ) → (N,)."""
    from scipy.stats import norm
    mu, sd = np.asarray(mu, np.float64), np.sqrt(np.asarray(var, np.float64))
    k = mu.shape[0]

    def h(t):
        with np.errstate(invalid="ignore"):
            return np.where(np.isneginf(t), 0.0, t * norm.cdf(t) + norm.pdf(t))
    total = np.zeros(mu.shape[1])
    for b in np.asarray(boxes, np.int64):
        term = np.ones(mu.shape[1])
        for j in range(k):
            lo, hi = coords[j, b[2 * j]], coords[j, b[2 * j + 1]]
            term = term * sd[j] * (h((hi - mu[j]) / sd[j]) - h((lo - mu[j]) / sd[j]))
        total = total + term
    return total


ESTIMATOR = dict(n=24, d=2, m=64, S=16, installs=16, seed=11, first_install=100)


def posterior64(state, Xc):
    """μ, σ² (N,) of a noise-free GPState at Xc in plain fp64 numpy."""
    import _paths_reference as P
    X, ls, var, alpha, Linv = P._bits(state)
    K = P._kernel64(X, np.asarray(Xc, np.float64), ls, var, state.kernel)
    A = Linv.T @ (Linv @ K)
    return alpha @ K, var - np.sum(K * A, 0)


def estimator_case():
    """The estimator test's fixed problem: two noise-free GP states with a trade-off on n shared inputs of [0, 1]^d,
    the observed front and its reference point, the 8 candidates of a fixed random pool, each at least 0.12 from every
    training input, with the largest exact EHVI, and that EHVI (fp64 numpy) → (states, X, Y, r, Xc, exact)."""
    from optimobo_amd.gp import GPState
    e = ESTIMATOR
    rng = np.random.default_rng(e["seed"])
    X = rng.uniform(0.0, 1.0, (e["n"], e["d"]))
    Y = np.stack([X[:, 0] ** 2 + 0.3 * np.sin(5.0 * X[:, 1]) + 0.3,
                  (1.0 - X[:, 0]) ** 2 + 0.3 * np.cos(4.0 * X[:, 1]) + 0.3], 1)
    states = [GPState(X, Y[:, o], rng.uniform(0.5, 0.9, e["d"]), float(np.var(Y[:, o])) + 0.1, kernel="matern52",
                      noise=0.0) for o in range(2)]
    r = Y.max(0) + 0.1
    pool = rng.uniform(0.0, 1.0, (400, e["d"]))
    pool = pool[np.min(np.linalg.norm(X[None, :, :] - pool[:, None, :], axis=2), axis=1) >= 0.12]
    coords, _, boxes = pareto.box_decomposition(pareto.calc_pf(Y), r)
    mv = [posterior64(st, pool) for st in states]
    a = ehvi_boxes(np.stack([m for m, _ in mv]), np.stack([v for _, v in mv]), coords, boxes)
    top = np.argsort(-a, kind="stable")[:8]
    return states, X, Y, r, pool[top], a[top]


def estimator_inputs(states, g):
    """Install g's draws, as AcquisitionEngine.sample_paths(S, m, seed=g, lower=0, upper=1) makes them: one
    numpy.random.default_rng(g), one draw_path_inputs per model in model order."""
    from optimobo_amd.paths import draw_path_inputs
    e = ESTIMATOR
    rng = np.random.default_rng(g)
    return [draw_path_inputs(st.kernel, e["n"], e["d"], e["S"], e["m"], rng, lower=np.zeros(e["d"]),
                             upper=np.ones(e["d"]), lengthscale=np.asarray(st.lengthscale, np.float64))
            for st in states]


def estimator_values(F, Fc, r):
    """The S per-path values t_s at the candidates from path values F (k, S, n) at the training inputs and Fc (k, S, N)
    at the candidates — fronts, decompositions and the box sum on the host → (S, N)."""
    S = F.shape[1]
    decomps = [pareto.box_decomposition(pareto.calc_pf(np.ascontiguousarray(F[:, s, :].T)), r) for s in range(S)]
    return path_values(Fc, *pareto.pack_box_lists(decomps))


def standard_errors(ts, exact):
    """|mean − exact| / (std / sqrt(count)) per candidate, ts (count, N)."""
    return np.abs(ts.mean(0) - exact) / (ts.std(0, ddof=1) / np.sqrt(len(ts)))
