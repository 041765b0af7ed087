"""Shared by tests/test_constraints_host.py (CPU) and tests/test_gpu_constraints.py (GPU): the surrogates of the
constraint tests, the probability of feasibility and its product rule restated in numpy, and the drivers' problem.

Surrogates are built as tests/test_gpu_var_mask.py builds its own: uniform inputs in [0, 1]^d, its lengthscale rule,
σ_f² = var(y), 1003 candidates.  Constraint targets: g₁ = x₀ + x₁ − 1, g₂ = 0.3 − x₁ (feasible: g ≤ 0).
"""
import numpy as np
from scipy.stats import norm

from oracle import gp as ogp

N_CAND = 1003          # no multiple of 16, 32 or 64
POF_EPS = 1e-5


def lengthscales(rng, n, d):
    """tests/test_gpu_var_mask.py's rule: a few nearest-neighbour spacings of n uniform points in [0, 1]^d."""
    return rng.uniform(1.0, 2.0, d) * np.sqrt(d) * n ** (-1.0 / d)


def objectives(X):
    """Four smooth objective targets (columns) on [0, 1]^d, d ≥ 2."""
    f1 = X[:, 0]
    g = 1 + 9.0 / (X.shape[1] - 1) * X[:, 1:].sum(1)
    return np.column_stack([f1, g * (1 - np.sqrt(f1 / g)), (1 + X[:, 1]) * (1.2 - f1),
                            0.5 + 0.5 * np.cos(2.0 * X[:, 0] + X[:, 1])])


def constraints(X, c=2):
    """c ≤ 7 constraint targets: g₁, g₂, then looser copies of them (g₁ − 0.4, g₂ − 0.4, g₁ − 0.5, …), whose feasible
    sets contain the first two's with a margin — they are there to be multiplied, not to move the bands."""
    base = [X[:, 0] + X[:, 1] - 1.0, 0.3 - X[:, 1]]
    return np.column_stack([base[j % 2] - (0.0 if j < 2 else 0.3 + 0.1 * (j // 2)) for j in range(c)])


def problem(n, d, seed, k, c, n_cand=N_CAND):
    """k objective and c ≤ 7 constraint surrogates on the same n inputs: (gps [(X, y, ℓ, σ_f²)], Y (n, 4), Xc, and the
    oracle's μ, σ² (k + c, N))."""
    rng = np.random.default_rng(seed)
    Xc = rng.uniform(0, 1, (n_cand, d))
    X = rng.uniform(0, 1, (n, d))
    Y = objectives(X)
    T = np.column_stack([Y[:, :k], constraints(X, c)])
    gps, mu, var = [], [], []
    for o in range(k + c):
        ls = lengthscales(rng, n, d)
        vf = float(np.var(T[:, o]))
        gps.append((X, T[:, o], ls, vf))
        m, v = ogp.ExactGP(X, T[:, o], ls, vf).predict(Xc)
        mu.append(m[:, 0])
        var.append(v[:, 0])
    return gps, Y, Xc, np.array(mu), np.array(var)


# ------------------------------------------------------------------------------------------- probability of feasibility
def pof(mu, var, pof_eps=POF_EPS):
    """F (N,) = Π_j Φ(−μ_j / sqrt(σ²_j + pof_eps)) over the rows of mu, var (c, N), with scipy's Φ."""
    mu, var = np.atleast_2d(mu), np.atleast_2d(var)
    return np.prod(norm.cdf(-mu / np.sqrt(var + pof_eps)), axis=0)


def bands(F):
    """Fractions of candidates with F in (0.01, 0.99), F ≥ 0.99 and F ≤ 0.01."""
    F = np.asarray(F)
    return float(np.mean((F > 0.01) & (F < 0.99))), float(np.mean(F >= 0.99)), float(np.mean(F <= 0.01))


def assert_bands(F, tag=""):
    """The condition the constraint tests put on their inputs (not a measurement of the code under test): a weight
    that is all 0 or all 1 would show nothing."""
    mid, top, bottom = bands(F)
    assert mid >= 0.05 and top >= 0.05 and bottom >= 0.25, (tag, mid, top, bottom)


def pof_value(value, k, pof_eps=POF_EPS):
    """value(mu, var) over k objective rows → the weighted acquisition over k + c rows."""
    return lambda mu, var: value(mu[:k], var[:k]) * pof(mu[k:], var[k:], pof_eps)


def pof_partials(value, partials, k, pof_eps=POF_EPS):
    """The product rule of a·F over tests/test_grad_reference.py's partials: rows 0..k−1 are the plan's ∂a/∂μ, ∂a/∂σ²
    times F; rows k.. are a·Π_{q≠j}Φ(z_q)·φ(z_j)·(−1/s_j) and a·Π_{q≠j}Φ(z_q)·φ(z_j)·μ_j/(2 s_j³),
    s_j = sqrt(σ²_j + pof_eps), z_j = −μ_j/s_j."""
    def f(mu, var):
        a = value(mu[:k], var[:k])
        dm0, dv0 = partials(mu[:k], var[:k])
        s = np.sqrt(var[k:] + pof_eps)
        z = -mu[k:] / s
        P, p = norm.cdf(z), norm.pdf(z)
        F = P.prod(0)
        dm, dv = np.zeros_like(mu), np.zeros_like(mu)
        dm[:k], dv[:k] = dm0 * F, dv0 * F
        for j in range(len(z)):
            others = a * np.prod(np.delete(P, j, axis=0), axis=0)
            dm[k + j] = others * p[j] * (-1.0 / s[j])
            dv[k + j] = others * p[j] * mu[k + j] / (2.0 * s[j] ** 3)
        return dm, dv
    return f


# ------------------------------------------------------------------------------------------- the drivers' problem
def driver_problem(n_ieq_constr=1, n_eq_constr=0, n_obj=2):
    """Two variables on [0, 1]², the constraint x₀ + x₁ ≥ 1.5 (g = 1.5 − x₀ − x₁ ≤ 0: the corner triangle, 12.5 % of
    the box), and two objectives with optima at (0.2, 0.1) — infeasible — and (0.9, 0.9) — inside the triangle.  The
    unconstrained Pareto set, between the two optima, is mostly infeasible; the constrained one has a stretch inside
    the triangle and a stretch on its edge.  A problem whose constrained front lay on the edge alone would not do: a
    maximiser of a·F settles there at F ≈ ½, |g| of the order of 1e-3, and which side of 0 such a proposal falls on
    says nothing about the weight."""
    from optimobo_amd.problem import ElementwiseProblem

    class Corner(ElementwiseProblem):
        def __init__(self):
            super().__init__(n_var=2, n_obj=n_obj, n_ieq_constr=n_ieq_constr, n_eq_constr=n_eq_constr,
                             xl=np.array([0.0, 0.0]), xu=np.array([1.0, 1.0]))

        def _evaluate(self, x, out, *args, **kwargs):
            f = [(x[0] - 0.2) ** 2 + 2.0 * (x[1] - 0.1) ** 2, 1.5 * (x[0] - 0.9) ** 2 + (x[1] - 0.9) ** 2]
            out["F"] = (f + [x[0] * x[1]] * n_obj)[:n_obj]

        def _evaluate_constraints(self, x, out, *args, **kwargs):
            out["G"] = [1.5 - x[0] - x[1]] * n_ieq_constr
            if n_eq_constr:
                out["H"] = [x[0] - x[1]] * n_eq_constr

    return Corner()
