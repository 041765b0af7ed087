"""The upper bound behind the arg-max chain's pruning, restated in numpy and held against the oracle.

Reference-mode EHVI-2D is Σ_i p2_i·G_i with σA = σ²₀·s00, σB = σ²₀·s01 (s01 > 0), p2_i = ψ(y2_i, y2_i, μ₁, σB) and
G_i = ψ(a, a, μ₀, σA) − ψ(b, b, μ₀, σA), a = y1[i−1] ≥ b = y1[i]; ψ(x, x, μ, σ) = E[(x − Y)⁺] increases in σ from
(x − μ)⁺.  Over σ²₀ ∈ [0, σ_f²]:

    value ≤ UB = Σ_i ψ(y2_i, y2_i, μ₁, σ_f²·s01)·[ψ(a, a, μ₀, σ_f²·s00) − (b − μ₀)⁺].

The device drops a candidate only if UB·(1 + 1e-9) + tiny < τ, tiny = 64·2⁻⁵²·Σ_i p2ub_i·(|a − μ₀| + |b − μ₀| + σ_f²·s00)
+ 1e-300; a violation here is a (candidate, σ²₀) whose oracle value that rule would have dropped against τ = the value
itself.  None is allowed, over fronts of 1, 2, 9 and 30 points, μ inside and far outside the front's box, σ²₀ at 0, at
σ_f² and on a 41-point grid between, at σ_f² = 0.09, 1 and 25: 4 fronts × 700 candidates × 43 variances × 3 = 361,200
cases.

On config 3's own training set the bound must also prune: fewer than 10% of 2^13 Sobol candidates may reach the true
maximum (the probes behind the change measured 0.0–1.3%).
"""
import numpy as np
import pytest

from oracle import acquisition as oacq
from oracle import gp as ogp
from oracle import pareto as opar


def bound(mu0, mu1, pf, r, s00, s01, sf2):
    """(UB, tiny) per candidate."""
    y1, y2 = oacq.stripes_2d(pf, r)
    n = len(y1) - 2
    sA, sB = sf2 * s00, sf2 * s01
    ub = np.zeros_like(mu0)
    scale = np.zeros_like(mu0)
    for i in range(1, n + 1):
        a, b = y1[i - 1], y1[i]
        g = np.maximum(oacq.psi_cal(a, a, mu0, sA) - np.maximum(b - mu0, 0.0), 0.0)
        p2 = np.maximum(oacq.psi_cal(y2[i], y2[i], mu1, sB), 0.0)
        ub = ub + p2 * g
        scale = scale + p2 * (np.abs(a - mu0) + np.abs(b - mu0) + sA)
    return ub, 64.0 * 2.0 ** -52 * scale + 1e-300


def pruned(ub, tiny, tau):
    """The device's rule: strict, and false on a NaN."""
    return ub * (1.0 + 1e-9) + tiny < tau


def _cache():
    from optimobo_amd.pareto import cached_samples
    cache = cached_samples(2, 5, seed=1)
    s00, s01 = oacq.cache_stats(cache)
    assert s00 > 0 and s01 > 0
    return cache, s00, s01


def _front(rng, P):
    """P mutually non-dominated points on a convex curve, jittered."""
    f1 = np.sort(rng.uniform(0.05, 0.95, P))
    f2 = (1.0 - np.sqrt(f1)) + 0.02 * rng.uniform(0, 1, P) * (P == 1)
    pf = opar.calc_pf(np.column_stack([f1, f2]))
    assert len(pf) == P
    return pf


@pytest.mark.parametrize("P", [1, 2, 9, 30])
def test_bound_dominates_the_oracle(P):
    rng = np.random.default_rng(100 + P)
    cache, s00, s01 = _cache()
    pf = _front(rng, P)
    r = pf.max(0) + 0.1
    lo, hi = pf.min(0), r
    n_c = 700
    # inside the front's box, around it, and far outside on either side of either objective
    mu = np.concatenate([rng.uniform(lo, hi, (300, 2)),
                         rng.uniform(lo - 0.5, hi + 0.5, (200, 2)),
                         rng.uniform(lo - 50.0, lo - 2.0, (50, 2)),
                         rng.uniform(hi + 2.0, hi + 50.0, (50, 2)),
                         np.column_stack([rng.uniform(lo[0] - 30, lo[0], 50), rng.uniform(hi[1], hi[1] + 30, 50)]),
                         np.column_stack([rng.uniform(hi[0], hi[0] + 30, 50), rng.uniform(lo[1] - 30, lo[1], 50)])])
    assert mu.shape == (n_c, 2)
    cases = 0
    for sf2 in (0.09, 1.0, 25.0):
        grid = np.concatenate([[0.0, sf2], np.linspace(0.0, sf2, 41)])
        ub, tiny = bound(mu[:, 0], mu[:, 1], pf, r, s00, s01, sf2)
        assert np.all(np.isfinite(ub)) and np.all(ub >= 0)
        for v0 in grid:
            with np.errstate(divide="ignore", invalid="ignore"):
                val = oacq.ehvi2d(mu.T, np.array([np.full(n_c, v0), np.zeros(n_c)]), pf, r, cache, mode="reference")
            bad = pruned(ub, tiny, val)
            assert not bad.any(), (P, sf2, v0, mu[bad][:3], ub[bad][:3], val[bad][:3])
            cases += len(val)
    assert cases == 3 * 43 * n_c   # 90,300 per front, 361,200 over the four


def test_bound_prunes_on_the_bench_training_set():
    import bench
    from optimobo_amd import pareto
    X, Y, ls, variances = bench.setup_problem(512, 6, tail_hi=0.3)
    Xc = bench.candidates(6, 0, 1 << 13)
    mu, var = [], []
    for o in range(2):
        m, v = ogp.ExactGP(X, Y[:, o], ls, variances[o]).predict(Xc)
        mu.append(m[:, 0])
        var.append(v[:, 0])
    mu, var = np.array(mu), np.array(var)
    pf = opar.calc_pf(Y)
    r = Y.max(axis=0) + 0.1 * (Y.max(axis=0) - Y.min(axis=0))
    cache = pareto.cached_samples(2, 5, seed=1)
    s00, s01 = oacq.cache_stats(cache)
    assert s01 > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        val = oacq.ehvi2d(mu, var, pf, r, cache, mode="reference")
    ub, tiny = bound(mu[0], mu[1], pf, r, s00, s01, variances[0])
    ok = np.isfinite(val) & (var[0] >= 0) & (var[0] <= variances[0])
    assert ok.mean() > 0.99
    assert not pruned(ub[ok], tiny[ok], val[ok]).any()
    best = np.nanmax(val)
    assert best > 0
    share = np.mean(~pruned(ub, tiny, best))
    print(f"candidates whose bound reaches the maximum: {share:.4%}")
    assert share < 0.10


def test_switch_and_stats_entry_match_the_header():
    import os
    import re
    from optimobo_amd import _lib
    src = open(os.path.join(os.path.dirname(__file__), "..", "include", "optimobo_hip.h")).read()
    assert re.search(r"OMB_DEBUG_ARGMAX_PRUNE\s*=\s*(\d+)", src).group(1) == str(_lib.DEBUG_ARGMAX_PRUNE)
    assert re.search(r"int omb_argmax_prune_stats\(omb_ctx\* ctx, int64_t\* stats_host\);", src)
    lib = _lib.load()
    assert lib.omb_argmax_prune_stats(None, None) == _lib.OMB_EINVAL
