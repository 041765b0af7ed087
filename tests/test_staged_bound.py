"""The staged order of the arg-max chain's pruning, restated in numpy and held against the oracle.

The bound of §29 is UB = Σ_i ψ(y2_i, y2_i, μ₁, sB)·[ψ(a_i, a_i, μ₀, sA) − (b_i − μ₀)⁺]⁺, sA = σ_f²·s00, sB = σ_f²·s01.  Its
second factor h(μ₀) rises below b_i and falls above it, so it is at most C_i = ψ(a_i, a_i, b_i, sA) for every μ₀, and

    value ≤ UB ≤ UB₁(μ₁) = Σ_i C_i·ψ(y2_i, y2_i, μ₁, sB)

needs objective 1's mean alone.  The device stores ubm1 = ub1·(1 + 1e-9) + tiny1 with ub1 taken at the low end μ̃₁ − ε₁ and
tiny1 = 64·2⁻⁵²·Σ_i p2_i·(|a_i| + |b_i| + 2M₀ + sA) + 1e-300, M₀ = σ_f²(0)·Σ_k |α_k(0)|·(1 + 2⁻²⁰) ≥ |μ₀|.

The staged selection: each group of G consecutive candidates gives the candidate with the smallest μ̃₁ as a seed — UB₁
decreases in μ₁, so that is the group's largest UB₁ at the centre of the interval, whatever the margins; τ₀ is the seeds'
best value; list A holds the other candidates unless τ₀ > 0 and ubm1 < τ₀; list B those of A unless τ₀ > 0 and ubm < τ₀ (ubm
the full margined bound of tests/test_prune_bound.py).  The arg-max must lie in seed ∪ B.
"""
import os
import re

import numpy as np
import pytest

from oracle import acquisition as oacq
from oracle import gp as ogp
from oracle import pareto as opar
from test_prune_bound import _cache, _front, bound

G = 256


def stripe_consts(pf, r, s00, s01, sf2, M0):
    """(C_i, W_i, y2_i) per stripe: the supremum of the second factor and tiny1's weight."""
    y1, y2 = oacq.stripes_2d(pf, r)
    n = len(y1) - 2
    sA = sf2 * s00
    a, b = y1[0:n], y1[1:n + 1]
    C = oacq.psi_cal(a, a, b, sA)
    W = np.abs(a) + np.abs(b) + 2.0 * M0 + sA
    return C, W, y2[1:n + 1]


def ubm1(mu1_low, pf, r, s00, s01, sf2, M0):
    """The margined objective-1 bound per candidate from the low end μ̃₁ − ε₁ of its mean."""
    C, W, y2 = stripe_consts(pf, r, s00, s01, sf2, M0)
    sB = sf2 * s01
    ub = np.zeros_like(mu1_low)
    scale = np.zeros_like(mu1_low)
    for Ci, Wi, yi in zip(C, W, y2):
        p2 = np.maximum(oacq.psi_cal(yi, yi, mu1_low, sB), 0.0)
        ub = ub + Ci * p2
        scale = scale + p2 * Wi
    return ub * (1.0 + 1e-9) + (64.0 * 2.0 ** -52 * scale + 1e-300)


def group_seeds(m1, group=G):
    """Each group's smallest comparable μ̃₁ (−∞ included), the lowest index on ties, the first where none compares."""
    seeds = []
    for first in range(0, len(m1), group):
        g = -m1[first:first + group]
        ok = ~np.isnan(g)
        seeds.append(first + (int(np.argmax(np.where(ok, g, -np.inf))) if ok.any() else 0))
    return np.array(seeds)


def staged_select(m1, u1, u, val, group=G):
    """→ (seeds, τ₀, A, B): index arrays, ascending.  m1: the screened means μ̃₁ (the seed's score); u1, u: ubm1 and
    ubm.  The device's rules: strict "<", false on a NaN."""
    seeds = group_seeds(m1, group)
    tau, _ = oacq.argmax(val[seeds])
    rest = np.ones(len(u1), bool)
    rest[seeds] = False
    with np.errstate(invalid="ignore"):
        keep_a = rest & ~((tau > 0) & (u1 < tau))
        keep_b = keep_a & ~((tau > 0) & (u < tau))
    return seeds, tau, np.flatnonzero(keep_a), np.flatnonzero(keep_b)


def _mus(rng, lo, hi):
    """test_prune_bound's 700 candidates: inside the front's box, around it and up to 50 units outside."""
    return np.concatenate([rng.uniform(lo, hi, (300, 2)),
                           rng.uniform(lo - 0.5, hi + 0.5, (200, 2)),
                           rng.uniform(lo - 50.0, lo - 2.0, (50, 2)),
                           rng.uniform(hi + 2.0, hi + 50.0, (50, 2)),
                           np.column_stack([rng.uniform(lo[0] - 30, lo[0], 50), rng.uniform(hi[1], hi[1] + 30, 50)]),
                           np.column_stack([rng.uniform(hi[0], hi[0] + 30, 50), rng.uniform(lo[1] - 30, lo[1], 50)])])


@pytest.mark.parametrize("P", [1, 2, 9, 30])
def test_second_factor_never_exceeds_its_stripe_constant(P):
    rng = np.random.default_rng(100 + P)
    _, s00, s01 = _cache()
    pf = _front(rng, P)
    r = pf.max(0) + 0.1
    y1, _ = oacq.stripes_2d(pf, r)
    M0 = 60.0
    for sf2 in (0.09, 1.0, 25.0):
        sA = sf2 * s00
        C, _, _ = stripe_consts(pf, r, s00, s01, sf2, M0)
        assert np.all(np.isfinite(C)) and np.all(C > 0)
        for i in range(1, P + 1):
            a, b = y1[i - 1], y1[i]
            m0 = np.concatenate([np.linspace(b - 3 * sA - 1, a + 3 * sA + 1, 4001), [b, a, -M0, M0]])
            h = oacq.psi_cal(a, a, m0, sA) - np.maximum(b - m0, 0.0)
            # the supremum is attained at μ₀ = b; what is left is the rounding of h's own terms
            slack = 8 * 2.0 ** -52 * (np.abs(a - m0) + np.abs(b - m0) + sA)
            assert np.all(h <= C[i - 1] + slack), (P, sf2, i, (h - C[i - 1]).max())
            assert h[4001] == pytest.approx(C[i - 1], rel=1e-12)


@pytest.mark.parametrize("P", [1, 2, 9, 30])
def test_ubm1_dominates_the_full_bound_and_the_oracle(P):
    rng = np.random.default_rng(100 + P)
    cache, s00, s01 = _cache()
    pf = _front(rng, P)
    r = pf.max(0) + 0.1
    mu = _mus(rng, pf.min(0), r)
    n_c = len(mu)
    M0 = np.abs(mu[:, 0]).max() * (1.0 + 2.0 ** -20)
    for sf2 in (0.09, 1.0, 25.0):
        ub, tiny = bound(mu[:, 0], mu[:, 1], pf, r, s00, s01, sf2)
        u = ub * (1.0 + 1e-9) + tiny
        for e1 in (0.0, 0.02):
            u1 = ubm1(mu[:, 1] - e1, pf, r, s00, s01, sf2, M0)
            assert np.all(np.isfinite(u1)) and np.all(u1 >= u), (P, sf2, e1, (u - u1).max())
        u1 = ubm1(mu[:, 1], pf, r, s00, s01, sf2, M0)
        for v0 in np.concatenate([[0.0, sf2], np.linspace(0.0, sf2, 41)]):
            with np.errstate(divide="ignore", invalid="ignore"):
                val = oacq.ehvi2d(mu.T, np.array([np.full(n_c, v0), np.zeros(n_c)]), pf, r, cache, mode="reference")
            bad = u1 < val
            assert not bad.any(), (P, sf2, v0, mu[bad][:3], u1[bad][:3], val[bad][:3])


_SETS = {}


def _bench_set(swap, log2n=17):
    """Config 3's training set with 2^17 unscrambled Sobol candidates: oracle means, variances and values, ubm1 and
    ubm; swap: the two objectives exchanged.  Built once."""
    if swap not in _SETS:
        import bench
        from optimobo_amd import pareto
        X, Y, ls, variances = bench.setup_problem(512, 6, tail_hi=0.3)
        N = 1 << log2n
        Xc = bench.candidates(6, 0, N)
        order = (1, 0) if swap else (0, 1)
        Y = Y[:, order]
        variances = [variances[o] for o in order]
        gps = [ogp.ExactGP(X, Y[:, o], ls, variances[o]) for o in range(2)]
        mu = np.empty((2, N))
        var0 = np.empty(N)
        for c0 in range(0, N, 1 << 14):
            sl = slice(c0, c0 + (1 << 14))
            m, v = gps[0].predict(Xc[sl])
            mu[0, sl], var0[sl] = m[:, 0], v[:, 0]
            mu[1, sl] = (ogp.KERNELS["matern52"](X, Xc[sl], gps[1].lengthscale, variances[1]).T @ gps[1].alpha)[:, 0]
        pf = opar.calc_pf(Y)
        r = Y.max(axis=0) + 0.1 * (Y.max(axis=0) - Y.min(axis=0))
        cache = pareto.cached_samples(2, 5, seed=1)
        s00, s01 = oacq.cache_stats(cache)
        with np.errstate(divide="ignore", invalid="ignore"):
            val = oacq.ehvi2d(np.array([mu[0], mu[1]]), np.array([var0, np.zeros(N)]), pf, r, cache, mode="reference")
        M0 = variances[0] * np.abs(gps[0].alpha).sum() * (1.0 + 2.0 ** -20)
        assert np.abs(mu[0]).max() <= M0
        ub, tiny = bound(mu[0], mu[1], pf, r, s00, s01, variances[0])
        _SETS[swap] = dict(N=N, mu=mu, val=val, u=ub * (1.0 + 1e-9) + tiny, M0=M0,
                           args=(pf, r, s00, s01, variances[0], M0))
    return _SETS[swap]


@pytest.mark.parametrize("e1", [0.0, 0.02])
def test_staged_selection_on_the_bench_training_set(e1):
    s = _bench_set(False)
    N, val = s["N"], s["val"]
    u1 = ubm1(s["mu"][1] - e1, *s["args"])
    assert np.all(u1 >= s["u"])
    seeds, tau, A, B = staged_select(s["mu"][1], u1, s["u"], val)
    # where no two bounds tie, the smallest mean is the largest bound at the centre
    u1c = ubm1(s["mu"][1], *s["args"])
    by_bound = np.array([f + int(np.argmax(u1c[f:f + G])) for f in range(0, N, G)])
    assert np.all((seeds == by_bound) | (u1c[seeds] == u1c[by_bound]))
    best_v, best_i = oacq.argmax(val)
    print(f"N={N} eps1={e1}: seeds {len(seeds)}, |A| {len(A)} ({len(A) / N:.2%}), |B| {len(B)}, tau0/max {tau / best_v}")
    assert best_v > 0 and len(seeds) == N // G
    assert best_i in seeds or best_i in B
    assert tau == best_v
    assert len(A) / N < 0.20
    assert set(B) <= set(A) and not set(A) & set(seeds)
    # nothing that reaches τ₀ is dropped at either stage
    kept = np.zeros(N, bool)
    kept[seeds] = kept[B] = True
    assert not np.any(val[~kept] >= tau)


def test_staged_selection_with_the_objectives_swapped():
    """The bad case: the objective whose mean decides least comes first and list A keeps most of the batch."""
    s = _bench_set(True, 16)
    N, val = s["N"], s["val"]
    u1 = ubm1(s["mu"][1] - 0.02, *s["args"])
    seeds, tau, A, B = staged_select(s["mu"][1], u1, s["u"], val)
    best_v, _ = oacq.argmax(val)
    print(f"swapped, N={N}: |A| {len(A)} ({len(A) / N:.2%}), |B| {len(B)}, tau0/max {tau / best_v}")
    kept = np.zeros(N, bool)
    kept[seeds] = kept[B] = True
    with np.errstate(invalid="ignore"):
        assert not np.any(val[~kept] >= tau)


def _toy(N=3 * G + 5, seed=5):
    rng = np.random.default_rng(seed)
    val = rng.uniform(0.0, 1.0, N)
    u = val + rng.uniform(0.0, 0.3, N)
    u1 = u + rng.uniform(0.0, 0.5, N)
    return val, u, u1


def _check(val, u, u1, m1=None):
    """m1 defaults to −ubm1: a uniform margin, under which the smallest mean is the largest bound."""
    seeds, tau, A, B = staged_select(-u1 if m1 is None else m1, u1, u, val)
    best_v, best_i = oacq.argmax(val)
    pool = np.concatenate([seeds, B])
    got_v, got_p = oacq.argmax(val[pool])
    if best_i >= 0:
        # the final reduction compares original indices: the lowest index among the maxima of seed ∪ B
        winners = pool[val[pool] == got_v]
        assert got_v == best_v and winners.min() == best_i, (best_v, best_i, got_v, winners)
    assert len(np.intersect1d(seeds, A)) == 0 and set(B) <= set(A)
    return seeds, tau, A, B


def test_edge_cases_of_the_two_stages():
    N = 3 * G + 5
    val, u, u1 = _toy()
    _check(val, u, u1)
    # a group of NaN μ̃₁ and ubm1: its first candidate is the seed and the rest stay through stage A (a NaN never
    # compares)
    v2, w2, w1 = val.copy(), u.copy(), u1.copy()
    w1[G:2 * G] = np.nan
    seeds, tau, A, B = _check(v2, w2, w1)
    assert seeds[1] == G and set(range(G + 1, 2 * G)) <= set(A)
    # a +∞ ubm1: with μ̃₁ = −∞ it is a seed (the lowest index where two share a group) or kept by stage A; with an
    # infinite ε₁ or M₀ alone (a finite μ̃₁) it is no seed and kept by stage A; its full bound decides stage B
    w1 = u1.copy()
    w1[[7, 9, G + 3]] = np.inf
    seeds, tau, A, B = _check(val, u, w1)
    assert seeds[0] == 7 and 9 in A and seeds[1] == G + 3
    w = u.copy()
    w[9] = np.inf
    _, _, A, B = _check(val, w, w1)
    assert 9 in A and 9 in B
    m1 = -u1
    seeds, tau, A, B = _check(val, w, w1, m1)
    assert 7 not in seeds and {7, 9, G + 3} <= set(A) and 9 in B
    # τ₀ ≤ 0, −∞ and NaN keep everything
    for v in (np.zeros(N), np.full(N, -1.0), np.full(N, -np.inf), np.full(N, np.nan)):
        seeds, tau, A, B = staged_select(-u1, u1, u, v)
        assert not tau > 0 and len(A) == len(B) == N - len(seeds)
    # ties inside a group and across groups: the lowest index wins, and a candidate tied with τ₀ stays (strict "<")
    v2, w2, w1 = val.copy(), u.copy(), u1.copy()
    top = 2.0
    for i in (5, 40, G + 1, 3 * G + 4):
        v2[i] = w2[i] = w1[i] = top
    seeds, tau, A, B = _check(v2, w2, w1)
    assert tau == top and seeds[0] == 5 and seeds[1] == G + 1 and seeds[3] == 3 * G + 4 and 40 in B
    # A empty: every seed's bound is its value and nothing else reaches τ₀
    v2 = np.full(N, 0.1)
    w2, w1 = v2 + 0.05, v2 + 0.1
    v2[::G] = w2[::G] = w1[::G] = 1.0
    seeds, tau, A, B = _check(v2, w2, w1)
    assert len(A) == 0 and len(B) == 0 and tau == 1.0
    # a single candidate: the seed alone
    seeds, tau, A, B = staged_select(-u1[:1], u1[:1], u[:1], val[:1])
    assert list(seeds) == [0] and len(A) == 0 and len(B) == 0


def test_switch_and_entries_match_the_header():
    from optimobo_amd import _lib
    root = os.path.join(os.path.dirname(__file__), "..")
    hdr = open(os.path.join(root, "include", "optimobo_hip.h")).read()
    api = open(os.path.join(root, "optimobo_amd", "csrc", "omb_api.hip")).read()
    internal = open(os.path.join(root, "optimobo_amd", "csrc", "omb_internal.h")).read()
    assert re.search(r"OMB_DEBUG_ARGMAX_STAGED\s*=\s*(\d+)", hdr).group(1) == str(_lib.DEBUG_ARGMAX_STAGED) == "18"
    assert "omb_debug_set(ctx, OMB_DEBUG_ARGMAX_STAGED, m)" in hdr
    assert re.search(r"\{OMB_DEBUG_ARGMAX_STAGED, &omb_ctx::argmax_staged, 0, 1, nullptr\}", api)
    assert re.search(r"int argmax_staged = 1;", api)
    assert re.search(r"int omb_argmax_stage_stats\(omb_ctx\* ctx, int64_t\* stats_host\);", hdr)
    assert re.search(r"int omb_posterior_screen_list\(omb_ctx\* ctx, const double\* Xc_dev, int64_t N, "
                     r"const int32_t\* idx_dev,\s+const int32_t\* count_dev, int obj, double\* mu_dev, "
                     r"double\* eps_dev\);", hdr)
    assert int(re.search(r"constexpr int kPruneSeedGroup = (\d+);", internal).group(1)) == G
    lib = _lib.load()
    assert lib.omb_argmax_stage_stats(None, None) == _lib.OMB_EINVAL
    assert lib.omb_posterior_screen_list(None, None, 0, None, None, 0, None, None) == _lib.OMB_EINVAL
