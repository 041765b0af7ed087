"""The arg-max chain's seed by bound, restated in numpy on top of test_prune_bound.bound and held against
the oracle.

The device computes ubm = ub·(1 + 1e-9) + tiny for every candidate, takes as seed the candidate with the largest
comparable ubm of each run of G consecutive candidates (lowest index on ties; the run's first candidate where none
compares), evaluates the seed exactly — τ is its best value — and keeps c ⇔ c is not its group's seed and not
(τ > 0 and ubm[c] < τ).  Held here, for G = 256 and 1024 on 2^15 unscrambled Sobol candidates and four training sets:
the lowest index among the oracle's maxima is a seed or a survivor, no candidate whose oracle value reaches τ is
dropped, and seed + survivors ≤ N/64 = 512 — a condition, not a measurement: the probes behind the change counted 32 to
156 against 2,049 to 2,220 for the strided seed of §29, which must also come out larger here.  Then the rule's edge
cases on synthetic bounds: a group of NaN, a +∞ bound, τ ≤ 0 and τ = −∞, and ties inside one group and across groups.
"""
import os
import re

import numpy as np
import pytest

from oracle import acquisition as oacq
from oracle import gp as ogp
from oracle import pareto as opar
from test_prune_bound import bound, pruned

N = 1 << 15
SETS = {"config 3": (512, 0.3), "uniform box": (512, 1.0), "n 256": (256, 0.3), "n 130": (130, 0.3)}
ROOT = os.path.join(os.path.dirname(__file__), "..")


def group_seeds(ubm, G):
    """The seed of each run of G candidates: the largest ubm that compares (ubm == ubm), the lowest index on ties, the
    run's first candidate where none compares."""
    seeds = []
    for first in range(0, len(ubm), G):
        u = ubm[first:first + G]
        idx = np.flatnonzero(u == u)
        seeds.append(first + (int(idx[np.argmax(u[idx])]) if len(idx) else 0))
    return np.array(seeds)


def seed_tau(val, seeds):
    """The best comparable value of the seed (argmax_pass2: NaN and −∞ never enter), −∞ where there is none."""
    v = val[seeds]
    v = v[(v == v) & (v > -np.inf)]
    return v.max() if len(v) else -np.inf


def keep_flags(ubm, seeds, tau, G):
    """prune_threshold_kernel: strict "<", false on a NaN, τ ≤ 0, −∞ or NaN keeps everything; the seeds are left out."""
    c = np.arange(len(ubm))
    with np.errstate(invalid="ignore"):
        return (c != seeds[c // G]) & ~((tau > 0.0) & (ubm < tau))


def covered(ubm, val, G):
    """(seeds, keep, τ) of the whole rule, and the checks that make the pair the dense one."""
    seeds = group_seeds(ubm, G)
    assert np.all(np.diff(seeds) > 0) and np.array_equal(seeds // G, np.arange(len(seeds)))   # ascending, one per group
    tau = seed_tau(val, seeds)
    keep = keep_flags(ubm, seeds, tau, G)
    assert not keep[seeds].any()                                  # the seed and the survivors are disjoint
    evaluated = keep.copy()
    evaluated[seeds] = True
    ok = (val == val) & (val > -np.inf)
    if ok.any():
        best = np.flatnonzero(ok & (val == val[ok].max()))[0]     # the dense chain's index: the lowest among the maxima
        assert evaluated[best], (best, val[best], ubm[best], tau)
        assert evaluated[ok & (val >= tau)].all()                 # nothing that reaches τ is dropped
    return seeds, keep, tau


_CASES = {}


def _case(name):
    """Oracle values and the margined bound of the N candidates under one training set, computed once."""
    if name not in _CASES:
        import bench
        from optimobo_amd import pareto
        n, tail_hi = SETS[name]
        X, Y, ls, variances = bench.setup_problem(n, 6, tail_hi=tail_hi)
        Xc = bench.candidates(6, 0, N)
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
        assert s00 > 0 and s01 > 0
        with np.errstate(divide="ignore", invalid="ignore"):
            val = oacq.ehvi2d(mu, var, pf, r, cache, mode="reference")
        ub, tiny = bound(mu[0], mu[1], pf, r, s00, s01, variances[0])
        _CASES[name] = dict(val=val, ub=ub, tiny=tiny, ubm=ub * (1.0 + 1e-9) + tiny)
    return _CASES[name]


@pytest.mark.parametrize("G", [256, 1024])
@pytest.mark.parametrize("name", list(SETS))
def test_seed_by_bound_keeps_the_maximum_and_evaluates_few(name, G):
    c = _case(name)
    val, ubm = c["val"], c["ubm"]
    assert np.nanmax(val) > 0
    seeds, keep, tau = covered(ubm, val, G)
    assert len(seeds) == N // G
    # the strided seed of §29 on the same numbers
    strided = np.arange(0, N, 16)
    tau_s = seed_tau(val, strided)
    assert tau_s > 0.0
    keep_s = ~pruned(c["ub"], c["tiny"], tau_s)
    keep_s[strided] = False
    ours, theirs = len(seeds) + int(keep.sum()), len(strided) + int(keep_s.sum())
    print(f"{name}, G = {G}: tau / max = {tau / np.nanmax(val):.4f}, seed {len(seeds)} + survivors {int(keep.sum())} "
          f"= {ours}; strided: tau / max = {tau_s / np.nanmax(val):.4f}, {len(strided)} + {int(keep_s.sum())} "
          f"= {theirs}")
    assert ours <= N // 64
    assert theirs > ours


@pytest.mark.parametrize("G", [256, 1024])
def test_a_group_of_nan_bounds(G):
    rng = np.random.default_rng(G)
    n = 4 * G + 37
    val = rng.uniform(0.1, 1.0, n)
    ubm = val * rng.uniform(1.0, 3.0, n)
    ubm[G:2 * G] = np.nan                                         # group 1 compares nowhere
    val[G + 5] = np.nan                                           # and some of its values are NaN as well
    seeds, keep, tau = covered(ubm, val, G)
    assert seeds[1] == G                                          # its first candidate is the seed
    assert keep[G + 1:2 * G].all() and not keep[G]                # and the rest survive
    assert tau > 0
    # every bound a NaN: the first candidates are the seeds, everything else survives
    seeds, keep, tau = covered(np.full(n, np.nan), val, G)
    assert np.array_equal(seeds, np.arange(0, n, G)) and keep.sum() == n - len(seeds)


@pytest.mark.parametrize("G", [256, 1024])
def test_an_infinite_bound_is_seed_or_kept(G):
    rng = np.random.default_rng(7 + G)
    n = 3 * G
    val = rng.uniform(0.1, 1.0, n)
    ubm = val * 1.5
    for slot in (3, G + 9, G + 200, 2 * G + G - 1):                # one, two in the same group, a group's last slot
        ubm[slot] = np.inf
    seeds, keep, tau = covered(ubm, val, G)
    assert list(seeds) == [3, G + 9, 3 * G - 1]                   # +∞ wins its group, the lower index on a tie
    assert keep[G + 200] and np.isfinite(tau)


@pytest.mark.parametrize("G", [256, 1024])
@pytest.mark.parametrize("fill", [0.0, -1.0, -np.inf, np.nan])
def test_nothing_is_dropped_without_a_positive_threshold(G, fill):
    n = 2 * G + 11
    val = np.full(n, fill)
    ubm = np.abs(np.random.default_rng(3).normal(size=n)) + 1e-300
    seeds, keep, tau = covered(ubm, val, G)
    assert not tau > 0.0
    assert len(seeds) == 3 and keep.sum() == n - 3


@pytest.mark.parametrize("G", [256, 1024])
def test_ties_inside_a_group_and_across_groups(G):
    rng = np.random.default_rng(11 + G)
    n = 4 * G + 5
    base = rng.uniform(0.1, 1.0, n)
    factor = rng.uniform(1.0, 1.2, n)
    for places in ([G + 7, G + 90], [G + 7, 3 * G + 1], [5, G - 1, G, 4 * G + 4], [2 * G + 100, 2 * G + 101, 3 * G]):
        val = base.copy()
        val[places] = 2.0                                         # the maximum, duplicated
        ubm = val * factor
        ubm[places[1:]] = val[places[1:]]                         # the later copies' bounds are tight: they tie with τ
        seeds, keep, tau = covered(ubm, val, G)                   # holds the lowest index among the maxima
        assert keep[places[0]] or places[0] in seeds
        for p in places:                                          # and every other copy reaches τ: none is dropped
            assert keep[p] or p in seeds


def test_switch_admits_the_seed_by_bound():
    hdr = open(os.path.join(ROOT, "include", "optimobo_hip.h")).read()
    doc = re.search(r"omb_debug_set\(ctx, OMB_DEBUG_ARGMAX_PRUNE, m\)(.*?)omb_debug_set\(ctx, OMB_DEBUG_ARGMAX_SCREEN",
                    hdr, re.S).group(1)
    for value in ("1 (default)", "3 the same at any batch size", "2 the earlier order at any batch size",
                  "0 the dense chain"):
        assert value in doc, value
    api = open(os.path.join(ROOT, "optimobo_amd", "csrc", "omb_api.hip")).read()
    assert re.search(r"\{OMB_DEBUG_ARGMAX_PRUNE, &omb_ctx::argmax_prune, 0, 3,", api)
    internal = open(os.path.join(ROOT, "optimobo_amd", "csrc", "omb_internal.h")).read()
    assert int(re.search(r"constexpr int kPruneSeedGroup = (\d+);", internal).group(1)) in (256, 1024)
