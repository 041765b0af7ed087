"""Objective 1's bound as one cut on its screened mean, restated in numpy as the device runs it.

ubm1(m) = Σ_i C_i·ψ(y2_i, y2_i, m, sB)·(1 + 1e-9) + tiny1(m) (tests/test_staged_bound.py) decreases in its one argument,
the low end m = μ̃₁ − ε₁, so "ubm1 < τ₀" for every candidate is one comparison against m*, the smallest number found with
the computed ubm1(m*) < τ₀:

    bracket  ubm1 at the largest y2; below τ₀: step left by (y2 range + sB)·2^k until a point is not below; not below:
             the right end is that y2 + 40·sB, where ubm1 is 1e-300 — if even that is not below τ₀, no bracket;
    solve    Newton on log ubm1 towards τ₀·(1 − 5e-8), a bisection step where the proposal leaves the bracket, until
             τ₀·(1 − 1e-7) ≤ ubm1(hi) < τ₀ or the ends are neighbouring doubles;
    walk     at most three predecessors of hi that still test below τ₀.

m* = +∞ (keep everything) where τ₀ is not > 0, where M₀ or a stripe constant is not finite and where no bracket exists.
A candidate past the seed goes to list A unless m* < ∞ and μ̃₁ − ε₁ ≥ m*.
"""
import os
import re

import numpy as np
import pytest

from oracle import acquisition as oacq
from test_prune_bound import _cache, _front, bound
from test_staged_bound import G, _bench_set, _mus, group_seeds, staged_select, stripe_consts, ubm1

BRACKET_STEPS, SOLVE_STEPS, WALK_STEPS = 64, 64, 3


def ubm1_at(m, C, W, y2, sB):
    """(ubm1(m), D = Σ_i C_i·Φ(u_i)) at one point."""
    with np.errstate(invalid="ignore", over="ignore"):
        u = (y2 - m) / sB
        cdf = oacq.norm_cdf(u)
        p2 = np.fmax(sB * oacq.norm_pdf(u) + (y2 - m) * cdf, 0.0)      # fmax: a NaN term counts 0, as the device's
        p2 = np.where(np.isnan(p2), 0.0, p2)
        ub, scale, D = np.sum(C * p2), np.sum(p2 * W), np.sum(C * cdf)
        return ub * (1.0 + 1e-9) + (64.0 * 2.0 ** -52 * scale + 1e-300), D


def solve_cut(tau, C, W, y2, sB, M0):
    """→ (m*, ubm1(m*), evaluations): prune_cut_kernel's loops."""
    inf = np.inf
    fin = np.isfinite(M0) and np.all(np.isfinite(C)) and np.all(np.isfinite(W)) and np.all(np.isfinite(y2))
    hi, uhi, lo, n_eval = inf, np.nan, -inf, 0
    if not (fin and tau > 0.0):
        return hi, uhi, n_eval
    ymax, ymin = y2.max(), y2.min()
    f, D = ubm1_at(ymax, C, W, y2, sB)
    n_eval += 1
    mN, fN, DN = ymax, f, D
    have_lo = False
    if f < tau:
        hi, uhi = ymax, f
        step = (ymax - ymin) + sB
        for _ in range(BRACKET_STEPS):
            m = ymax - step
            step = 2.0 * step
            f, D = ubm1_at(m, C, W, y2, sB)
            n_eval += 1
            if f < tau:
                hi, uhi, mN, fN, DN = m, f, m, f, D
            else:
                lo, have_lo = m, True
                break
    else:
        lo, have_lo = ymax, True
        m = ymax + 40.0 * sB
        f, D = ubm1_at(m, C, W, y2, sB)
        n_eval += 1
        if f < tau:
            hi, uhi = m, f
    if have_lo and hi < inf:
        tt, tw = tau * (1.0 - 5e-8), tau * (1.0 - 1e-7)
        done = uhi >= tw
        for _ in range(SOLVE_STEPS):
            if done:
                break
            with np.errstate(all="ignore"):
                m = mN + fN * np.log(fN / tt) / (DN * (1.0 + 1e-9))
            if not (lo < m < hi):
                m = lo + 0.5 * (hi - lo)
            if not (lo < m < hi):
                break
            f, D = ubm1_at(m, C, W, y2, sB)
            n_eval += 1
            mN, fN, DN = m, f, D
            if f < tau:
                hi, uhi = m, f
                done = f >= tw
            else:
                lo = m
        for _ in range(WALK_STEPS):
            m = np.nextafter(hi, -inf)
            if not m > lo:
                break
            f, _ = ubm1_at(m, C, W, y2, sB)
            n_eval += 1
            if not f < tau:
                break
            hi, uhi = m, f
    return hi, uhi, n_eval


def cut_list(low, seeds, mstar):
    """List A by the cut: not a seed and not (m* < ∞ and the low end ≥ m*); a NaN low end never compares."""
    rest = np.ones(len(low), bool)
    rest[seeds] = False
    with np.errstate(invalid="ignore"):
        return np.flatnonzero(rest & ~((mstar < np.inf) & (low >= mstar)))


def check_cut(tau, mstar, ustar, consts, sB):
    """ubm1(m*) < τ₀ and the resolution: ubm1(m*) ≥ τ₀·(1 − 1e-7), or m*'s predecessor is not below τ₀."""
    assert np.isfinite(mstar) and ustar < tau, (mstar, ustar, tau)
    assert ustar == ubm1_at(mstar, *consts, sB)[0]
    if not ustar >= tau * (1.0 - 1e-7):
        assert not ubm1_at(np.nextafter(mstar, -np.inf), *consts, sB)[0] < tau, (mstar, ustar, tau)


def check_lists(low, seeds, tau, A_ref, u1, val, mstar):
    """The cut's list against the per-candidate one: they differ only inside the 1e-6 window around τ₀, and nothing
    whose value reaches τ₀ is dropped."""
    A = cut_list(low, seeds, mstar)
    diff = np.setxor1d(A, A_ref)
    assert np.all(np.abs(u1[diff] - tau) < 1e-6 * tau), (len(diff), u1[diff][:5], tau)
    kept = np.zeros(len(low), bool)
    kept[seeds] = kept[A] = True
    with np.errstate(invalid="ignore"):
        assert not np.any(val[~kept] >= tau)
    return A, diff


@pytest.mark.parametrize("P", [1, 2, 9, 30])
def test_cut_on_random_fronts(P):
    rng = np.random.default_rng(100 + P)
    cache, s00, s01 = _cache()
    pf = _front(rng, P)
    r = pf.max(0) + 0.1
    mu = _mus(rng, pf.min(0), r)
    n_c = len(mu)
    M0 = np.abs(mu[:, 0]).max() * (1.0 + 2.0 ** -20)
    for sf2 in (0.09, 1.0, 25.0):
        C, W, y2 = stripe_consts(pf, r, s00, s01, sf2, M0)
        sB = sf2 * s01
        ub, tiny = bound(mu[:, 0], mu[:, 1], pf, r, s00, s01, sf2)
        u = ub * (1.0 + 1e-9) + tiny
        with np.errstate(divide="ignore", invalid="ignore"):
            val = oacq.ehvi2d(mu.T, np.array([np.full(n_c, 0.5 * sf2), np.zeros(n_c)]), pf, r, cache, mode="reference")
        for e1 in (0.0, 0.02):
            low = mu[:, 1] - e1
            u1 = ubm1(low, pf, r, s00, s01, sf2, M0)
            seeds, tau, A_ref, _ = staged_select(mu[:, 1], u1, u, val)
            assert tau > 0
            # the single-point evaluation is the vector one's arithmetic
            assert ubm1_at(low[17], C, W, y2, sB)[0] == pytest.approx(u1[17], rel=1e-13)
            mstar, ustar, n_eval = solve_cut(tau, C, W, y2, sB, M0)
            check_cut(tau, mstar, ustar, (C, W, y2), sB)
            A, diff = check_lists(low, seeds, tau, A_ref, u1, val, mstar)
            print(f"P={P} sf2={sf2} e1={e1}: m* {mstar:.6g}, {n_eval} evaluations, |A| {len(A)} ({len(A_ref)}), "
                  f"differ {len(diff)}")
            assert n_eval <= 24                                            # Newton, not the bisection fallback


@pytest.mark.parametrize("swap,log2n,e1", [(False, 17, 0.0), (False, 17, 0.02), (True, 16, 0.0), (True, 16, 0.02)])
def test_cut_on_the_bench_training_set(swap, log2n, e1):
    s = _bench_set(swap, log2n)
    pf, r, s00, s01, sf2, M0 = s["args"]
    C, W, y2 = stripe_consts(pf, r, s00, s01, sf2, M0)
    sB = sf2 * s01
    low = s["mu"][1] - e1
    u1 = ubm1(low, *s["args"])
    seeds, tau, A_ref, _ = staged_select(s["mu"][1], u1, s["u"], s["val"])
    mstar, ustar, n_eval = solve_cut(tau, C, W, y2, sB, M0)
    check_cut(tau, mstar, ustar, (C, W, y2), sB)
    A, diff = check_lists(low, seeds, tau, A_ref, u1, s["val"], mstar)
    print(f"swap={swap} e1={e1}: tau0 {tau:.6g}, m* {mstar:.9g}, ubm1(m*)/tau0 - 1 = {ustar / tau - 1:.3g}, {n_eval} "
          f"evaluations, |A| by cut {len(A)}, per candidate {len(A_ref)}, symmetric difference {len(diff)}")
    # the per-candidate reference alone: no candidate of these sets lies inside the window, so the lists are equal
    assert int(np.sum(np.abs(u1 - tau) < 1e-6 * tau)) == 0 and len(diff) == 0
    assert n_eval <= 24


def _toy_consts(sf2=1.0, P=9, seed=3):
    rng = np.random.default_rng(seed)
    _, s00, s01 = _cache()
    pf = _front(rng, P)
    r = pf.max(0) + 0.1
    M0 = 7.0
    C, W, y2 = stripe_consts(pf, r, s00, s01, sf2, M0)
    return C, W, y2, sf2 * s01, M0


def test_edges_of_the_cut():
    C, W, y2, sB, M0 = _toy_consts()
    inf, nan = np.inf, np.nan
    # τ₀ zero, negative, −∞ or NaN; M₀, a C_i or a W_i not finite: no cut, everything past the seed stays
    for tau in (0.0, -1.0, -inf, nan):
        assert solve_cut(tau, C, W, y2, sB, M0)[0] == inf
    assert solve_cut(0.1, C, W + inf, y2, sB, inf)[0] == inf
    Cb = C.copy()
    Cb[2] = nan
    assert solve_cut(0.1, Cb, W, y2, sB, M0)[0] == inf
    low = np.array([0.3, nan, -inf, inf, 0.1, 5.0])
    seeds = np.array([0])
    assert list(cut_list(low, seeds, inf)) == [1, 2, 3, 4, 5]
    # no bracket: τ₀ at or under the 1e-300 floor of the bound
    assert solve_cut(1e-300, C, W, y2, sB, M0)[0] == inf and solve_cut(5e-324, C, W, y2, sB, M0)[0] == inf
    # a τ₀ just above the floor, and a huge one, left of every stripe: both solved
    for tau in (3e-300, 1e-200, 1e-30, 1e-3, 1.0, 1e6, 1e15):
        mstar, ustar, n_eval = solve_cut(tau, C, W, y2, sB, M0)
        check_cut(tau, mstar, ustar, (C, W, y2), sB)
        assert n_eval <= 1 + BRACKET_STEPS + SOLVE_STEPS + WALK_STEPS, (tau, n_eval)
    # the low ends: NaN and −∞ stay, +∞ goes (τ₀ > 0 and a cut exists), exactly m* goes, its predecessor stays
    tau = 0.05
    mstar, ustar, _ = solve_cut(tau, C, W, y2, sB, M0)
    low = np.array([mstar - 1.0, nan, -inf, inf, mstar, np.nextafter(mstar, -inf), mstar + 1.0])
    assert list(cut_list(low, seeds, mstar)) == [1, 2, 5]
    # a τ₀ above ubm1 at every candidate's low end: A is empty
    low = np.linspace(mstar + 0.1, mstar + 3.0, 2 * G + 9)
    seeds = group_seeds(low)
    assert np.all(np.array([ubm1_at(m, C, W, y2, sB)[0] for m in low[::37]]) < tau)
    assert len(cut_list(low, seeds, mstar)) == 0
    # N = 1: the seed alone
    assert len(cut_list(np.array([mstar - 1.0]), np.array([0]), mstar)) == 0
    # solving against a larger τ₀ moves the cut left: a decreasing bound
    assert solve_cut(2 * tau, C, W, y2, sB, M0)[0] < mstar


def test_the_computed_bound_follows_its_monotone_majorant():
    """§34's argument uses monotonicity of the real-arithmetic majorant only: the computed ubm1 need not be monotone
    bit for bit (one neighbour step in 131,071 rises by 3.9e-13 on config 3's set).  Whatever rise there is stays far
    inside the 1e-9 factor."""
    C, W, y2, sB, _ = _toy_consts(P=30)
    m = np.sort(np.random.default_rng(8).uniform(y2.min() - 2.0, y2.max() + 8 * sB, 20000))
    f = np.array([ubm1_at(x, C, W, y2, sB)[0] for x in m])
    rise = (f[1:] - f[:-1]) / f[:-1]
    print(f"largest relative rise between sorted neighbours: {rise.max():.3g}")
    assert rise.max() < 1e-11


def test_switch_and_entry_match_the_header():
    from optimobo_amd import _lib
    root = os.path.join(os.path.dirname(__file__), "..")
    hdr = open(os.path.join(root, "include", "optimobo_hip.h")).read()
    api = open(os.path.join(root, "optimobo_amd", "csrc", "omb_api.hip")).read()
    acq = open(os.path.join(root, "optimobo_amd", "csrc", "omb_acquisition.hip")).read()
    assert re.search(r"OMB_DEBUG_ARGMAX_CUT\s*=\s*(\d+)", hdr).group(1) == str(_lib.DEBUG_ARGMAX_CUT) == "19"
    assert "omb_debug_set(ctx, OMB_DEBUG_ARGMAX_CUT, m)" in hdr
    assert re.search(r"\{OMB_DEBUG_ARGMAX_CUT, &omb_ctx::argmax_cut, 0, 1, nullptr\}", api)
    assert re.search(r"int argmax_cut = 1;", api)
    assert re.search(r"int omb_argmax_cut_stats\(omb_ctx\* ctx, double\* stats_host\);", hdr)
    # the restatement's trip counts are the kernel's
    for name, v in (("kCutBracketSteps", BRACKET_STEPS), ("kCutSolveSteps", SOLVE_STEPS), ("kCutWalkSteps", WALK_STEPS)):
        assert int(re.search(rf"constexpr int {name} = (\d+);", acq).group(1)) == v
    lib = _lib.load()
    assert lib.omb_argmax_cut_stats(None, None) == _lib.OMB_EINVAL
