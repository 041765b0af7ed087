"""GPU: the arg-max chain seeded by the bound returns the dense chain's pair bit for bit.

"argmax_prune" 3 forces the ordering means → bound of every candidate → seed = each group's best bound → τ →
threshold → survivors at any batch size; 2 is the strided seed of §29 / §30, 0 the dense chain, 1 (default) the seed by
bound from 2^16 candidates on.  "argmax_screen" 0 / 1 feeds the bound fp64 means or the fp32 screen under both.

Shapes: n_train 130, 300, 520 (the three ring instantiations at n_var ≤ 8) with n_var 2, 6, 6; N around every edge of
the seed group (255, 256, 257, 1023, 1024, 1025 cover both admissible group sizes), a single candidate, a single part
group, 1003 and 4099 (part-filled last workgroups in every kernel).  Before each measured call the chain runs on other
candidates in the same mode, so a slot that the call failed to write would hold a stale number.  Every case ends in
synchronize(), which raises if a call marked the fault word.
"""
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import bench  # noqa: E402
from test_gpu_argmax_prune import N_MAX, _bits, _install, _problem, dev  # noqa: E402

SHAPES = [(130, 2), (300, 6), (520, 6)]
SIZES = (1, 7, 255, 256, 257, 1003, 1023, 1024, 1025, N_MAX)
_HDR = os.path.join(os.path.dirname(__file__), "..", "optimobo_amd", "csrc", "omb_internal.h")
G = int(re.search(r"constexpr int kPruneSeedGroup = (\d+);", open(_HDR).read()).group(1))


@pytest.fixture(scope="module")
def ctx():
    from optimobo_amd.device import AcqContext
    c = AcqContext(0)
    yield c
    c.close()


def _seed(N):
    return (N + G - 1) // G


def _pair(ctx, prune, screen, call, stale):
    """The pair of call() under the two switches after stale() in the same mode, and the call's stats."""
    ctx.debug_set("argmax_prune", prune)
    ctx.debug_set("argmax_screen", screen)
    try:
        stale()
        pair = call().cpu().numpy()
        ctx.synchronize()
        return pair, ctx.argmax_prune_stats()
    finally:
        ctx.debug_set("argmax_prune", 1)
        ctx.debug_set("argmax_screen", 1)


def _all(ctx, call, stale, tag):
    """dense, strided seed and seed by bound, the latter two on fp64 means and on the screen: the same pair.
    → (pair, {(prune, screen): stats})."""
    dense, st0 = _pair(ctx, 0, 1, call, stale)
    assert st0 == (False, 0, 0), (tag, st0)
    stats = {}
    for prune in (2, 3):
        for screen in (0, 1):
            got, st = _pair(ctx, prune, screen, call, stale)
            assert st[0], (tag, prune, screen, st)
            assert np.array_equal(_bits(dense), _bits(got)), (tag, prune, screen, dense, got, st)
            stats[(prune, screen)] = st
    return dense, stats


@pytest.mark.parametrize("n,d", SHAPES)
def test_pair_is_the_dense_pair_and_the_seed_prunes(ctx, n, d):
    p = _problem(n, d)
    _install(ctx, p)
    Xc = p["Xc"]
    for N in SIZES:
        Xd, Xs = dev(Xc[:N]), dev(Xc[::-1][:N].copy())            # (a one-row reversed view counts as contiguous)
        for offset in (0, 123457):
            pair, stats = _all(ctx, lambda: ctx.eval_argmax(Xd, offset=offset), lambda: ctx.eval_argmax(Xs),
                               (n, d, N, offset))
            assert offset <= pair[1] < offset + N and (pair[0] > 0 or N < 1003)
            for screen in (0, 1):
                st2, st3 = stats[(2, screen)], stats[(3, screen)]
                print(f"n={n} d={d} N={N} screen={screen}: by bound {st3[1]} + {st3[2]}, strided {st2[1]} + {st2[2]}")
                assert st2[1] == (N + 15) // 16, (n, d, N, screen, st2)
                assert st3[1] == _seed(N), (n, d, N, screen, st3)
                # a single candidate is its own seed: nothing is left to prune
                assert st3[2] < N - st3[1] or N == 1 and st3[2] == 0, (n, d, N, screen, st3)
                if (n, d, N) == (520, 6, N_MAX):
                    assert st3[1] + st3[2] < st2[1] + st2[2], (screen, st2, st3)


@pytest.mark.parametrize("n,d", [(130, 2), (520, 6)])
def test_sobol_entry(ctx, n, d):
    p = _problem(n, d)
    _install(ctx, p)
    ctx.set_sobol(d, np.zeros(d), np.ones(d), scramble=False)
    for start, N in ((0, 1003), (5000, N_MAX)):
        pair, stats = _all(ctx, lambda: ctx.eval_argmax_sobol(start, N), lambda: ctx.eval_argmax_sobol(start + 77, N),
                           (n, d, start, N))
        assert start <= pair[1] < start + N and stats[(3, 1)][1] == _seed(N)
        # the same points through the other entry
        X = dev(bench.candidates(d, start, N))
        for screen in (0, 1):
            other, _ = _pair(ctx, 3, screen, lambda: ctx.eval_argmax(X, offset=start), lambda: None)
            assert np.array_equal(_bits(pair), _bits(other)), (n, d, start, N, screen)


@pytest.mark.parametrize("n,d,N", [(300, 6, 1003), (520, 6, N_MAX)])
def test_lowest_index_wins_a_tie(ctx, n, d, N):
    """The arg-max candidate copied inside its own seed group, to the ends of another group and far away."""
    p = _problem(n, d)
    _install(ctx, p)
    Xc = p["Xc"][:N].copy()
    ctx.debug_set("argmax_prune", 0)
    best = int(ctx.eval_argmax(dev(Xc)).cpu().numpy()[1])
    g = best // G
    end = min((g + 1) * G, N)                        # one past the group's last candidate
    if best - g * G < 2 or end - best < 3:           # keep room on either side of it inside the group
        mid = g * G + (end - g * G) // 2
        Xc[[best, mid]] = Xc[[mid, best]]
        best = int(ctx.eval_argmax(dev(Xc)).cpu().numpy()[1])
        assert best == mid
    ctx.debug_set("argmax_prune", 1)
    places = [(g * G, best), (best, end - 1), (best - 1, best + 1)]            # inside its own group
    groups = (N + G - 1) // G
    assert groups > 1 or N < N_MAX
    if groups > 1:
        og = 0 if g != 0 else 1                                                # another group's first and last slot
        places += [(og * G, min((og + 1) * G, N) - 1), (og * G, best), (min((og + 1) * G, N) - 1, best)]
    places.append((33, N - 2))
    for lo, hi in places:
        X2 = Xc.copy()
        X2[lo] = Xc[best]
        X2[hi] = Xc[best]
        Xd, Xs = dev(X2), dev(Xc[::-1])
        pair, _ = _all(ctx, lambda: ctx.eval_argmax(Xd, offset=7), lambda: ctx.eval_argmax(Xs), (n, d, lo, hi))
        assert int(pair[1]) == min(lo, hi, best) + 7, (pair, lo, hi, best)


@pytest.mark.parametrize("n,d", [(130, 6), (520, 6)])
def test_candidates_on_training_points(ctx, n, d):
    """σ²₀ ≈ 0, or slightly negative (the value is then NaN and never wins): on and off the seed groups' boundaries, a
    whole group of them, and a batch of nothing else."""
    p = _problem(n, d)
    _install(ctx, p)
    N = N_MAX
    Xs = dev(p["Xc"][::-1][:N])
    X2 = p["Xc"][:N].copy()
    for row, slot in enumerate((0, 5, G - 1, G, G + 1, 2 * G - 1, 2 * G, N - 1, N - 4)):
        X2[slot] = p["X"][2 * row]
    _all(ctx, lambda: ctx.eval_argmax(dev(X2), offset=5), lambda: ctx.eval_argmax(Xs), (n, d, "training points"))
    X3 = p["Xc"][:N].copy()
    X3[G:2 * G] = np.tile(p["X"], (G // n + 1, 1))[:G]                         # group 1: training points alone
    _all(ctx, lambda: ctx.eval_argmax(dev(X3), offset=5), lambda: ctx.eval_argmax(Xs), (n, d, "a group of them"))
    X4 = np.tile(p["X"][:59], (N // 59 + 1, 1))[:N]                            # nothing but training points
    _all(ctx, lambda: ctx.eval_argmax(dev(X4), offset=5), lambda: ctx.eval_argmax(Xs), (n, d, "only training points"))


def test_nothing_is_pruned_when_no_value_is_positive(ctx):
    """A front and reference point far below every posterior mean: every value is 0, τ = 0, every candidate past the
    seed survives and the lowest index wins."""
    p = _problem(300, 6)
    for o, st in enumerate(p["states"]):
        ctx.set_gp_state(o, st)
    ctx.plan_ehvi2d(np.array([[-101.0, -101.0]]), np.array([-100.0, -100.0]), p["s00"], p["s01"], mode="reference")
    for N in (1003, N_MAX):
        Xd, Xs = dev(p["Xc"][:N]), dev(p["Xc"][::-1][:N])
        pair, stats = _all(ctx, lambda: ctx.eval_argmax(Xd, offset=11), lambda: ctx.eval_argmax(Xs), "tau = 0")
        assert pair[0] <= 0 and int(pair[1]) == 11
        for screen in (0, 1):
            assert stats[(3, screen)] == (True, _seed(N), N - _seed(N)), (N, screen, stats)


def test_the_default_seeds_by_the_bound_from_65536_candidates(ctx):
    p = _problem(520, 6)
    _install(ctx, p)
    N = 1 << 16
    Xd = dev(bench.candidates(6, 0, N))
    dense, _ = _pair(ctx, 0, 1, lambda: ctx.eval_argmax(Xd, offset=3), lambda: None)
    got = ctx.eval_argmax(Xd, offset=3).cpu().numpy()                          # the switches at their defaults
    ctx.synchronize()
    st = ctx.argmax_prune_stats()
    print(f"default at N = 2^16: {st}")
    assert st[0] and st[1] == _seed(N) and st[2] < N - st[1], st
    assert np.array_equal(_bits(dense), _bits(got))
    ctx.eval_argmax(dev(p["Xc"][:1003]))
    ctx.synchronize()
    assert ctx.argmax_prune_stats() == (False, 0, 0)
