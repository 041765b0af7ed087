"""GPU: the arg-max chain's two-phase path returns the dense chain's pair bit for bit.

Under a reference-mode EHVI-2D plan with s01 > 0 the chain may evaluate the full posterior only for a seed sample
(every 16th candidate) and for the candidates whose upper bound — from the means alone — reaches the seed's best value.
Debug switch "argmax_prune" = 2 forces that path at any batch size, 0 the dense chain.

Shapes: n_train 130, 300, 520 (the three ring instantiations at n_var ≤ 8; 130 and 300 leave a part-filled last
chunk) × n_var 2 and 6, N = 1003 and 4099 (neither a multiple of 16 or 32; 4099 = 256·16 + 3 leaves a 3-candidate last
workgroup in the bound kernel, 1003 and 4099 a part-filled last ring workgroup in seed and survivor lists alike), offset
0 and a non-zero one, omb_eval_argmax and omb_eval_argmax_sobol.  Before each measured call the chain runs on other
candidates in the same mode, so a slot of the lists or of the compacted moments that the call failed to write would
hold a stale number.  Every case ends in synchronize(), which raises if a call marked the fault word.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import bench  # noqa: E402
from oracle import acquisition as oacq  # noqa: E402
from oracle import pareto as opar  # noqa: E402

N_MAX = 4099
SHAPES = [(n, d) for n in (130, 300, 520) for d in (2, 6)]


@pytest.fixture(scope="module")
def ctx():
    from optimobo_amd.device import AcqContext
    c = AcqContext(0)
    yield c
    c.close()


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device="cuda:0")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


_PROBLEMS = {}


def _problem(n, d):
    """The bench's mid-run training set at (n, d): x_2..x_d scaled by 0.3, ZDT1, its front, reference point and
    cache statistics; Sobol candidates.  Built once per shape."""
    if (n, d) not in _PROBLEMS:
        from optimobo_amd import pareto
        from optimobo_amd.gp import GPState
        X, Y, ls, variances = bench.setup_problem(n, d, tail_hi=0.3)
        states = [GPState(X, Y[:, o], ls, variances[o]) for o in range(2)]
        pf = opar.calc_pf(Y)
        r = Y.max(axis=0) + 0.1 * (Y.max(axis=0) - Y.min(axis=0))
        s00, s01 = oacq.cache_stats(pareto.cached_samples(2, 5, seed=1))
        assert s01 > 0
        _PROBLEMS[(n, d)] = dict(X=X, states=states, stripes=pareto.stripes_2d(pf), r=r, s00=s00, s01=s01,
                                 Xc=bench.candidates(d, 0, N_MAX))
    return _PROBLEMS[(n, d)]


def _install(ctx, p, s01=None):
    for o, st in enumerate(p["states"]):
        ctx.set_gp_state(o, st)
    ctx.plan_ehvi2d(p["stripes"], p["r"], p["s00"], p["s01"] if s01 is None else s01, mode="reference")


def _pair(ctx, mode, call, stale):
    """The pair of call() under "argmax_prune" = mode after stale() in the same mode, and the call's stats."""
    ctx.debug_set("argmax_prune", mode)
    try:
        stale()
        pair = call().cpu().numpy()
        ctx.synchronize()
        return pair, ctx.argmax_prune_stats()
    finally:
        ctx.debug_set("argmax_prune", 1)


def _both(ctx, call, stale, tag, two_phase=True):
    dense, st0 = _pair(ctx, 0, call, stale)
    got, st2 = _pair(ctx, 2, call, stale)
    assert st0 == (False, 0, 0), (tag, st0)
    assert st2[0] == two_phase, (tag, st2)
    assert np.array_equal(_bits(dense), _bits(got)), (tag, dense, got, st2)
    return dense, st2


@pytest.mark.parametrize("n,d", SHAPES)
def test_pair_is_the_dense_pair_and_the_path_prunes(ctx, n, d):
    p = _problem(n, d)
    _install(ctx, p)
    Xc = p["Xc"]
    for N in (1003, N_MAX):
        Xd, Xs = dev(Xc[:N]), dev(Xc[::-1][:N])
        seed = (N + 15) // 16
        for offset in (0, 123457):
            pair, st = _both(ctx, lambda: ctx.eval_argmax(Xd, offset=offset), lambda: ctx.eval_argmax(Xs), (n, d, N, offset))
            assert pair[0] > 0 and offset <= pair[1] < offset + N
            print(f"n={n} d={d} N={N}: seed {st[1]}, survivors {st[2]} of {N - seed}")
            # the path must actually prune; at n_var 6 some candidates past the seed also have to survive (the oracle
            # predicts 3 to 81 of them), at n_var 2 the maximum is Sobol point 0 — in the seed — and none may
            assert st[1] == seed and st[2] + seed < N, (n, d, N, st)
            assert st[2] > 0 or d == 2, (n, d, N, st)
    # the default leaves batches this small to the dense chain
    ctx.eval_argmax(dev(Xc[:1003]))
    assert ctx.argmax_prune_stats() == (False, 0, 0)


@pytest.mark.parametrize("n,d", [(130, 2), (520, 6)])
def test_sobol_entry(ctx, n, d):
    p = _problem(n, d)
    _install(ctx, p)
    ctx.set_sobol(d, np.zeros(d), np.ones(d), scramble=False)
    for start, N in ((0, 1003), (5000, N_MAX)):
        pair, st = _both(ctx, lambda: ctx.eval_argmax_sobol(start, N), lambda: ctx.eval_argmax_sobol(start + 77, N),
                         (n, d, start, N))
        assert start <= pair[1] < start + N and st[1] == (N + 15) // 16
        # the same points through the other entry
        X = dev(bench.candidates(d, start, N))
        other, _ = _pair(ctx, 2, lambda: ctx.eval_argmax(X, offset=start), lambda: None)
        assert np.array_equal(_bits(pair), _bits(other))


@pytest.mark.parametrize("n,d,N", [(300, 6, 1003), (520, 6, N_MAX)])
def test_lowest_index_wins_a_tie(ctx, n, d, N):
    """The arg-max candidate copied to a lower and to a higher index, on and off the seed sample's stride."""
    p = _problem(n, d)
    _install(ctx, p)
    Xc = p["Xc"][:N].copy()
    ctx.debug_set("argmax_prune", 0)
    best = int(ctx.eval_argmax(dev(Xc)).cpu().numpy()[1])
    ctx.debug_set("argmax_prune", 1)
    assert 40 < best < N - 40, best
    lo_seed, hi_seed = (best - 1) // 16 * 16, (best // 16 + 1) * 16           # evaluated with the seed sample
    lo_off, hi_off = lo_seed - 1, hi_seed + 1                                 # and only if their bound keeps them
    for lo, hi in ((lo_seed, hi_seed), (lo_off, hi_seed), (lo_seed, hi_off), (lo_off, hi_off), (33, N - 2)):
        X2 = Xc.copy()
        X2[lo] = Xc[best]
        X2[hi] = Xc[best]
        Xd, Xs = dev(X2), dev(Xc[::-1])
        pair, _ = _both(ctx, lambda: ctx.eval_argmax(Xd, offset=7), lambda: ctx.eval_argmax(Xs), (n, d, lo, hi))
        assert int(pair[1]) == lo + 7, (pair, lo, hi, best)


def test_plans_without_a_bound_take_the_dense_path(ctx):
    p = _problem(300, 6)
    N = 1003
    Xd, Xs = dev(p["Xc"][:N]), dev(p["Xc"][::-1][:N])
    _install(ctx, p, s01=-p["s01"])                                   # σB < 0: p2 is not monotone
    _both(ctx, lambda: ctx.eval_argmax(Xd, offset=3), lambda: ctx.eval_argmax(Xs), "s01 < 0", two_phase=False)
    _install(ctx, p)
    ctx.set_gp_state(2, p["states"][1])
    ctx.plan_constraints(1)                                           # a weight between EHVI and the arg-max
    _both(ctx, lambda: ctx.eval_argmax(Xd, offset=3), lambda: ctx.eval_argmax(Xs), "constraint", two_phase=False)
    ctx.plan_constraints(0)
    _both(ctx, lambda: ctx.eval_argmax(Xd, offset=3), lambda: ctx.eval_argmax(Xs), "cleared", two_phase=True)
    ctx.plan_ehvi2d(p["stripes"], p["r"], p["s00"], p["s01"], mode="textbook")
    _both(ctx, lambda: ctx.eval_argmax(Xd, offset=3), lambda: ctx.eval_argmax(Xs), "textbook", two_phase=False)


def test_nothing_is_pruned_when_no_value_is_positive(ctx):
    """A front and reference point far below every posterior mean: every value is 0, τ = 0, every candidate past the
    seed survives and the lowest index wins."""
    p = _problem(300, 6)
    for o, st in enumerate(p["states"]):
        ctx.set_gp_state(o, st)
    ctx.plan_ehvi2d(np.array([[-101.0, -101.0]]), np.array([-100.0, -100.0]), p["s00"], p["s01"], mode="reference")
    N = 1003
    Xd, Xs = dev(p["Xc"][:N]), dev(p["Xc"][::-1][:N])
    pair, st = _both(ctx, lambda: ctx.eval_argmax(Xd, offset=11), lambda: ctx.eval_argmax(Xs), "tau = 0")
    assert pair[0] <= 0 and int(pair[1]) == 11
    assert st == (True, 63, N - 63)


@pytest.mark.parametrize("n,d", [(130, 6), (520, 6)])
def test_candidates_on_training_points(ctx, n, d):
    """σ²₀ ≈ 0, or slightly negative (the value is then NaN and never wins), on and off the seed's stride."""
    p = _problem(n, d)
    _install(ctx, p)
    N = 1003
    X2 = p["Xc"][:N].copy()
    for slot, row in ((0, 0), (5, 3), (32, 7), (33, 11), (1002, 17), (992, 19)):
        X2[slot] = p["X"][row]
    Xd, Xs = dev(X2), dev(p["Xc"][::-1][:N])
    _both(ctx, lambda: ctx.eval_argmax(Xd, offset=5), lambda: ctx.eval_argmax(Xs), (n, d, "training points"))
    X3 = np.tile(p["X"][:59], (17, 1))[:N]                           # nothing but training points
    Xd3 = dev(X3)
    _both(ctx, lambda: ctx.eval_argmax(Xd3, offset=5), lambda: ctx.eval_argmax(Xs), (n, d, "only training points"))
