"""GPU: the fp32 screen behind the arg-max chain's bound.

omb_posterior_screen returns μ̃ (kernel transform of the fp64 r² in fp32, fp64 sum) and a margin ε; the two-phase path
("argmax_prune" 2) prunes with the interval [μ̃ − ε, μ̃ + ε] under "argmax_screen" 1 (default) and with fp64 means
under 0.  Held here: |μ̃ − μ| ≤ ε against omb_posterior's μ for every candidate; the pair under the screen equals the
dense chain's and the fp64-means path's bit for bit; the screen keeps at least what the fp64 bound keeps and still
prunes.

Shapes are those of test_gpu_argmax_prune (n_train 130, 300, 520 × n_var 2, 6: every ring and mean instantiation and
every part-filled tail; N = 1003 and 4099; offset 0 and non-zero; both entries), plus N = 7 and 17 for the screen alone.
Before each measured call the chain runs on other candidates in the same mode.  Every case ends in synchronize().
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import bench  # noqa: E402
from test_gpu_argmax_prune import N_MAX, SHAPES, _bits, _install, _problem, dev  # noqa: E402


@pytest.fixture(scope="module")
def ctx():
    from optimobo_amd.device import AcqContext
    c = AcqContext(0)
    yield c
    c.close()


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


def _three(ctx, call, stale, tag):
    """dense, fp64-means path and screened path: the same pair; (pair, stats of the fp64 path, stats of the screen)."""
    dense, st0 = _pair(ctx, 0, 1, call, stale)
    fp64, st64 = _pair(ctx, 2, 0, call, stale)
    got, st = _pair(ctx, 2, 1, call, stale)
    assert st0 == (False, 0, 0), (tag, st0)
    assert st64[0] and st[0] and st64[1] == st[1], (tag, st64, st)
    assert np.array_equal(_bits(dense), _bits(got)), (tag, dense, got, st)
    assert np.array_equal(_bits(dense), _bits(fp64)), (tag, dense, fp64, st64)
    assert st[2] >= st64[2], (tag, st64, st)
    return dense, st64, st


def _check_margin(ctx, X, tag):
    Xd = dev(X)
    mu, _ = ctx.posterior(Xd, n_obj=2)
    mt, eps = ctx.posterior_screen(Xd, n_obj=2)
    ctx.synchronize()
    mu, mt, eps = mu.cpu().numpy(), mt.cpu().numpy(), eps.cpu().numpy()
    assert mt.shape == eps.shape == (2, len(X))
    assert np.all(np.isfinite(eps)) and np.all(eps > 0), tag
    ratio = np.abs(mt - mu) / eps
    print(f"{tag}: max |mu~ - mu| / eps = {ratio.max():.4f}, max eps = {eps.max(1)}")
    assert np.all(np.abs(mt - mu) <= eps), (tag, ratio.max())


@pytest.mark.parametrize("n,d", SHAPES)
def test_screen_margin_covers_the_fp64_mean(ctx, n, d):
    p = _problem(n, d)
    _install(ctx, p)
    for N in (7, 17, 1003, N_MAX):
        X = p["Xc"][:N].copy()
        k = min(len(X[::5]), len(p["X"]))
        X[::5][:k] = p["X"][:k]                              # every fifth candidate a training point
        _check_margin(ctx, X, (n, d, N))


def test_screen_margin_rbf(ctx):
    from optimobo_amd.gp import GPState
    X, Y, ls, variances = bench.setup_problem(300, 6, tail_hi=0.3)
    for o in range(2):
        ctx.set_gp_state(o, GPState(X, Y[:, o], ls, variances[o], kernel="rbf"))
    Xc = bench.candidates(6, 0, 1003)
    Xc[:40] = X[:40]
    _check_margin(ctx, Xc, "rbf 300")


@pytest.mark.parametrize("n,d", SHAPES)
def test_pair_is_the_dense_pair_and_the_screen_prunes(ctx, n, d):
    p = _problem(n, d)
    _install(ctx, p)
    Xc = p["Xc"]
    for N in (1003, N_MAX):
        Xd, Xs = dev(Xc[:N]), dev(Xc[::-1][:N])
        seed = (N + 15) // 16
        for offset in (0, 123457):
            pair, st64, st = _three(ctx, lambda: ctx.eval_argmax(Xd, offset=offset), lambda: ctx.eval_argmax(Xs),
                                    (n, d, N, offset))
            assert pair[0] > 0 and offset <= pair[1] < offset + N
            print(f"n={n} d={d} N={N}: seed {st[1]}, survivors {st[2]} (screen) against {st64[2]} (fp64) of {N - seed}")
            assert st[1] == seed and st[2] < N - seed, (n, d, N, st)


@pytest.mark.parametrize("n,d", [(130, 2), (520, 6)])
def test_sobol_entry(ctx, n, d):
    p = _problem(n, d)
    _install(ctx, p)
    ctx.set_sobol(d, np.zeros(d), np.ones(d), scramble=False)
    for start, N in ((0, 1003), (5000, N_MAX)):
        pair, _, st = _three(ctx, lambda: ctx.eval_argmax_sobol(start, N), lambda: ctx.eval_argmax_sobol(start + 77, N),
                             (n, d, start, N))
        assert start <= pair[1] < start + N and st[1] == (N + 15) // 16
        X = dev(bench.candidates(d, start, N))
        other, _ = _pair(ctx, 2, 1, lambda: ctx.eval_argmax(X, offset=start), lambda: None)
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
    lo_seed, hi_seed = (best - 1) // 16 * 16, (best // 16 + 1) * 16
    lo_off, hi_off = lo_seed - 1, hi_seed + 1
    for lo, hi in ((lo_seed, hi_seed), (lo_off, hi_seed), (lo_seed, hi_off), (lo_off, hi_off), (33, N - 2)):
        X2 = Xc.copy()
        X2[lo] = Xc[best]
        X2[hi] = Xc[best]
        Xd, Xs = dev(X2), dev(Xc[::-1])
        pair, _, _ = _three(ctx, lambda: ctx.eval_argmax(Xd, offset=7), lambda: ctx.eval_argmax(Xs), (n, d, lo, hi))
        assert int(pair[1]) == lo + 7, (pair, lo, hi, best)


def test_nothing_is_pruned_when_no_value_is_positive(ctx):
    p = _problem(300, 6)
    for o, st in enumerate(p["states"]):
        ctx.set_gp_state(o, st)
    ctx.plan_ehvi2d(np.array([[-101.0, -101.0]]), np.array([-100.0, -100.0]), p["s00"], p["s01"], mode="reference")
    N = 1003
    Xd, Xs = dev(p["Xc"][:N]), dev(p["Xc"][::-1][:N])
    pair, st64, st = _three(ctx, lambda: ctx.eval_argmax(Xd, offset=11), lambda: ctx.eval_argmax(Xs), "tau = 0")
    assert pair[0] <= 0 and int(pair[1]) == 11
    assert st == (True, 63, N - 63) and st64 == st


@pytest.mark.parametrize("n,d", [(130, 6), (520, 6)])
def test_candidates_on_training_points(ctx, n, d):
    p = _problem(n, d)
    _install(ctx, p)
    N = 1003
    X2 = p["Xc"][:N].copy()
    for slot, row in ((0, 0), (5, 3), (32, 7), (33, 11), (1002, 17), (992, 19)):
        X2[slot] = p["X"][row]
    Xd, Xs = dev(X2), dev(p["Xc"][::-1][:N])
    _three(ctx, lambda: ctx.eval_argmax(Xd, offset=5), lambda: ctx.eval_argmax(Xs), (n, d, "training points"))
    Xd3 = dev(np.tile(p["X"][:59], (17, 1))[:N])                     # nothing but training points
    _three(ctx, lambda: ctx.eval_argmax(Xd3, offset=5), lambda: ctx.eval_argmax(Xs), (n, d, "only training points"))


def test_a_model_with_huge_weights_keeps_everything(ctx):
    """Σ|α| = 2·10⁸·n with μ unchanged: every training row twice, with weights α_k + B and −B, and L⁻¹ extended by
    zero rows (σ² unchanged).  ε is then about 10 units against a front inside [0, 5]²: the screen can drop nothing,
    the fp64 bound still prunes, and the pair is the dense one."""
    p = _problem(130, 6)
    B, n = 1e8, 130
    for o, st in enumerate(p["states"]):
        X2 = np.concatenate([st.X, st.X])
        a2 = np.concatenate([np.asarray(st.alpha).reshape(-1) + B, np.full(n, -B)])
        Linv2 = np.zeros((2 * n, 2 * n))
        Linv2[:n, :n] = st.Linv
        ctx.set_gp(o, X2, st.lengthscale, st.variance, a2, Linv2, st.kernel)
    ctx.plan_ehvi2d(p["stripes"], p["r"], p["s00"], p["s01"], mode="reference")
    N = 1003
    Xd, Xs = dev(p["Xc"][:N]), dev(p["Xc"][::-1][:N])
    _check_margin(ctx, p["Xc"][:N], "huge weights")
    pair, st64, st = _three(ctx, lambda: ctx.eval_argmax(Xd, offset=3), lambda: ctx.eval_argmax(Xs), "huge weights")
    assert st == (True, 63, N - 63) and st64[2] < N - 63, (st64, st)
    # the original models back for the tests that share the context's slots
    _install(ctx, p)
