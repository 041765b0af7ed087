"""GPU: the staged order's first list drawn by one cut on μ̃₁ − ε₁ returns the dense chain's pair bit for bit.

"argmax_cut" 1 (default) replaces objective 1's bound per candidate by: the seeds by the smallest μ̃₁ alone, one
workgroup solving ubm1(m*) = τ₀ once the seeds' τ₀ is known, and a threshold that keeps a candidate unless its low end
μ̃₁ − ε₁ is at least m*.  0 is §33's path, the A/B partner.  Every pair check is bitwise against the dense chain
("argmax_prune" 0); the lists may differ only for candidates whose bound lies within 1e-6·τ₀ of τ₀.

Shapes, sizes and helpers are tests/test_gpu_argmax_seed.py's and tests/test_gpu_argmax_prune.py's: every edge of the
group size up to N_MAX on the models (130, 2), (300, 6), (520, 6).  Before each measured call the chain runs on other
candidates in the same mode, so a slot that the call failed to write would hold a stale number.  Every case ends in
synchronize(), which raises if a call marked the fault word.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import bench  # noqa: E402
from test_cut_bound import ubm1_at  # noqa: E402
from test_gpu_argmax_prune import N_MAX, _bits, _install, _problem, dev  # noqa: E402
from test_gpu_argmax_seed import G, SHAPES, SIZES, _seed  # noqa: E402
from test_staged_bound import group_seeds, stripe_consts, ubm1  # noqa: E402


@pytest.fixture(scope="module")
def ctx():
    from optimobo_amd.device import AcqContext
    c = AcqContext(0)
    yield c
    c.close()


def _pair(ctx, prune, cut, call, stale):
    """The pair of call() under the two switches after stale() in the same mode, and the call's stats."""
    ctx.debug_set("argmax_prune", prune)
    ctx.debug_set("argmax_cut", cut)
    try:
        stale()
        pair = call().cpu().numpy()
        ctx.synchronize()
        return pair, ctx.argmax_prune_stats(), ctx.argmax_stage_stats(), ctx.argmax_cut_stats()
    finally:
        ctx.debug_set("argmax_prune", 1)
        ctx.debug_set("argmax_cut", 1)


def _check_cut(cs, tag):
    """The stats entry: ubm1(m*) < τ₀ and within 1e-7 of it (a neighbouring double cannot be probed from here: the
    resolution's other branch is the CPU test's), or no cut at all."""
    taken, ms, tau, u = cs
    assert taken, (tag, cs)
    if np.isfinite(ms):
        assert tau > 0 and u < tau and u >= tau * (1.0 - 1e-7), (tag, cs)
    else:
        assert ms == np.inf and np.isnan(u), (tag, cs)


def _three(ctx, call, stale, tag, N):
    """dense, "argmax_cut" 0 and 1 under "argmax_prune" 3: the same pair.  → (pair, cut 0's stage stats, cut 1's, cut
    1's cut stats)"""
    dense, st, sg, cs = _pair(ctx, 0, 1, call, stale)
    assert st == (False, 0, 0) and sg == (False, 0, 0) and cs == (False, 0.0, 0.0, 0.0), (tag, st, sg, cs)
    per, st0, sg0, cs0 = _pair(ctx, 3, 0, call, stale)
    assert st0[0] and st0[1] == _seed(N) and sg0[0] and cs0 == (False, 0.0, 0.0, 0.0), (tag, st0, sg0, cs0)
    assert np.array_equal(_bits(dense), _bits(per)), (tag, dense, per, st0)
    got, st1, sg1, cs1 = _pair(ctx, 3, 1, call, stale)
    assert st1[0] and st1[1] == _seed(N) and sg1[0] and sg1[2] == st1[2], (tag, st1, sg1)
    assert sg1[1] <= N - _seed(N) and sg1[2] <= sg1[1], (tag, N, sg1)
    _check_cut(cs1, tag)
    assert np.array_equal(_bits(dense), _bits(got)), (tag, dense, got, st1, sg1, cs1)
    return dense, sg0, sg1, cs1


def _restated(ctx, p, Xd, N):
    """From the device's own μ̃₁, ε₁ and values: the restated ubm1 per candidate, τ₀ of the seeds by the smallest μ̃₁,
    the candidates past the seed and the stripe constants."""
    from oracle import acquisition as oacq
    mt, eps = ctx.posterior_screen(Xd, n_obj=2)
    vals = ctx.eval(Xd)
    ctx.synchronize()
    mt, eps, vals = mt.cpu().numpy(), eps.cpu().numpy(), vals.cpu().numpy()
    st0 = p["states"][0]
    M0 = st0.variance * np.abs(np.asarray(st0.alpha)).sum() * (1.0 + 2.0 ** -20)
    args = (p["stripes"], p["r"], p["s00"], p["s01"], st0.variance, M0)
    u1 = ubm1(mt[1] - eps[1], *args)
    seeds = group_seeds(mt[1], G)
    tau, _ = oacq.argmax(vals[seeds])
    rest = np.ones(N, bool)
    rest[seeds] = False
    return u1, tau, rest, stripe_consts(*args), st0.variance * p["s01"]


@pytest.mark.parametrize("n,d", SHAPES)
def test_pair_is_the_dense_pair_at_every_edge_of_the_group(ctx, n, d):
    p = _problem(n, d)
    _install(ctx, p)
    Xc = p["Xc"]
    for N in SIZES:
        Xd, Xs = dev(Xc[:N]), dev(Xc[::-1][:N].copy())
        u1, tau, rest, _, _ = _restated(ctx, p, Xd, N)
        window = int(np.sum(rest & (np.abs(u1 - tau) < 1e-6 * tau))) if tau > 0 else 0
        for offset in (0, 123457):
            pair, sg0, sg1, cs = _three(ctx, lambda: ctx.eval_argmax(Xd, offset=offset), lambda: ctx.eval_argmax(Xs),
                                        (n, d, N, offset), N)
            print(f"n={n} d={d} N={N}: |A| {sg1[1]} by cut, {sg0[1]} per candidate, {window} in the window; |B| "
                  f"{sg1[2]}, {sg0[2]}; m* {cs[1]:.9g}")
            assert offset <= pair[1] < offset + N
            assert abs(sg1[1] - sg0[1]) <= window, (n, d, N, sg0, sg1, window)
            if N == 1:
                assert sg1 == (True, 0, 0)


@pytest.mark.parametrize("n,d", [(300, 6), (520, 6)])
def test_stats_and_list_against_the_restated_bound(ctx, n, d):
    """τ₀ and ubm1(m*) of the stats entry against numpy on the device's own μ̃₁, ε₁ and values, and |A| against the
    restated per-candidate list but for the 1e-6 window (tests/test_gpu_argmax_staged.py's rule)."""
    p = _problem(n, d)
    _install(ctx, p)
    N = N_MAX
    Xd = dev(p["Xc"][:N])
    u1, tau, rest, consts, sB = _restated(ctx, p, Xd, N)
    _, _, sg, cs = _pair(ctx, 3, 1, lambda: ctx.eval_argmax(Xd), lambda: None)
    _check_cut(cs, (n, d))
    assert tau > 0 and cs[2] == tau, (cs, tau)
    u_np = ubm1_at(cs[1], *consts, sB)[0]
    print(f"n={n} d={d}: m* {cs[1]:.12g}, device ubm1(m*) {cs[3]:.12g}, numpy {u_np:.12g}, tau0 {tau:.12g}")
    assert abs(u_np - cs[3]) <= 1e-9 * cs[3], (u_np, cs)
    sure = int(np.sum(rest & (u1 >= tau * (1 + 1e-6))))
    maybe = int(np.sum(rest & (np.abs(u1 - tau) < tau * 1e-6)))
    assert sure <= sg[1] <= sure + maybe, (sg, sure, maybe)


def test_the_default_takes_the_cut_from_65536_candidates(ctx):
    p = _problem(520, 6)
    _install(ctx, p)
    N = 1 << 16
    Xd = dev(bench.candidates(6, 0, N))
    dense, _, _, _ = _pair(ctx, 0, 1, lambda: ctx.eval_argmax(Xd, offset=3), lambda: None)
    per, _, sg0, _ = _pair(ctx, 1, 0, lambda: ctx.eval_argmax(Xd, offset=3), lambda: None)
    got = ctx.eval_argmax(Xd, offset=3).cpu().numpy()                          # the switches at their defaults
    ctx.synchronize()
    sg, cs = ctx.argmax_stage_stats(), ctx.argmax_cut_stats()
    print(f"default at N = 2^16: {sg} {cs}; cut 0: {sg0}")
    _check_cut(cs, "default")
    assert np.isfinite(cs[1]) and sg[0] and sg[1] < N - _seed(N)
    assert np.array_equal(_bits(dense), _bits(got)) and np.array_equal(_bits(dense), _bits(per))
    # without the staged order there is no cut
    ctx.debug_set("argmax_staged", 0)
    try:
        got0 = ctx.eval_argmax(Xd, offset=3).cpu().numpy()
        ctx.synchronize()
        assert ctx.argmax_prune_stats()[0] and ctx.argmax_cut_stats() == (False, 0.0, 0.0, 0.0)
        assert np.array_equal(_bits(dense), _bits(got0))
    finally:
        ctx.debug_set("argmax_staged", 1)


def test_nothing_is_cut_when_no_value_is_positive(ctx):
    """A front and reference point far below every posterior mean: τ₀ = 0, m* = +∞, list A is everything past the
    seeds."""
    p = _problem(300, 6)
    for o, st in enumerate(p["states"]):
        ctx.set_gp_state(o, st)
    ctx.plan_ehvi2d(np.array([[-101.0, -101.0]]), np.array([-100.0, -100.0]), p["s00"], p["s01"], mode="reference")
    for N in (1003, N_MAX):
        Xd, Xs = dev(p["Xc"][:N]), dev(p["Xc"][::-1][:N])
        pair, _, sg, cs = _three(ctx, lambda: ctx.eval_argmax(Xd, offset=11), lambda: ctx.eval_argmax(Xs), "tau = 0", N)
        assert pair[0] <= 0 and int(pair[1]) == 11
        assert cs[1] == np.inf and not cs[2] > 0, cs
        assert sg == (True, N - _seed(N), N - _seed(N)), (N, sg)
    _install(ctx, p)


def test_a_model_with_huge_weights_keeps_everything(ctx):
    """Σ|α| = 2·10⁸·n: ε₁ is huge, every low end lies far left of the cut and both stages keep every candidate."""
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
    _, _, sg, _ = _three(ctx, lambda: ctx.eval_argmax(Xd, offset=3), lambda: ctx.eval_argmax(Xs), "huge weights", N)
    assert sg == (True, N - _seed(N), N - _seed(N)), sg
    _install(ctx, p)


@pytest.mark.parametrize("n", [130, 300, 520])
def test_ill_conditioned_models(ctx, n):
    """n_var 2: hundreds of training points in the unit square give weights whose margins ε are large."""
    p = _problem(n, 2)
    _install(ctx, p)
    for N in (1003, N_MAX):
        Xd, Xs = dev(p["Xc"][:N]), dev(p["Xc"][::-1][:N])
        _, sg0, sg1, cs = _three(ctx, lambda: ctx.eval_argmax(Xd, offset=2), lambda: ctx.eval_argmax(Xs), (n, 2, N), N)
        print(f"n={n} d=2 N={N}: |A| {sg1[1]} ({sg0[1]}), |B| {sg1[2]} ({sg0[2]}), m* {cs[1]:.6g}")


@pytest.mark.parametrize("n,d,N", [(300, 6, 1003), (520, 6, N_MAX)])
def test_lowest_index_wins_a_tie(ctx, n, d, N):
    """The arg-max candidate copied inside its own seed group, to the ends of another group and far away."""
    p = _problem(n, d)
    _install(ctx, p)
    Xc = p["Xc"][:N].copy()
    ctx.debug_set("argmax_prune", 0)
    best = int(ctx.eval_argmax(dev(Xc)).cpu().numpy()[1])
    ctx.debug_set("argmax_prune", 1)
    g = best // G
    end = min((g + 1) * G, N)
    places = [(g * G, end - 1), (max(best - 1, 0), min(best + 1, N - 1)), (33, N - 2)]
    if (N + G - 1) // G > 1:
        og = 0 if g != 0 else 1
        places += [(og * G, min((og + 1) * G, N) - 1), (og * G, best)]
    for lo, hi in places:
        X2 = Xc.copy()
        X2[lo] = Xc[best]
        X2[hi] = Xc[best]
        Xd, Xs = dev(X2), dev(Xc[::-1])
        pair, _, _, _ = _three(ctx, lambda: ctx.eval_argmax(Xd, offset=7), lambda: ctx.eval_argmax(Xs), (n, d, lo, hi),
                               N)
        assert int(pair[1]) == min(lo, hi, best) + 7, (pair, lo, hi, best)


@pytest.mark.parametrize("n,d", [(130, 2), (520, 6)])
def test_sobol_entry(ctx, n, d):
    p = _problem(n, d)
    _install(ctx, p)
    ctx.set_sobol(d, np.zeros(d), np.ones(d), scramble=False)
    for start, N in ((0, 1003), (5000, N_MAX)):
        pair, _, _, _ = _three(ctx, lambda: ctx.eval_argmax_sobol(start, N),
                               lambda: ctx.eval_argmax_sobol(start + 77, N), (n, d, start, N), N)
        assert start <= pair[1] < start + N
        X = dev(bench.candidates(d, start, N))
        other, _, _, cs = _pair(ctx, 3, 1, lambda: ctx.eval_argmax(X, offset=start), lambda: None)
        assert cs[0] and np.array_equal(_bits(pair), _bits(other)), (n, d, start, N)


def test_swapped_objectives(ctx):
    """The states installed in the other order and the front's columns swapped: list A keeps most of the batch under
    either form of the bound, and the pair is still the dense one."""
    from optimobo_amd import pareto
    from oracle import pareto as opar
    p = _problem(520, 6)
    N = N_MAX
    Xd, Xs = dev(p["Xc"][:N]), dev(p["Xc"][::-1][:N])
    for o, st in enumerate(p["states"][::-1]):
        ctx.set_gp_state(o, st)
    X, Y, _, _ = bench.setup_problem(520, 6, tail_hi=0.3)
    Ys = Y[:, ::-1]
    r = Ys.max(axis=0) + 0.1 * (Ys.max(axis=0) - Ys.min(axis=0))
    ctx.plan_ehvi2d(pareto.stripes_2d(opar.calc_pf(Ys)), r, p["s00"], p["s01"], mode="reference")
    pair, sg0, sg1, cs = _three(ctx, lambda: ctx.eval_argmax(Xd, offset=9), lambda: ctx.eval_argmax(Xs), "swapped", N)
    print(f"swapped objectives, N={N}: |A| {sg1[1]} ({sg0[1]}), |B| {sg1[2]} ({sg0[2]}), m* {cs[1]:.9g}")
    assert pair[0] > 0 and np.isfinite(cs[1]) and sg1[1] > N // 2 and sg0[1] > N // 2
    _install(ctx, p)
