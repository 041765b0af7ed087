"""GPU: the arg-max chain's staged order returns the dense chain's pair bit for bit.

"argmax_staged" 1 (default) runs the seeded-by-bound path ("argmax_prune" 1 or 3, "argmax_screen" 1) in two stages:
objective 1's screen and the bound ubm1 from it alone for every candidate, the seed and list A by ubm1, then objective
0's screen and the full interval bound for list A only, which leaves list B for the ring.  0 is §31's order.  Every pair
check is bitwise against the dense chain ("argmax_prune" 0).

Shapes: n_train 130, 300, 520 with n_var 2, 6, 6; N around every edge of the seed group and of the 16-candidate
column, a single candidate (seed only: both lists empty), 1003 and 4099.  Before each measured call the chain runs on
other candidates in the same mode, so a slot that the call failed to write would hold a stale number.  Every case ends
in synchronize(), which raises if a call marked the fault word.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import bench  # noqa: E402
from test_gpu_argmax_prune import N_MAX, _bits, _install, _problem, dev  # noqa: E402
from test_gpu_argmax_seed import G, SHAPES, SIZES, _seed  # noqa: E402


@pytest.fixture(scope="module")
def ctx():
    from optimobo_amd.device import AcqContext
    c = AcqContext(0)
    yield c
    c.close()


def _pair(ctx, prune, staged, call, stale):
    """The pair of call() under the two switches after stale() in the same mode, and the call's two stats."""
    ctx.debug_set("argmax_prune", prune)
    ctx.debug_set("argmax_staged", staged)
    try:
        stale()
        pair = call().cpu().numpy()
        ctx.synchronize()
        return pair, ctx.argmax_prune_stats(), ctx.argmax_stage_stats()
    finally:
        ctx.debug_set("argmax_prune", 1)
        ctx.debug_set("argmax_staged", 1)


def _three(ctx, call, stale, tag, N):
    """dense, staged 0 and staged 1 under "argmax_prune" 3: the same pair.  → (pair, §31's stats, staged stats)"""
    dense, st, sg = _pair(ctx, 0, 1, call, stale)
    assert st == (False, 0, 0) and sg == (False, 0, 0), (tag, st, sg)
    flat, st0, sg0 = _pair(ctx, 3, 0, call, stale)
    assert st0[0] and st0[1] == _seed(N) and sg0 == (False, 0, 0), (tag, st0, sg0)
    assert np.array_equal(_bits(dense), _bits(flat)), (tag, dense, flat, st0)
    got, st1, sg1 = _pair(ctx, 3, 1, call, stale)
    assert st1[0] and st1[1] == _seed(N), (tag, st1)
    assert sg1[0] and sg1[2] == st1[2], (tag, st1, sg1)
    assert sg1[1] <= N - _seed(N) and sg1[2] <= sg1[1], (tag, N, sg1)
    assert np.array_equal(_bits(dense), _bits(got)), (tag, dense, got, st1, sg1)
    return dense, st0, sg1


@pytest.mark.parametrize("n,d", SHAPES)
def test_pair_is_the_dense_pair_and_both_stages_prune(ctx, n, d):
    p = _problem(n, d)
    _install(ctx, p)
    Xc = p["Xc"]
    for N in SIZES:
        Xd, Xs = dev(Xc[:N]), dev(Xc[::-1][:N].copy())
        for offset in (0, 123457):
            pair, st0, sg = _three(ctx, lambda: ctx.eval_argmax(Xd, offset=offset), lambda: ctx.eval_argmax(Xs),
                                   (n, d, N, offset), N)
            print(f"n={n} d={d} N={N}: seed {_seed(N)}, |A| {sg[1]}, |B| {sg[2]}; unstaged survivors {st0[2]}")
            assert offset <= pair[1] < offset + N
            if N >= 1003 and pair[0] > 0:
                assert sg[2] + _seed(N) < N, (n, d, N, sg)
            if N == 1:
                assert sg == (True, 0, 0)


def test_the_default_takes_the_staged_order_from_65536_candidates(ctx):
    p = _problem(520, 6)
    _install(ctx, p)
    N = 1 << 16
    Xd = dev(bench.candidates(6, 0, N))
    dense, _, _ = _pair(ctx, 0, 1, lambda: ctx.eval_argmax(Xd, offset=3), lambda: None)
    flat, st0, _ = _pair(ctx, 1, 0, lambda: ctx.eval_argmax(Xd, offset=3), lambda: None)
    got = ctx.eval_argmax(Xd, offset=3).cpu().numpy()                          # the switches at their defaults
    ctx.synchronize()
    st, sg = ctx.argmax_prune_stats(), ctx.argmax_stage_stats()
    print(f"default at N = 2^16: {st} {sg}; staged 0: {st0}")
    assert st[0] and st[1] == _seed(N) and sg[0] and sg[2] == st[2], (st, sg)
    assert sg[2] <= sg[1] < N - _seed(N) and sg[2] + _seed(N) < N, sg
    assert np.array_equal(_bits(dense), _bits(got)) and np.array_equal(_bits(dense), _bits(flat))
    ctx.eval_argmax(dev(p["Xc"][:1003]))
    ctx.synchronize()
    assert ctx.argmax_prune_stats() == (False, 0, 0) and ctx.argmax_stage_stats() == (False, 0, 0)
    # the staged order needs the screen: without it the seed by bound runs §31's order
    ctx.debug_set("argmax_screen", 0)
    try:
        got0 = ctx.eval_argmax(Xd, offset=3).cpu().numpy()
        ctx.synchronize()
        assert ctx.argmax_prune_stats()[0] and ctx.argmax_stage_stats() == (False, 0, 0)
        assert np.array_equal(_bits(dense), _bits(got0))
    finally:
        ctx.debug_set("argmax_screen", 1)


@pytest.mark.parametrize("n,d", SHAPES)
def test_posterior_screen_list_has_the_dense_bits(ctx, n, d):
    p = _problem(n, d)
    _install(ctx, p)
    N = N_MAX
    Xd = dev(p["Xc"][:N])
    mu_d, eps_d = ctx.posterior_screen(Xd, n_obj=2)
    ctx.synchronize()
    mu_d, eps_d = mu_d.cpu().numpy(), eps_d.cpu().numpy()
    rng = np.random.default_rng(n + d)
    sentinel = -12345.678
    for obj in (0, 1):
        for size in (1, 15, 16, 17, 1003):
            idx = np.sort(rng.choice(N, size, replace=False)).astype(np.int32)
            if size == 17:
                idx[-1] = N - 1                                                # the batch's last slot
            if size == 1003:
                idx[0] = 0
            # the list's buffer is longer than its count: what lies past the count is never read as an index
            buf = np.full(size + 40, 2**31 - 1, np.int32)
            buf[:size] = idx
            idx_d = torch.as_tensor(buf, device="cuda:0")
            cnt_d = torch.as_tensor(np.array([size], np.int32), device="cuda:0")
            mu = torch.full((N,), sentinel, dtype=torch.float64, device="cuda:0")
            eps = torch.full((N,), sentinel, dtype=torch.float64, device="cuda:0")
            ctx.posterior_screen_list(Xd, idx_d, cnt_d, obj, mu, eps)
            ctx.synchronize()
            mu, eps = mu.cpu().numpy(), eps.cpu().numpy()
            listed = np.zeros(N, bool)
            listed[idx] = True
            assert np.array_equal(_bits(mu[listed]), _bits(mu_d[obj][listed])), (n, d, obj, size)
            assert np.array_equal(_bits(eps[listed]), _bits(eps_d[obj][listed])), (n, d, obj, size)
            assert np.all(mu[~listed] == sentinel) and np.all(eps[~listed] == sentinel), (n, d, obj, size)
        # a count of 0 writes nothing
        idx_d = torch.as_tensor(np.full(64, 2**31 - 1, np.int32), device="cuda:0")
        cnt_d = torch.zeros(1, dtype=torch.int32, device="cuda:0")
        mu = torch.full((N,), sentinel, dtype=torch.float64, device="cuda:0")
        eps = torch.full((N,), sentinel, dtype=torch.float64, device="cuda:0")
        ctx.posterior_screen_list(Xd, idx_d, cnt_d, obj, mu, eps)
        ctx.synchronize()
        assert bool((mu == sentinel).all()) and bool((eps == sentinel).all())


@pytest.mark.parametrize("n,d", [(130, 2), (520, 6)])
def test_sobol_entry(ctx, n, d):
    p = _problem(n, d)
    _install(ctx, p)
    ctx.set_sobol(d, np.zeros(d), np.ones(d), scramble=False)
    for start, N in ((0, 1003), (5000, N_MAX)):
        pair, _, _ = _three(ctx, lambda: ctx.eval_argmax_sobol(start, N), lambda: ctx.eval_argmax_sobol(start + 77, N),
                            (n, d, start, N), N)
        assert start <= pair[1] < start + N
        X = dev(bench.candidates(d, start, N))
        other, _, sg = _pair(ctx, 3, 1, lambda: ctx.eval_argmax(X, offset=start), lambda: None)
        assert sg[0] and np.array_equal(_bits(pair), _bits(other)), (n, d, start, N)


@pytest.mark.parametrize("n,d,N", [(300, 6, 1003), (520, 6, N_MAX)])
def test_lowest_index_wins_a_tie(ctx, n, d, N):
    """test_gpu_argmax_seed's placements: the arg-max candidate copied inside its own seed group, to the ends of
    another group and far away."""
    p = _problem(n, d)
    _install(ctx, p)
    Xc = p["Xc"][:N].copy()
    ctx.debug_set("argmax_prune", 0)
    best = int(ctx.eval_argmax(dev(Xc)).cpu().numpy()[1])
    g = best // G
    end = min((g + 1) * G, N)
    if best - g * G < 2 or end - best < 3:
        mid = g * G + (end - g * G) // 2
        Xc[[best, mid]] = Xc[[mid, best]]
        best = int(ctx.eval_argmax(dev(Xc)).cpu().numpy()[1])
        assert best == mid
    ctx.debug_set("argmax_prune", 1)
    places = [(g * G, best), (best, end - 1), (best - 1, best + 1)]
    groups = (N + G - 1) // G
    if groups > 1:
        og = 0 if g != 0 else 1
        places += [(og * G, min((og + 1) * G, N) - 1), (og * G, best), (min((og + 1) * G, N) - 1, best)]
    places.append((33, N - 2))
    for lo, hi in places:
        X2 = Xc.copy()
        X2[lo] = Xc[best]
        X2[hi] = Xc[best]
        Xd, Xs = dev(X2), dev(Xc[::-1])
        pair, _, _ = _three(ctx, lambda: ctx.eval_argmax(Xd, offset=7), lambda: ctx.eval_argmax(Xs), (n, d, lo, hi), N)
        assert int(pair[1]) == min(lo, hi, best) + 7, (pair, lo, hi, best)


@pytest.mark.parametrize("n,d", [(130, 6), (520, 6)])
def test_candidates_on_training_points(ctx, n, d):
    """σ²₀ ≈ 0 or slightly negative: on and off the groups' boundaries, a whole group, and a batch of nothing else."""
    p = _problem(n, d)
    _install(ctx, p)
    N = N_MAX
    Xs = dev(p["Xc"][::-1][:N])
    X2 = p["Xc"][:N].copy()
    for row, slot in enumerate((0, 5, G - 1, G, G + 1, 2 * G - 1, 2 * G, N - 1, N - 4)):
        X2[slot] = p["X"][2 * row]
    _three(ctx, lambda: ctx.eval_argmax(dev(X2), offset=5), lambda: ctx.eval_argmax(Xs), (n, d, "training points"), N)
    X3 = p["Xc"][:N].copy()
    X3[G:2 * G] = np.tile(p["X"], (G // n + 1, 1))[:G]
    _three(ctx, lambda: ctx.eval_argmax(dev(X3), offset=5), lambda: ctx.eval_argmax(Xs), (n, d, "a group of them"), N)
    X4 = np.tile(p["X"][:59], (N // 59 + 1, 1))[:N]
    _three(ctx, lambda: ctx.eval_argmax(dev(X4), offset=5), lambda: ctx.eval_argmax(Xs), (n, d, "only training points"),
           N)


def test_nothing_is_pruned_when_no_value_is_positive(ctx):
    """A front and reference point far below every posterior mean: every value is 0, τ₀ = 0, both stages keep every
    candidate past the seed and the lowest index wins."""
    p = _problem(300, 6)
    for o, st in enumerate(p["states"]):
        ctx.set_gp_state(o, st)
    ctx.plan_ehvi2d(np.array([[-101.0, -101.0]]), np.array([-100.0, -100.0]), p["s00"], p["s01"], mode="reference")
    for N in (1003, N_MAX):
        Xd, Xs = dev(p["Xc"][:N]), dev(p["Xc"][::-1][:N])
        pair, _, sg = _three(ctx, lambda: ctx.eval_argmax(Xd, offset=11), lambda: ctx.eval_argmax(Xs), "tau = 0", N)
        assert pair[0] <= 0 and int(pair[1]) == 11
        assert sg == (True, N - _seed(N), N - _seed(N)), (N, sg)


def test_swapped_objectives_keep_most_of_the_batch_in_list_a(ctx):
    """The states installed in the other order and the front's columns swapped: objective 1's mean decides little, list
    A keeps most of the batch, and the pair is still the dense one."""
    from optimobo_amd import pareto
    from oracle import pareto as opar
    p = _problem(520, 6)
    N = N_MAX
    Xd, Xs = dev(p["Xc"][:N]), dev(p["Xc"][::-1][:N])
    _install(ctx, p)
    _, _, sg_plain = _three(ctx, lambda: ctx.eval_argmax(Xd, offset=9), lambda: ctx.eval_argmax(Xs), "unswapped", N)
    for o, st in enumerate(p["states"][::-1]):
        ctx.set_gp_state(o, st)
    X, Y, _, _ = bench.setup_problem(520, 6, tail_hi=0.3)
    Ys = Y[:, ::-1]
    r = Ys.max(axis=0) + 0.1 * (Ys.max(axis=0) - Ys.min(axis=0))
    ctx.plan_ehvi2d(pareto.stripes_2d(opar.calc_pf(Ys)), r, p["s00"], p["s01"], mode="reference")
    pair, st0, sg = _three(ctx, lambda: ctx.eval_argmax(Xd, offset=9), lambda: ctx.eval_argmax(Xs), "swapped", N)
    print(f"swapped objectives, N={N}: |A| {sg[1]}, |B| {sg[2]}; unstaged survivors {st0[2]}; unswapped {sg_plain}")
    assert pair[0] > 0
    # objective 1 is now the one whose mean decides least: list A is several times the unswapped one
    assert sg[1] > 3 * sg_plain[1], (sg, sg_plain)
    _install(ctx, p)


@pytest.mark.parametrize("n", [130, 300, 520])
def test_ill_conditioned_models(ctx, n):
    """n_var 2: hundreds of training points in the unit square give weights whose margins ε are large."""
    p = _problem(n, 2)
    _install(ctx, p)
    for N in (1003, N_MAX):
        Xd, Xs = dev(p["Xc"][:N]), dev(p["Xc"][::-1][:N])
        _, eps = ctx.posterior_screen(Xd, n_obj=2)
        pair, _, sg = _three(ctx, lambda: ctx.eval_argmax(Xd, offset=2), lambda: ctx.eval_argmax(Xs), (n, 2, N), N)
        print(f"n={n} d=2 N={N}: max eps1 {float(eps[1].max()):.3g}, |A| {sg[1]}, |B| {sg[2]}")


def test_a_model_with_huge_weights_keeps_everything(ctx):
    """test_gpu_argmax_screen's model with Σ|α| = 2·10⁸·n: ε₁ and M₀ are huge, both stages keep every candidate."""
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
    _, _, sg = _three(ctx, lambda: ctx.eval_argmax(Xd, offset=3), lambda: ctx.eval_argmax(Xs), "huge weights", N)
    assert sg == (True, N - _seed(N), N - _seed(N)), sg
    _install(ctx, p)


@pytest.mark.parametrize("n,d", [(300, 6), (520, 6)])
def test_list_a_is_the_restated_bound_s_list(ctx, n, d):
    """|A| against tests/test_staged_bound.py's ubm1 on the device's own μ̃₁, ε₁ and values: the seeds by the smallest
    μ̃₁, τ₀ their best value, A what ubm1 keeps.  The device evaluates φ and Φ by its own approximations, so candidates
    whose restated ubm1 lies within 1e-6 of τ₀ may fall either way; every other one must agree."""
    from test_staged_bound import group_seeds, ubm1
    from oracle import acquisition as oacq
    p = _problem(n, d)
    _install(ctx, p)
    N = N_MAX
    Xd = dev(p["Xc"][:N])
    mt, eps = ctx.posterior_screen(Xd, n_obj=2)
    vals = ctx.eval(Xd)
    ctx.synchronize()
    mt, eps, vals = mt.cpu().numpy(), eps.cpu().numpy(), vals.cpu().numpy()
    _, _, sg = _pair(ctx, 3, 1, lambda: ctx.eval_argmax(Xd), lambda: None)
    st0 = p["states"][0]
    M0 = st0.variance * np.abs(np.asarray(st0.alpha)).sum() * (1.0 + 2.0 ** -20)
    u1 = ubm1(mt[1] - eps[1], p["stripes"], p["r"], p["s00"], p["s01"], st0.variance, M0)
    seeds = group_seeds(mt[1], G)
    tau, _ = oacq.argmax(vals[seeds])
    assert tau > 0
    rest = np.ones(N, bool)
    rest[seeds] = False
    sure = int(np.sum(rest & (u1 >= tau * (1 + 1e-6))))
    maybe = int(np.sum(rest & (np.abs(u1 - tau) < tau * 1e-6)))
    print(f"n={n} d={d}: |A| {sg[1]}, restated {sure} + at most {maybe}")
    assert sure <= sg[1] <= sure + maybe, (sg, sure, maybe)
