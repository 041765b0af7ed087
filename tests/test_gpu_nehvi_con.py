"""GPU: constraints through sample paths above the kernel — the fused chain under ``plan_hvi_paths_con``,
its coherence with the installed state, ``sample_fronts(n_con=…)``, the estimator against exact EHVI × probability of
feasibility, constrained Thompson batches and the drivers' ``constraints="paths"``.  Small problems throughout:
n ≤ 40, d ≤ 3, 64 features."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _constraints_fixture as cf  # noqa: E402
import _nehvi_reference as R  # noqa: E402

from optimobo_amd import pareto  # noqa: E402
from optimobo_amd._lib import HVI_PATHS_CHUNK, OMB_ESTATE, OMB_EUNSUP, OMBError  # noqa: E402

M = 64      # random Fourier features


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device="cuda:0")


def host(t):
    return t.cpu().numpy()


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _models(k, c, n=30, d=2, seed=3, shift=0.0):
    """k objective states and c constraint states (g_j = Σx − 0.9 − 0.1j + shift: both signs over the box at
    shift = 0) on shared inputs."""
    from optimobo_amd.gp import GPState
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 1.0, (n, d))
    Y = np.stack([np.sin(3 * X[:, 0] + 1.3 * o) + np.cos(2 * X[:, 1] - o) + (X[:, 0] if o % 2 else -X[:, 0])
                  for o in range(k)] + [X.sum(1) - 0.9 - 0.1 * j + shift for j in range(c)], 1)
    return [GPState(X, Y[:, o], rng.uniform(0.4, 0.9, d), float(np.var(Y[:, o])) + 0.5, kernel="matern52", noise=1e-3)
            for o in range(k + c)], X, Y


def _engine(k, c, **kw):
    from optimobo_amd.acquisition import AcquisitionEngine
    models, X, Y = _models(k, c, **kw)
    d = X.shape[1]
    return AcquisitionEngine(0).load_models(models), models, X, Y, np.zeros(d), np.ones(d)


# ------------------------------------------------------------------------------------------- 1. sample_fronts
@pytest.mark.parametrize("k", [1, 2])
def test_sample_fronts_are_feasible_fronts_of_the_path_values(k):
    eng, models, X, Y, lower, upper = _engine(k, 1)
    try:
        r = None if k == 1 else Y[:, :k].max(0) + 0.2
        for bad in (-1, k + 1):
            with pytest.raises(ValueError, match="n_con"):
                eng.sample_fronts(4, r, lower, upper, n_con=bad)
        S = 6
        fronts = eng.sample_fronts(S, r, lower, upper, seed=9, n_features=M, n_con=1)
        F = host(eng.path_values(X))                                   # (k + 1, S, n)
        feas = F[k] <= 0
        assert 0 < feas.sum() < feas.size and len(set(feas.sum(1))) > 1          # the paths disagree on the rows
        want, decomps = pareto.feasible_fronts(F[:k], F[k:], r)
        assert all(same(a, b) for a, b in zip(fronts, want))
        for got, w in zip(eng._front_lists, pareto.pack_box_lists(decomps)):
            assert same(got, w) and got.dtype == w.dtype
        Xd = dev(np.random.default_rng(1).uniform(0, 1, (1025, X.shape[1])))
        y = eng.path_values(Xd)
        for eta in (0.0, 0.05):
            v = host(eng.nehvi(Xd, eta=eta))
            assert same(v, host(eng.ctx.hvi_paths_con(y, 1, *eng._front_lists, eta=eta)))
            assert np.all(v >= 0.0) and np.any(v > 0.0)
            eng.plan_nehvi(eta=eta)
            assert eng.ctx.plan_kind[0] == "omb_plan_hvi_paths_con" and not eng.has_gradient()
            assert same(host(eng.ctx.eval(Xd)), v)
        # candidates infeasible under every path score exactly 0
        dead = np.all(host(y)[k] > 0, axis=0)
        assert dead.any() and np.all(host(eng.nehvi(Xd))[dead] == 0.0)
        with pytest.raises(ValueError, match="no gradient through"):
            eng.nehvi_value_and_grad(host(Xd[:3]))
        # without constraints the earlier entries, and eta has nothing to smooth
        eng.sample_fronts(S, Y.max(0) + 0.2, lower, upper, seed=9, n_features=M)      # k + 1 objectives
        eng.plan_nehvi()
        assert eng.ctx.plan_kind[0] == "omb_plan_hvi_paths"
        with pytest.raises(ValueError, match="eta"):
            eng.nehvi(Xd, eta=0.1)
        with pytest.raises(ValueError, match="eta"):
            eng.plan_nehvi(eta=0.1)
    finally:
        eng.ctx.close()


# ------------------------------------------------------------------------------------------- 2. the chain
@pytest.fixture(scope="module")
def planned():
    """k = 2 objectives and one constraint model, S = 16 feasible fronts sampled, the plan set."""
    eng, models, X, Y, lower, upper = _engine(2, 1, n=40, d=3, seed=5, shift=-0.5)
    eng.sample_fronts(16, Y[:, :2].max(0) + 0.2, lower, upper, seed=2, n_features=M, n_con=1)
    eng.plan_nehvi()
    yield eng, models, lower, upper
    eng.ctx.close()


@pytest.mark.parametrize("chunk", [1000, 4096])
def test_eval_is_paths_eval_then_hvi_paths_con(planned, chunk):
    eng, _, lower, upper = planned
    ctx = eng.ctx
    try:
        ctx.debug_set("hvi_paths_chunk", chunk)
        for N in (1, 33, chunk - 1, chunk, chunk + 1):
            ctx.set_sobol(3, lower, upper, seed=N % 7)
            Xd = ctx.sobol(3, N)
            want = host(ctx.hvi_paths_con(ctx.paths_eval(Xd, 3), 1, *eng._front_lists))
            got = host(ctx.eval(Xd))
            assert same(got, want) and (N < 33 or (np.any(want > 0) and np.any(want == 0))), N
            best = int(np.argmax(want))
            pair = host(ctx.eval_argmax(Xd, offset=11))
            assert pair[0] == want[best] and int(pair[1]) == best + 11
            pair = host(ctx.eval_argmax_sobol(3, N))
            assert pair[0] == want[best] and int(pair[1]) == best + 3
            if N == chunk + 1:                           # one pass, the default, and a pass size that divides nothing
                for other in (0, HVI_PATHS_CHUNK, 777):
                    ctx.debug_set("hvi_paths_chunk", other)
                    assert same(host(ctx.eval(Xd)), want), other
    finally:
        ctx.debug_set("hvi_paths_chunk", HVI_PATHS_CHUNK)


def test_the_three_refusals_leave_the_plan_alone(planned):
    eng, _, lower, upper = planned
    ctx = eng.ctx
    lib, h = ctx.lib, ctx._h
    ctx.set_sobol(3, lower, upper, seed=8)
    Xd = ctx.sobol(0, 65)
    before = host(ctx.eval(Xd))
    assert lib.omb_plan_constraints(h, 1, 1e-5) == OMB_EUNSUP and b"sampled-front" in lib.omb_last_error(h)
    assert lib.omb_plan_constraints(h, 0, 0.0) == 0                   # clearing what is not there is no request
    for on in (1, 0):
        assert lib.omb_plan_log(h, on) == OMB_EUNSUP and b"sampled-front" in lib.omb_last_error(h)
    with pytest.raises(OMBError) as e:
        ctx.eval_grad(Xd)
    assert e.value.code == OMB_EUNSUP and "sampled-front" in str(e.value)
    assert not ctx.plan_has_gradient() and same(host(ctx.eval(Xd)), before)
    # omb_plan_hvi_paths and its refusals: as they were
    ctx.plan_hvi_paths(*eng._front_lists)
    assert lib.omb_plan_constraints(h, 1, 1e-5) == OMB_EUNSUP and b"takes no constraints" in lib.omb_last_error(h)
    plain = host(ctx.eval(Xd))
    assert same(plain, host(ctx.hvi_paths(ctx.paths_eval(Xd, 2), *eng._front_lists))) and np.all(plain >= before)
    eng.plan_nehvi()
    assert same(host(ctx.eval(Xd)), before)


@pytest.mark.parametrize("change", ["set_gp", "other_S", "no_gp"])
def test_a_changed_constraint_slot_is_refused_not_evaluated(change):
    from optimobo_amd.paths import draw_path_inputs
    eng, models, X, Y, lower, upper = _engine(2, 1)
    ctx = eng.ctx
    try:
        Xd = dev(np.random.default_rng(0).uniform(0, 1, (9, 2)))
        out = torch.full((9,), -7.0, dtype=torch.float64, device="cuda:0")
        eng.sample_fronts(4, Y[:, :2].max(0) + 0.2, lower, upper, seed=1, n_features=M, n_con=1)
        lists = eng._front_lists
        eng.plan_nehvi()
        assert np.all(host(ctx.eval(Xd)) >= 0)
        st = models[2]
        if change == "set_gp":
            ctx.set_gp_state(2, st)                      # the constraint slot loses its paths
        elif change == "other_S":
            om, ph, w, z = draw_path_inputs(st.kernel, len(X), 2, 5, M, np.random.default_rng(1), lower=lower,
                                            upper=upper, lengthscale=np.asarray(st.lengthscale, np.float64))
            ctx.paths_set(2, om, ph, w, z, noise=1e-3)   # the plan says 4
        else:                                            # two constraints planned, one constraint model loaded
            ctx.plan_hvi_paths_con(2, *lists)
        for call in (lambda: ctx.lib.omb_eval(ctx._h, ctypes.c_void_p(Xd.data_ptr()), 9, ctypes.c_void_p(out.data_ptr())),
                     lambda: ctx.lib.omb_eval_argmax(ctx._h, ctypes.c_void_p(Xd.data_ptr()), 9, 0,
                                                     ctypes.c_void_p(out.data_ptr()))):
            assert call() == OMB_ESTATE
            assert b"omb_paths_set" in ctx.lib.omb_last_error(ctx._h) and \
                (b"objective 3" if change == "no_gp" else b"objective 2") in ctx.lib.omb_last_error(ctx._h)
        ctx.synchronize()
        assert bool((out == -7.0).all())                             # nothing was launched
        # the unconstrained plan over the same state reads the objectives' slots alone: it still stands
        ctx.plan_hvi_paths(*lists)
        assert np.all(np.isfinite(host(ctx.eval(Xd))))
        eng.sample_fronts(4, Y[:, :2].max(0) + 0.2, lower, upper, seed=1, n_features=M, n_con=1)
        eng.plan_nehvi()
        assert np.all(np.isfinite(host(ctx.eval(Xd))))
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------- 3. the estimator
def test_mean_of_the_weighted_path_values_is_exact_ehvi_times_feasibility():
    """Noise 0 and |g| ≥ 0.05 at every training row: every path's feasible front is the observed feasible front up to
    the jitter draw, the objectives' and the constraint's paths are independent, so the mean of u_s = t_s·1[g_s ≤ 0]
    estimates EHVI(feasible front)·P(g ≤ 0).  256 per-path values (16 installs of 16 paths) at 8 candidates away from
    the data with 0.1 < F < 0.9; the bar is 5 standard errors (DESIGN §24's).  The numpy restatement of the paths alone, on
    these seeds and candidates, is at 1.49 (run on the CPU); the device's figure is in DESIGN §26."""
    from optimobo_amd.acquisition import AcquisitionEngine
    from optimobo_amd.gp import GPState
    e = R.ESTIMATOR
    states, X, Y, r, _, _ = R.estimator_case()
    # the constraint x0 + x1 ≤ 1 observed with a margin: g = h + 0.05·sign(h), h = x0 + x1 − 1
    h = X.sum(1) - 1.0
    g = h + np.where(h <= 0, -0.05, 0.05)
    assert np.abs(g).min() >= 0.05 and 4 <= int((g <= 0).sum()) <= len(g) - 4
    # a short lengthscale: away from the data the constraint's posterior is wide enough for 0.1 < F < 0.9
    con = GPState(X, g, np.array([0.3, 0.3]), float(np.var(g)) + 0.1, kernel="matern52", noise=0.0)
    eng2 = AcquisitionEngine(0).load_models(states)
    eng = AcquisitionEngine(0).load_models(states + [con])
    try:
        rng = np.random.default_rng(e["seed"] + 1)
        pool = rng.uniform(0.0, 1.0, (600, e["d"]))
        pool = pool[np.min(np.linalg.norm(X[None, :, :] - pool[:, None, :], axis=2), axis=1) >= 0.12]
        pf = pareto.calc_pf(Y[g <= 0])
        Fp = host(eng.feasibility(pool, 1, pof_eps=0.0))
        a = host(eng2.ehvi_exact(pool, r, pf)) * Fp
        ok = np.flatnonzero((Fp > 0.1) & (Fp < 0.9))
        top = ok[np.argsort(-a[ok], kind="stable")[:8]]
        Xc, exact = pool[top], a[top]
        assert len(top) == 8 and np.all(exact > 0)
        us = []
        for i in range(e["installs"]):
            fronts = eng.sample_fronts(e["S"], r, np.zeros(e["d"]), np.ones(e["d"]), seed=e["first_install"] + i,
                                       n_features=e["m"], n_con=1)
            Ft = host(eng.path_values(X))
            assert np.array_equal(Ft[2] <= 0, np.broadcast_to(g <= 0, Ft[2].shape))   # every draw: the observed split
            assert all(len(f) >= 1 for f in fronts)
            v, u = eng.ctx.hvi_paths_con(eng.path_values(Xc), 1, *eng._front_lists, per_path=True)
            us.append(host(u))
            assert np.allclose(host(v), us[-1].mean(0), rtol=1e-12) and same(host(eng.nehvi(Xc)), host(v))
        us = np.concatenate(us)
        se = R.standard_errors(us, exact)
        print(f"path-mean constrained EHVI: worst {se.max():.2f} standard errors over 8 candidates (bar 5); "
              f"EHVI·F {exact.min():.3g}..{exact.max():.3g}, F {Fp[top].min():.2f}..{Fp[top].max():.2f}, "
              f"feasible paths per candidate {(us > 0).mean(0).round(2)}")
        assert us.shape == (256, 8) and se.max() <= 5.0
    finally:
        eng.ctx.close()
        eng2.ctx.close()


# ------------------------------------------------------------------------------------------- 4. Thompson batches
def _draws(eng, sampler, q, n_c, seed, lower, upper, n_models):
    """The draws ``thompson_batch`` took, made again: (candidates, draws (n_models, q, n_c))."""
    ctx = eng.ctx
    ctx.set_sobol(len(lower), lower, upper, seed=seed)
    Xc = ctx.sobol(0, n_c)
    if sampler == "paths":                               # the installed paths are the batch's
        return Xc, host(eng.path_values(Xc))
    rng = np.random.default_rng(seed)
    out = torch.empty((n_models, q, n_c), dtype=torch.float64, device="cuda:0")
    for o in range(n_models):
        ctx.posterior_samples(o, Xc, dev(rng.standard_normal((q, n_c))), out=out[o])
    return Xc, host(out)


@pytest.mark.parametrize("sampler", ["joint", "paths"])
@pytest.mark.parametrize("k", [1, 2])
def test_thompson_batch_nominates_feasible_candidates_else_the_least_violating(sampler, k):
    q, n_c, seed = 6, 1 << 10, 4
    for shift in (0.0, 3.0):                             # a feasible region; then none anywhere near
        eng, models, X, Y, lower, upper = _engine(k, 1, n=20, shift=shift)
        try:
            Yo, g = Y[:, :k], Y[:, k]
            feas = g <= 0
            PF = pareto.calc_pf(Yo[feas]) if k > 1 else None
            r = Yo.max(0) + 0.2 if k > 1 else None
            best = float(Yo[feas, 0].min() if feas.any() else Yo[:, 0].max()) if k == 1 else None
            kw = dict(PF=PF, max_point=r, n_candidates=n_c, seed=seed, sampler=sampler, n_features=M, n_con=1, best=best)
            Xb, info = eng.thompson_batch(q, lower, upper, **kw)
            Xc, D = _draws(eng, sampler, q, n_c, seed, lower, upper, k + 1)
            idx = info["indices"]
            assert same(Xb, host(Xc)[idx]) and len(set(idx.tolist())) == q           # no duplicates
            G = D[k]                                                                 # (q, n_c)
            has = (G <= 0).any(axis=1)
            assert info["infeasible_draws"] == int((~has).sum()) and info["zero_draws"] >= info["infeasible_draws"]
            assert has.all() if shift == 0.0 else not has.any()
            others = np.ones(n_c, bool)
            others[idx] = False
            for b in range(q):
                if has[b]:
                    assert G[b, idx[b]] <= 0 and info["values"][b] >= 0               # feasible under its own draw
                else:                                                                # the least violating one left
                    viol = np.maximum(G[b], 0.0)
                    assert info["values"][b] == -viol[idx[b]] and viol[idx[b]] <= viol[others].min()
            if k == 1 and shift == 0.0:      # the improvement over best, where there is one: the pick's own u
                f = D[0][np.arange(q), idx]
                assert same(info["values"], np.maximum(best - f, 0.0))
            if k == 1:
                with pytest.raises(ValueError, match="best"):
                    eng.thompson_batch(q, lower, upper, **{**kw, "best": None})
            if sampler == "paths":
                with pytest.raises(ValueError, match="polish"):
                    eng.thompson_batch(q, lower, upper, polish=True, **kw)
                Xr, ir = eng.thompson_batch(q, lower, upper, refine_rounds=1, n_refine=256, **kw)
                yr = host(eng.path_values(Xr))
                for b in range(q):               # a refined nominee never scores worse under its own draw
                    gb = yr[k, b, b]
                    assert (gb <= 0) if has[b] else (max(gb, 0.0) <= -info["values"][b])
                    assert ir["values"][b] >= info["values"][b]
        finally:
            eng.ctx.close()


# ------------------------------------------------------------------------------------------- 5. drivers
def _drive(kind, constraints):
    import optimobo_amd.algorithms.optimisers as opti
    import optimobo_amd.scalarisations as sc
    np.random.seed(17)
    common = dict(seed=1, n_candidates=1 << 10, polish="auto", batch_size=2,
                  **({} if constraints is None else dict(constraints=constraints)))
    if kind == "nehvi":
        opt = opti.MultiSurrogateOptimiser(cf.driver_problem(), [0, 0], [2.5, 2.0], mode="textbook", acquisition="nehvi",
                                           **common)
    elif kind == "nei":
        opt = opti.MonoSurrogateOptimiser(cf.driver_problem(), [0, 0], [2.5, 2.0], acquisition="nei", **common)
    else:
        opt = opti.MultiSurrogateOptimiser(cf.driver_problem(), [0, 0], [2.5, 2.0], mode="textbook",
                                           batch_strategy="thompson", thompson_sampler="paths", **common)
    opt.nehvi_samples, opt.nehvi_features = 4, M
    opt.thompson_candidates, opt.thompson_features, opt.thompson_refine_rounds = 1 << 10, M, 1
    if kind == "nei":
        return opt, opt.solve(sc.Tchebicheff([0, 0], [2.5, 2.0]), budget=6, n_init_samples=10)
    return opt, opt.solve(budget=6, n_init_samples=10)


@pytest.mark.parametrize("kind", ["nehvi", "nei", "thompson"])
def test_drivers_with_constraints_through_paths(kind):
    from optimobo_amd.result import Constrained_Res
    opt, a = _drive(kind, "paths")
    X = a.Xsample
    assert isinstance(a, Constrained_Res) and X.shape == (16, 2) and np.all(X >= 0) and np.all(X <= 1)
    assert len(np.unique(X.round(9), axis=0)) == 16 and opt.thompson_fallbacks == 0
    g = 1.5 - X[:, 0] - X[:, 1]
    assert len(a.X_feasible) == int((g <= 0).sum()) and len(a.X_infeasible) == int((g > 0).sum())
    assert len(a.hypervolume_convergence) == 3 and np.all(np.diff(a.hypervolume_convergence) >= 0)
    _, b = _drive(kind, "paths")
    assert same(a.Xsample, b.Xsample) and same(a.ysample, b.ysample)                 # bitwise repeatable
    _, free = _drive(kind, None)
    gf = 1.5 - free.Xsample[:, 0] - free.Xsample[:, 1]
    assert same(free.Xsample[:10], X[:10])                                           # the same initial design
    n_con, n_free = int((g[10:] <= 0).sum()), int((gf[10:] <= 0).sum())
    print(f"{kind}: {n_con} of 6 proposals feasible with constraints='paths', {n_free} of 6 with constraints=None "
          f"({int((g[:10] <= 0).sum())} of the 10 initial)")
    assert n_con >= n_free
