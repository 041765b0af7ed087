"""GPU: max-value entropy search — omb_mes, omb_plan_mes in the fused chain, its analytic gradient, the engine's
sample_minima / mes / plan_mes and the drivers' acquisition="mes" (DESIGN §23).

References and inputs come from tests/_mes_reference.py; tests/test_mes_host.py states, without a device, the
restatement's own error on exactly these inputs and the conditions on them.

Accuracy bar (DESIGN §22's rule): the worst e = |x − ref| / max(1, |ref|) of the device against the 60-digit reference
is at most 8 × the worst e of the fp64 numpy restatement on the same inputs.  Both figures are printed.  The accuracy
is taken on the full batch of each case; the smaller batches must give bitwise its leading values.
Gradient bar: tests/test_gpu_grad.py's, |dev − ref| ≤ 1e-9 · Σ|terms|.
"""
import ctypes

import numpy as np
import pytest
from scipy import linalg

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _constraints_fixture as cf  # noqa: E402
import _mes_reference as R  # noqa: E402
import test_grad_reference as ref  # noqa: E402

from optimobo_amd import _lib  # noqa: E402

BAR = 8.0
TOL = 1e-9
SENT = -7.5
N_SMALL = (1, 63, 64, 65)


@pytest.fixture(scope="module")
def ctx():
    from optimobo_amd.device import AcqContext
    c = AcqContext(0)
    yield c
    c.close()


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device="cuda:0")


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def host(t):
    return t.cpu().numpy()


def same(a, b):
    """Bit for bit, NaN matching NaN."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    na = np.isnan(a)
    return a.shape == b.shape and np.array_equal(na, np.isnan(b)) and \
        np.array_equal(a[~na].view(np.int64), b[~na].view(np.int64))


def padded(a, N):
    t = torch.full((a.shape[0], N + 3), float("nan"), dtype=torch.float64, device="cuda:0")
    t[:, :N] = dev(a[:, :N])
    return t[:, :N]


def upload(ctx, gps):
    for o, g in enumerate(gps):
        Linv = linalg.solve_triangular(g.L, np.eye(len(g.L)), lower=True)
        ctx.set_gp(o, g.X, g.lengthscale, g.variance, g.alpha, Linv, g.kernel)


# ------------------------------------------------------------------------------------------- 1. omb_mes
@pytest.mark.parametrize("k,S", R.CASES)
def test_mes_against_the_reference(ctx, k, S):
    mu, var, ys = R.inputs(k, S)
    want = R.reference(k, S)
    N = R.N_ACC
    out = torch.full((N + 1,), SENT, dtype=torch.float64, device="cuda:0")
    ctx.mes(padded(mu, N), padded(var, N), ys, out=out)
    ctx.synchronize()
    full = host(out)
    assert full[N] == SENT
    full = full[:N]
    e_dev, e_np = R.err(full, want).max(), R.err(R.mes(mu, var, ys), want).max()
    print(f"MES k={k} S={S} N={N}: device worst e {e_dev:.3g}, restatement worst e {e_np:.3g} (bar {BAR:g}x)")
    assert np.all(np.isfinite(full)) and np.all(full >= 0.0)
    assert e_dev <= BAR * e_np, (e_dev, e_np)
    for n in N_SMALL:                     # a pitch of n + 3 with NaN padding, a sentinel past n
        o = torch.full((n + 1,), SENT, dtype=torch.float64, device="cuda:0")
        ctx.mes(padded(mu, n), padded(var, n), ys, out=o)
        ctx.synchronize()
        assert same(host(o)[:n], full[:n]) and float(o[n]) == SENT, n
    # column 0 is column 17 of a batch shifted by 17
    sh = host(ctx.mes(dev(np.roll(mu, 17, axis=1)), dev(np.roll(var, 17, axis=1)), ys))
    assert same(sh[17:18], full[0:1]) and same(sh[17:], full[:N - 17])


def test_edge_rules_stay_in_their_column(ctx):
    mu, var, ys = R.inputs(3, 5)
    N = 130
    m, v = np.array(mu[:, :N]), np.array(var[:, :N])
    clean = host(ctx.mes(dev(m), dev(v), ys))
    m[1, 3], v[2, 64], v[0, 65], m[0, 129] = np.nan, 0.0, -1e-3, np.nan
    v[1, 7] = np.nan
    got = host(ctx.mes(dev(m), dev(v), ys))
    bad = np.zeros(N, bool)
    bad[[3, 64, 65, 129, 7]] = True
    assert np.all(np.isnan(got[bad])) and same(got[~bad], clean[~bad])
    assert np.all(got[~bad] >= 0.0)
    # a NaN y* is not inspected by the stand-alone entry: NaN for every candidate
    yn = np.array(ys)
    yn[1, 2] = np.nan
    assert np.all(np.isnan(host(ctx.mes(dev(m), dev(v), yn))))


def test_entry_checks(ctx):
    lib, h = ctx.lib, ctx._h
    E, OK = _lib.OMB_EINVAL, _lib.OMB_OK
    N = 9
    mu = torch.zeros((3, N), dtype=torch.float64, device="cuda:0")
    var = torch.ones((3, N), dtype=torch.float64, device="cuda:0")
    ys = torch.zeros((3, 64), dtype=torch.float64, device="cuda:0")
    out = torch.full((N,), SENT, dtype=torch.float64, device="cuda:0")
    f = lambda k, m, v, ld, n, y, S, o: lib.omb_mes(h, k, m, v, ld, n, y, S, o)  # noqa: E731
    assert f(0, ptr(mu), ptr(var), N, N, ptr(ys), 5, ptr(out)) == E and f(9, ptr(mu), ptr(var), N, N, ptr(ys), 5, ptr(out)) == E
    assert f(3, ptr(mu), ptr(var), N, N, ptr(ys), 0, ptr(out)) == E and f(3, ptr(mu), ptr(var), N, N, ptr(ys), 65, ptr(out)) == E
    assert f(3, ptr(mu), ptr(var), N, -1, ptr(ys), 5, ptr(out)) == E
    for args in ((None, ptr(var), ptr(ys), ptr(out)), (ptr(mu), None, ptr(ys), ptr(out)),
                 (ptr(mu), ptr(var), None, ptr(out)), (ptr(mu), ptr(var), ptr(ys), None)):
        assert f(3, args[0], args[1], N, N, args[2], 5, args[3]) == E
    assert f(3, ptr(mu), ptr(var), N - 1, N, ptr(ys), 5, ptr(out)) == E
    assert f(1, ptr(mu), ptr(var), 0, N, ptr(ys), 5, ptr(out)) == OK            # one row: the pitch is not read
    ctx.synchronize()
    assert bool(torch.isfinite(out).all())
    out.fill_(SENT)
    assert f(3, None, None, 0, 0, None, 64, None) == OK
    assert f(8, None, None, 0, 0, None, 1, None) == OK
    ctx.synchronize()
    assert bool((out == SENT).all())


# ------------------------------------------------------------------------------------------- 2. the chain
def _ystar(k, S, lo=0.1, hi=0.45, seed=0):
    return np.random.default_rng(60 + seed + 10 * k + S).uniform(lo, hi, (k, S))


@pytest.mark.parametrize("k,S", [(1, 3), (3, 5), (2, 64)])
def test_plan_mes_is_mes_over_the_posterior(ctx, k, S):
    gps = ref.acq_gps(k)
    upload(ctx, gps)
    ys = _ystar(k, S)
    Xc = ref.make_candidates(gps[0], 257, train_point=False)
    Xd = dev(Xc)
    ctx.plan_mes(ys)
    assert ctx.plan_has_gradient()
    vals = host(ctx.eval(Xd))
    mu, var = ctx.posterior(Xd, k)
    assert same(vals, host(ctx.mes(mu, var, ys)))
    assert np.all(np.isfinite(vals)) and np.all(vals >= 0.0)
    for off in (0, 1000):
        pair = host(ctx.eval_argmax(Xd, offset=off))
        assert same(pair[:1], vals[[np.argmax(vals)]]) and int(pair[1]) == int(np.argmax(vals)) + off
    # a Sobol' batch through the chain: the pair is the arg-max of eval over the same points
    ctx.set_sobol(3, np.zeros(3), np.ones(3), seed=2)
    Xs = ctx.sobol(5, 300)
    vs = host(ctx.eval(Xs))
    pair = host(ctx.eval_argmax_sobol(5, 300))
    assert same(pair[:1], vs[[np.argmax(vs)]]) and int(pair[1]) == 5 + int(np.argmax(vs))


def test_plan_mes_refuses_non_finite_minima(ctx):
    gps = ref.acq_gps(2)
    upload(ctx, gps)
    Xd = dev(ref.make_candidates(gps[0], 9, train_point=False))
    out = torch.full((9,), SENT, dtype=torch.float64, device="cuda:0")
    for bad in (np.nan, np.inf, -np.inf):
        ctx.plan_mes(_ystar(2, 5))
        ys = _ystar(2, 5)
        ys[1, 4] = bad
        assert ctx.lib.omb_plan_mes(ctx._h, 2, 5, ctypes.c_void_p(ys.ctypes.data)) == _lib.OMB_EINVAL
        assert ctx.lib.omb_eval(ctx._h, ptr(Xd), 9, ptr(out)) == _lib.OMB_ESTATE          # no plan is left
    ys = _ystar(2, 5)
    yp = ctypes.c_void_p(ys.ctypes.data)
    for k, S in ((0, 5), (9, 5), (2, 0), (2, 65)):
        assert ctx.lib.omb_plan_mes(ctx._h, k, S, yp) == _lib.OMB_EINVAL
    assert ctx.lib.omb_plan_mes(ctx._h, 2, 5, None) == _lib.OMB_EINVAL
    ctx.synchronize()
    assert bool((out == SENT).all())
    with pytest.raises(_lib.OMBError):
        ctx.plan_mes(np.full((2, 5), np.nan))
    assert not ctx.plan_has_gradient()


def test_plan_log_refuses_and_constraints_weigh(ctx):
    gps = ref.acq_gps(3, centre=[0.5, 0.5, 0.0])
    upload(ctx, gps)
    Xd = dev(ref.make_candidates(gps[0], 65, train_point=False))
    ys = _ystar(2, 5)
    ctx.plan_mes(ys)
    before = host(ctx.eval(Xd))
    for on in (1, 0):
        assert ctx.lib.omb_plan_log(ctx._h, on) == _lib.OMB_EUNSUP
        assert b"max-value entropy search" in ctx.lib.omb_last_error(ctx._h)
    assert ctx.lib.omb_plan_log(ctx._h, 2) == _lib.OMB_EINVAL
    assert same(host(ctx.eval(Xd)), before)
    ctx.plan_constraints(1, 1e-5)
    weighted = host(ctx.eval(Xd))
    mu, var = ctx.posterior(Xd, 3)
    assert same(weighted, host(ctx.feasibility(mu[2:], var[2:], 1e-5, acq=dev(before))))
    assert not same(weighted, before)
    ctx.plan_constraints(0)
    assert same(host(ctx.eval(Xd)), before)


# ------------------------------------------------------------------------------------------- 3. the gradient
GRAD_CASES = {
    # name: (k, S, constraint rows, (lo, hi) of y*)
    "k1": (1, 3, 0, (0.1, 0.45)), "k3": (3, 5, 0, (0.1, 0.45)), "k1-far": (1, 3, 0, (12.0, 12.5)),
    "k3-far": (3, 5, 0, (12.0, 12.5)), "k1+1": (1, 3, 1, (0.1, 0.45)), "k3+2-far": (3, 5, 2, (12.0, 12.5)),
}


@pytest.mark.parametrize("name", sorted(GRAD_CASES))
def test_eval_grad_on_mes(ctx, name):
    k, S, c, (lo, hi) = GRAD_CASES[name]
    gps = ref.acq_gps(k + c, centre=[0.5] * k + [0.0] * c)
    upload(ctx, gps)
    ys = _ystar(k, S, lo, hi)
    ctx.plan_mes(ys)
    if c:
        ctx.plan_constraints(c, 1e-5)
    assert ctx.plan_has_gradient()
    Xc = ref.make_candidates(gps[0], 33, train_point=False)
    vals, grad = ctx.eval_grad(dev(Xc))
    assert same(host(vals), host(ctx.eval(dev(Xc))))
    partials = lambda m, v: R.mes_partials(m, v, ys)  # noqa: E731
    if c:
        partials = cf.pof_partials(lambda m, v: R.mes(m, v, ys), partials, k, 1e-5)
    with np.errstate(all="ignore"):
        rg, scale = ref.eval_grad(gps, Xc, partials)
    g = host(grad)
    assert np.all(np.isfinite(g)) and np.all(np.isfinite(rg))
    e = np.abs(g - rg) / np.where(scale > 0, scale, 1.0)
    print(f"MES {name}: |dev - ref| / sum|terms| = {e.max():.3e} (tol {TOL:g}); |grad| up to {np.abs(rg).max():.3g}")
    assert np.all(np.abs(g - rg) <= TOL * scale), e.max()
    assert (np.abs(g).max(1) > 0).sum() == 33
    if name.endswith("far"):
        mu, var = ctx.posterior(dev(Xc), k)
        gam = (host(mu)[:, None, :] - ys[:, :, None]) / np.sqrt(host(var))[:, None, :]
        assert (gam.max(axis=(0, 1)) < -40.0).sum() >= 5
    for i in (0, 5, 32):           # N = 1 is that row of N = 33, bit for bit
        v1, g1 = ctx.eval_grad(dev(Xc[i:i + 1]))
        assert same(host(v1), host(vals[i:i + 1])) and same(host(g1[0]), host(grad[i]))


def test_eval_grad_nan_row_rule_on_mes(ctx):
    gps = ref.acq_gps(2)
    upload(ctx, gps)
    g = gps[0]
    Linv = linalg.solve_triangular(g.L, np.eye(len(g.L)), lower=True)
    ctx.set_gp(0, g.X, g.lengthscale, g.variance, g.alpha, 2.0 * Linv, g.kernel)      # a negative σ² at the data
    ctx.plan_mes(_ystar(2, 5))
    far = 3.0 + np.random.default_rng(3).uniform(0, 1, (6, 3))
    Xc = np.concatenate([far[:3], g.X[4:5], far[3:]])
    vals, grad = ctx.eval_grad(dev(Xc))
    assert bool(torch.isnan(vals[3])) and bool(torch.isnan(grad[3]).all())
    for i in (0, 1, 2, 4, 5, 6):
        v1, g1 = ctx.eval_grad(dev(Xc[i:i + 1]))
        assert bool(torch.isfinite(grad[i]).all())
        assert same(host(v1), host(vals[i:i + 1])) and same(host(g1[0]), host(grad[i]))


# ------------------------------------------------------------------------------------------- 4. engine
def _engine(k, n=30, d=2, seed=3):
    from optimobo_amd.acquisition import AcquisitionEngine
    from optimobo_amd.gp import GPState
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 1.0, (n, d))
    Y = np.stack([np.sin(3 * X[:, 0] + o) + np.cos(2 * X[:, 1] - o) for o in range(k)], 1)
    models = [GPState(X, Y[:, o], rng.uniform(0.4, 0.9, d), float(np.var(Y[:, o])) + 0.5) for o in range(k)]
    return AcquisitionEngine(0).load_models(models), X, np.zeros(d), np.ones(d)


@pytest.mark.parametrize("k", [1, 2])
def test_sample_minima(k):
    eng, X, lower, upper = _engine(k)
    try:
        with pytest.raises(RuntimeError, match="sample_minima"):
            eng.mes(X)
        with pytest.raises(RuntimeError, match="sample_minima"):
            eng.plan_mes()
        for S in (0, 17):
            with pytest.raises(ValueError, match="one path install"):
                eng.sample_minima(S, lower, upper)
        S, n_c, seed = 5, 1 << 10, 9
        ys = eng.sample_minima(S, lower, upper, n_candidates=n_c, seed=seed, n_features=128)
        assert ys.shape == (k, S) and ys is eng.ystar and np.all(np.isfinite(ys))
        # rebuilt from the same seed: the smaller of paths_min over the Sobol' set and over the training inputs
        eng.sample_paths(S, n_features=128, seed=seed, lower=lower, upper=upper)
        eng.ctx.set_sobol(2, lower, upper, seed=seed)
        vs, _ = eng.ctx.paths_min(eng.ctx.sobol(0, n_c), k)
        vt, _ = eng.ctx.paths_min(dev(X), k)
        assert same(ys, host(torch.minimum(vs, vt)))
        at_data = host(eng.path_values(X)).min(-1)
        assert np.all(ys <= at_data)
        # one refinement round: no entry increases
        yr = eng.sample_minima(S, lower, upper, n_candidates=n_c, seed=seed, n_features=128, refine_rounds=1,
                               n_refine=256)
        assert yr.shape == ys.shape and np.all(yr <= ys)
        # mes / plan_mes with None take the last result
        Xd = dev(np.random.default_rng(1).uniform(0, 1, (65, 2)))
        v = host(eng.mes(Xd))
        assert same(v, host(eng.mes(Xd, yr))) and np.all(v >= 0.0)
        eng.plan_mes()
        assert eng.has_gradient() and same(host(eng.ctx.eval(Xd)), v)
    finally:
        eng.ctx.close()


def test_maximise_with_the_analytic_polish():
    eng, X, lower, upper = _engine(2)
    try:
        eng.sample_minima(5, lower, upper, n_candidates=1 << 10, seed=4, n_features=128)
        eng.plan_mes()
        kw = dict(n_candidates=1 << 10, seed=3, refine_rounds=0)
        _, v0 = eng.maximise(None, lower, upper, polish=False, **kw)
        x, v = eng.maximise(None, lower, upper, polish="analytic", **kw)
        print(f"MES maximise: Sobol' round's best {v0:.6f}, polished {v:.6f}")
        assert np.isfinite(v) and v >= v0 and np.all(x >= lower) and np.all(x <= upper)
    finally:
        eng.ctx.close()


# ------------------------------------------------------------------------------------------- 5. drivers
def _check(out, n_init, budget, iters=None):
    X, Y = out.Xsample, out.ysample
    assert X.shape == (n_init + budget, 2) and Y.shape == (n_init + budget, 2)
    assert np.all(X >= 0.0) and np.all(X <= 1.0) and np.all(np.isfinite(Y))
    assert len(out.hypervolume_convergence) == (budget if iters is None else iters)


@pytest.mark.parametrize("constraints", [None, "pof"])
def test_mono_surrogate_mes(constraints):
    import optimobo_amd.algorithms.optimisers as opti
    import optimobo_amd.scalarisations as sc
    np.random.seed(41)
    opt = opti.MonoSurrogateOptimiser(cf.driver_problem(), [0, 0], [2.5, 2.0], constraints=constraints, seed=1,
                                      n_candidates=1 << 10, acquisition="mes", mes_samples=4, mes_candidates=1 << 10,
                                      polish="auto")
    _check(opt.solve(sc.Tchebicheff([0, 0], [2.5, 2.0]), budget=3, n_init_samples=8), 8, 3)
    assert constraints == "pof" or opt._mes_picks == 3      # (while no row is feasible a pick maximises F alone)


@pytest.mark.parametrize("constraints,batch_size", [(None, 1), ("pof", 1), (None, 2)])
def test_multi_surrogate_mes(constraints, batch_size):
    import optimobo_amd.algorithms.optimisers as opti
    np.random.seed(42)
    opt = opti.MultiSurrogateOptimiser(cf.driver_problem(), [0, 0], [2.5, 2.0], constraints=constraints, seed=1,
                                       mode="textbook", n_candidates=1 << 10, acquisition="mes", mes_samples=4,
                                       mes_candidates=1 << 10, polish="auto", batch_size=batch_size)
    _check(opt.solve(budget=3, n_init_samples=8), 8, 3, iters=2 if batch_size == 2 else 3)
    assert constraints == "pof" or opt._mes_picks == 3      # every pick of a believer batch samples again
