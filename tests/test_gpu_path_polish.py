"""GPU: the sample paths' gradient at work — ``sample_minima(polish=True)``, ``thompson_batch(polish=True)``
and ``maximise(polish="paths")`` on tiny models (n ≤ 40, d ≤ 3, m = 256), the flags' defaults bit for bit, and the
drivers' ``path_gradients`` switch."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from optimobo_amd import pareto  # noqa: E402

M = 256      # random Fourier features


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _models(k, n=30, d=3, seed=3, kernel="matern52"):
    from optimobo_amd.gp import GPState
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 1.0, (n, d))
    Y = np.stack([np.sin(3 * X[:, 0] + 1.3 * o) + np.cos(2 * X[:, 1] - o) + (X[:, -1] if o % 2 else -X[:, -1])
                  for o in range(k)], 1)
    return [GPState(X, Y[:, o], rng.uniform(0.4, 0.9, d), float(np.var(Y[:, o])) + 0.5, kernel=kernel, noise=1e-3)
            for o in range(k)], X, Y


@pytest.fixture(scope="module")
def eng():
    from optimobo_amd.acquisition import AcquisitionEngine
    e = AcquisitionEngine(0)
    yield e
    e.ctx.close()


LO, HI = np.zeros(3), np.ones(3)


# ------------------------------------------------------------------------------------------- sample_minima
@pytest.mark.parametrize("k,kernel", [(1, "matern52"), (2, "rbf")])
def test_sample_minima_polish(eng, k, kernel):
    models, X, Y = _models(k, n=40, kernel=kernel)
    eng.load_models(models)
    kw = dict(n_candidates=1 << 10, seed=5, n_features=M, refine_rounds=1, n_refine=256)
    plain = eng.sample_minima(8, LO, HI, **kw).copy()
    plain_X = eng.ystar_X.copy()
    off = eng.sample_minima(8, LO, HI, polish=False, **kw)
    assert same(off, plain) and same(eng.ystar_X, plain_X)               # the default, bit for bit
    pol = eng.sample_minima(8, LO, HI, polish=True, **kw)
    assert pol.shape == (k, 8) and eng.ystar_X.shape == (k, 8, 3) and eng.ystar is pol
    assert np.all(pol <= plain) and np.any(pol < plain)
    assert np.all(eng.ystar_X >= LO) and np.all(eng.ystar_X <= HI)
    vals = eng.path_values(eng.ystar_X.reshape(k * 8, 3)).cpu().numpy()  # (k, 8, k·8): each value is its path's own
    for o in range(k):
        for s in range(8):
            assert pol[o, s] == vals[o, s, o * 8 + s], (o, s)
    dec = plain - pol
    print(f"k={k} {kernel}: {int((dec > 0).sum())} of {dec.size} minima moved, median decrease {np.median(dec):.3e}, "
          f"largest {dec.max():.3e} (path values of order {np.abs(plain).mean():.2f})")


# ------------------------------------------------------------------------------------------- thompson_batch
@pytest.mark.parametrize("k", [1, 2])
def test_thompson_batch_polish(eng, k):
    models, X, Y = _models(k, n=40)
    eng.load_models(models)
    q = 6
    kw = dict(n_candidates=1 << 10, seed=9, sampler="paths", n_features=M, refine_rounds=1, n_refine=256)
    if k > 1:
        kw.update(PF=pareto.calc_pf(Y), max_point=Y.max(0) + 0.1)
    X0, i0 = eng.thompson_batch(q, LO, HI, **kw)
    Xf, jf = eng.thompson_batch(q, LO, HI, polish=False, **kw)
    assert same(X0, Xf) and same(i0["values"], jf["values"]) and "polished" not in jf    # the default, bit for bit
    X1, i1 = eng.thompson_batch(q, LO, HI, polish=True, **kw)
    assert 0 <= i1["polished"] <= q and i1["refined"] == i0["refined"] and same(i1["indices"], i0["indices"])
    moved = np.any(X1 != X0, axis=1)
    assert int(moved.sum()) == i1["polished"] and i1["polished"] >= 1
    v0, v1 = np.asarray(i0["values"]), np.asarray(i1["values"])
    assert np.all(v1 <= v0) if k == 1 else np.all(v1 >= v0)              # never worse
    assert np.all((v1 < v0) == moved) if k == 1 else np.all((v1 > v0) == moved)   # moved only on strict improvement
    assert np.all(X1 >= LO) and np.all(X1 <= HI)
    # distinct starts (thompson_select), and a run that ends on another nominee's point stays where it was
    assert len(np.unique(X0, axis=0)) == q and len(np.unique(X1, axis=0)) == q
    # values are the draw's own score at the returned X (the paths of the last call are still installed)
    F = eng.path_values(X1)                                              # (k, q, q)
    for b in range(q):
        if k == 1:
            assert v1[b] == float(F[0, b, b])
        else:
            coords, _, boxes = pareto.box_decomposition(kw["PF"], kw["max_point"])
            assert v1[b] == float(eng.ctx.hvi_boxes(F[:, b, :].contiguous(), coords, boxes)[b])
    with pytest.raises(ValueError, match="polish"):
        eng.thompson_batch(q, LO, HI, n_candidates=1 << 10, seed=9, polish=True,
                           **({} if k == 1 else dict(PF=kw["PF"], max_point=kw["max_point"])))


# ------------------------------------------------------------------------------------------- maximise
@pytest.mark.parametrize("k", [1, 2])
def test_maximise_polish_paths(eng, k):
    models, X, Y = _models(k, n=30)
    eng.load_models(models)
    eng.sample_fronts(8, (Y.max(0) + 0.1) if k > 1 else None, LO, HI, seed=4, n_features=M)
    eng.plan_nehvi()
    kw = dict(n_candidates=1 << 10, seed=2, refine_rounds=1, starts=3)
    x0, v0 = eng.maximise(None, LO, HI, polish=False, **kw)
    x1, v1 = eng.maximise(None, LO, HI, polish="paths", **kw)
    assert v1 >= v0 and np.all(x1 >= LO) and np.all(x1 <= HI)
    assert v1 == float(eng.score(None, x1[None, :])[0])
    v, g = eng.nehvi_value_and_grad(np.stack([x0, x1]))
    assert g.shape == (2, 3) and same(v, eng.nehvi(np.stack([x0, x1])).cpu().numpy()) and v[1] == v1
    print(f"k={k}: polish=False {v0:.6e}, polish='paths' {v1:.6e}, |grad| at the polished point {np.abs(g[1]).max():.2e}")
    # the plan layer is as it was: no analytic gradient under the sampled-front plan
    assert not eng.has_gradient()
    with pytest.raises(ValueError):
        eng.maximise(None, LO, HI, polish="analytic", **kw)
    # refused without its plan, its fronts or with an acq_fn
    with pytest.raises(ValueError, match="paths"):
        eng.maximise(lambda Xd: eng.nehvi(Xd), LO, HI, polish="paths", **kw)
    eng.plan_ei(float(Y[:, 0].min()))
    with pytest.raises(ValueError, match="paths"):
        eng.maximise(None, LO, HI, polish="paths", **kw)
    eng.plan_nehvi()
    eng.sample_paths(8, n_features=M, seed=1, lower=LO, upper=HI)        # new paths: the fronts are gone
    with pytest.raises(ValueError, match="paths"):
        eng.maximise(None, LO, HI, polish="paths", **kw)
    with pytest.raises(ValueError, match="polish"):
        eng.maximise(None, LO, HI, polish="gradient", **kw)


def test_polish_batch_default_is_the_plan(eng):
    models, X, Y = _models(1, n=30)
    eng.load_models(models)
    eng.plan_ei(float(Y[:, 0].min()))
    starts = np.random.default_rng(0).uniform(0.1, 0.9, (3, 3))
    a = eng.polish_batch(starts, LO, HI)
    b = eng.polish_batch(starts, LO, HI, value_and_grad=None)
    c = eng.polish_batch(starts, LO, HI, value_and_grad=eng.value_and_grad)
    for (xa, va), (xb, vb), (xc, vc) in zip(a, b, c):
        assert same(xa, xb) and va == vb and same(xa, xc) and va == vc


# ------------------------------------------------------------------------------------------- drivers
def _problem(n_obj, sd=0.02, seed=0):
    from optimobo_amd.problem import ElementwiseProblem

    class Noisy(ElementwiseProblem):
        def __init__(self):
            super().__init__(n_var=2, n_obj=n_obj, xl=np.zeros(2), xu=np.ones(2))
            self.rng = np.random.default_rng(seed)

        def _evaluate(self, x, out, *args, **kwargs):
            f = [x[0] + 0.2 * np.sin(4 * x[1]), (1 - x[0]) * (1 + x[1])][:n_obj]
            out["F"] = list(np.asarray(f) + sd * self.rng.standard_normal(n_obj))
    return Noisy()


def _run(budget=6, **kw):
    import optimobo_amd.algorithms.optimisers as opti
    np.random.seed(17)
    opt = opti.MultiSurrogateOptimiser(_problem(2), [-0.5, -0.5], [2.5, 2.5], seed=1, n_candidates=1 << 10,
                                       noise="fit", polish="auto", mode="textbook", **kw)
    opt.nehvi_samples, opt.nehvi_features, opt.mes_features, opt.thompson_features = 4, 64, 64, 64
    opt.thompson_candidates, opt.thompson_refine_rounds = 1 << 10, 1
    out = opt.solve(budget=budget, n_init_samples=8)
    X, Y = out.Xsample, out.ysample
    assert X.shape == (8 + budget, 2) and np.all(X >= 0.0) and np.all(X <= 1.0) and np.all(np.isfinite(Y))
    return out


DRIVERS = {"mes": dict(acquisition="mes", mes_samples=4, mes_candidates=1 << 10),
           "nehvi": dict(acquisition="nehvi"),
           "thompson": dict(batch_strategy="thompson", thompson_sampler="paths", batch_size=2)}


@pytest.mark.parametrize("name", sorted(DRIVERS))
def test_drivers_with_path_gradients(name):
    out = _run(path_gradients=True, **DRIVERS[name])
    again = _run(path_gradients=True, **DRIVERS[name])
    assert same(out.Xsample, again.Xsample)                              # seeded: the same run


def test_flag_off_is_the_run_that_never_names_it_and_misuse_raises():
    import optimobo_amd.algorithms.optimisers as opti
    a = _run(budget=3, **DRIVERS["nehvi"])
    b = _run(budget=3, path_gradients=False, **DRIVERS["nehvi"])
    assert same(a.Xsample, b.Xsample) and same(a.ysample, b.ysample)
    with pytest.raises(ValueError, match="path_gradients"):
        opti.MultiSurrogateOptimiser(_problem(2), [-0.5, -0.5], [2.5, 2.5], mode="textbook", path_gradients=True)
    with pytest.raises(ValueError, match="path_gradients"):
        opti.MultiSurrogateOptimiser(_problem(2), [-0.5, -0.5], [2.5, 2.5], mode="textbook", acquisition="mes",
                                     path_gradients=1)
