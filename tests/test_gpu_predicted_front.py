"""GPU: the predicted Pareto set above the kernel — ``AcquisitionEngine.predicted_front`` against the host
recomputation from omb_posterior's own output, its independence of ``chunk``, constraints, the empty front,
``path_fronts`` against the definition on ``path_values``, and ``MultiSurrogateOptimiser(model_front=True)``.
Small problems throughout: n = 40, d ≤ 3, 4096 candidates."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _constraints_fixture as cf  # noqa: E402
import _nondominated_reference as R  # noqa: E402

N_CAND = 4096


def _models(k, d, n=40, seed=3, n_con=0):
    from optimobo_amd.gp import GPState
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 1.0, (n, d))
    F = cf.objectives(X)                                 # f0 = x0 against (1 + x1)(1.2 − x0), then the ZDT1-like column
    Y = [F[:, o] for o in (0, 2, 1)[:k]]
    Y += [0.8 - X[:, 0] - X[:, 1]][:n_con]              # g ≤ 0 feasible: the half of the box beyond x0 + x1 = 0.8
    return [GPState(X, y, rng.uniform(0.4, 0.9, d), float(np.var(y)) + 0.5, noise=1e-3) for y in Y], X


def _engine(k, d, **kw):
    from optimobo_amd.acquisition import AcquisitionEngine
    models, X = _models(k, d, **kw)
    return AcquisitionEngine(0).load_models(models), X


def _host_front(eng, X, d, k, n_con=0, min_feasibility=0.5, seed=0):
    """The candidates in ``predicted_front``'s order, omb_posterior's own moments at them, and the definition."""
    eng.ctx.set_sobol(d, np.zeros(d), np.ones(d), seed=seed)
    C = torch.cat([torch.as_tensor(X, device="cuda:0"), eng.ctx.sobol(0, N_CAND)])
    mu, var = (t.cpu().numpy() for t in eng.posterior(C))
    feas = np.ones(len(C), bool)
    if n_con:
        F = eng.ctx.feasibility(*(torch.as_tensor(a[k:], device="cuda:0") for a in (mu, var)), 1e-5).cpu().numpy()
        feas = F >= min_feasibility
    idx = np.flatnonzero(feas)[R.definition(mu[:k, feas].T)]
    return C.cpu().numpy(), mu, var, feas, idx


@pytest.mark.parametrize("k, d", [(2, 2), (3, 3)])
def test_predicted_front_is_the_host_recomputation(k, d):
    eng, X = _engine(k, d)
    C, mu, var, _, idx = _host_front(eng, X, d, k)
    out = eng.predicted_front(np.zeros(d), np.ones(d), n_candidates=N_CAND, include=X)
    print(f"k = {k}: {len(idx)} of {len(C)} candidates on the model's front, {np.sum(idx < len(X))} of them training rows")
    assert 5 <= len(idx) < len(C) // 4
    assert np.array_equal(out["index"], idx) and out["index"].dtype == np.int64
    assert np.array_equal(out["X"], C[idx]) and np.array_equal(out["mean"], mu[:k, idx].T)
    assert np.array_equal(out["var"], var[:k, idx].T)
    assert out["info"] == dict(chunk_survivors=[len(idx)], feasible=len(C), candidates=len(C))
    # chunk = 1000: pieces that end inside the Sobol' points; 25: inside the training rows as well
    for chunk in (1000, 25 if k == 2 else 4136):
        got = eng.predicted_front(np.zeros(d), np.ones(d), n_candidates=N_CAND, include=X, chunk=chunk)
        for key in ("X", "mean", "var", "index"):
            assert np.array_equal(got[key], out[key]), (chunk, key)
        assert len(got["info"]["chunk_survivors"]) == -(-len(C) // chunk)
        assert sum(got["info"]["chunk_survivors"]) >= len(idx)
    # without the training rows the indices are the Sobol' points' own
    bare = eng.predicted_front(np.zeros(d), np.ones(d), n_candidates=N_CAND)
    sob = R.definition(mu[:k, len(X):].T)
    assert np.array_equal(bare["index"], np.flatnonzero(sob)) and np.array_equal(bare["X"], C[len(X):][sob])


def test_predicted_front_under_a_constraint_model():
    k, d = 2, 2
    eng, X = _engine(k, d, n_con=1)
    C, mu, var, feas, idx = _host_front(eng, X, d, k, n_con=1, min_feasibility=0.6)
    assert 0.2 < feas.mean() < 0.8 and len(idx) >= 5
    free = np.flatnonzero(R.definition(mu[:k].T))
    assert not np.array_equal(free, idx)                # the constraint changes the front
    for chunk in (1 << 18, 1000):
        out = eng.predicted_front(np.zeros(d), np.ones(d), n_candidates=N_CAND, n_con=1, min_feasibility=0.6, include=X,
                                  chunk=chunk)
        assert np.array_equal(out["index"], idx) and np.array_equal(out["mean"], mu[:k, idx].T)
        assert np.array_equal(out["var"], var[:k, idx].T) and out["mean"].shape[1] == k
        assert out["info"]["feasible"] == feas.sum()
        F = eng.feasibility(torch.as_tensor(out["X"], device="cuda:0"), 1).cpu().numpy()
        assert np.all(F >= 0.6)
    # a threshold no candidate reaches: the empty front, not an error
    out = eng.predicted_front(np.zeros(d), np.ones(d), n_candidates=N_CAND, n_con=1, min_feasibility=1.5, include=X)
    assert out["info"]["feasible"] == 0 and out["X"].shape == (0, d) and out["mean"].shape == (0, k)
    assert out["var"].shape == (0, k) and out["index"].shape == (0,)


@pytest.mark.parametrize("S", [1, 16])
def test_path_fronts_are_the_definition_on_path_values(S):
    k, d = 2, 2
    eng, X = _engine(k, d)
    eng.sample_paths(S, n_features=64, seed=7, lower=np.zeros(d), upper=np.ones(d))
    Xc = torch.as_tensor(np.random.default_rng(S).uniform(size=(2049, d)), device="cuda:0")
    Y = eng.path_values(Xc).cpu().numpy()               # (k, S, N)
    fronts = eng.path_fronts(Xc)
    assert len(fronts) == S
    sizes = []
    for s, (idx, vals) in enumerate(fronts):
        want = np.flatnonzero(R.definition(Y[:, s, :].T))
        assert idx.dtype == torch.int64 and np.array_equal(idx.cpu().numpy(), want)
        assert np.array_equal(vals.cpu().numpy(), Y[:, s, want].T)
        sizes.append(len(want))
    assert min(sizes) >= 1 and (S == 1 or len({tuple(f[0].tolist()) for f in fronts}) > 1)      # the sets differ


def _readme_problem():
    from optimobo_amd.problem import ElementwiseProblem

    class MyProblem(ElementwiseProblem):        # README.md:28-39
        def __init__(self):
            super().__init__(n_var=2, n_obj=2, xl=np.array([-2, -2]), xu=np.array([2, 2]))

        def _evaluate(self, x, out, *args, **kwargs):
            out["F"] = [100 * (x[0] ** 2 + x[1] ** 2), (x[0] - 1) ** 2 + x[1] ** 2]
    return MyProblem()


def _run(**kw):
    import optimobo_amd.algorithms.optimisers as opti
    np.random.seed(0)
    opt = opti.MultiSurrogateOptimiser(_readme_problem(), [0, 0], [700, 12], n_candidates=4096, seed=1, **kw)
    return opt, opt.solve(budget=14, n_init_samples=10)


def test_driver_reports_the_model_front():
    from optimobo_amd import acquisition
    kw = dict(model_front=True, model_front_candidates=N_CAND)
    opt, out = _run(**kw)
    Xm, mean, var = out.model_pf_inputs, out.model_pf_mean, out.model_pf_var
    P = len(Xm)
    print(f"model front: {P} points, {len(out.pf_approx)} on the observed front")
    assert P >= 1 and Xm.shape == (P, 2) and mean.shape == (P, 2) and var.shape == (P, 2)
    assert np.all(Xm >= -2) and np.all(Xm <= 2) and np.all(np.isfinite(mean)) and np.all(np.isfinite(var))
    assert R.definition(mean).all()                     # mutually non-dominated
    # the engine still holds the final fit: no evaluated point's posterior mean dominates a member
    eng = acquisition._ENGINES[torch.cuda.current_device()]
    mu = eng.posterior(torch.as_tensor(out.Xsample, device="cuda:0"))[0].cpu().numpy()[:2].T
    assert R.definition(np.vstack([mu, mean]))[len(mu):].all()
    _, again = _run(**kw)
    _, off = _run()
    assert out.ysample.shape == (24, 2) and np.array_equal(out.ysample, off.ysample)
    assert np.array_equal(out.Xsample, off.Xsample) and np.array_equal(out.pf_approx, off.pf_approx)
    assert off.model_pf_inputs is None and off.model_pf_mean is None and off.model_pf_var is None
    for a, b in ((Xm, again.model_pf_inputs), (mean, again.model_pf_mean), (var, again.model_pf_var),
                 (out.ysample, again.ysample)):
        assert np.array_equal(a, b)
