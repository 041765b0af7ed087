"""GPU: Thompson-sampling batches from posterior sample paths — AcquisitionEngine.thompson_batch(sampler="paths")
checked against a host recomputation from the device path values, its refinement rounds, and the drivers'
``thompson_sampler="paths"``."""
import warnings

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from _hvi_fixture import hvi_numpy  # noqa: E402

from optimobo_amd import pareto  # noqa: E402

N_C = 4096


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _models(n, d, k, seed):
    """k fixed-hyperparameter GPs on n points of smooth test functions over [-1, 2]^d."""
    from optimobo_amd.gp import GPState
    rng = np.random.default_rng(seed)
    lower, upper = np.full(d, -1.0), np.full(d, 2.0)
    X = rng.uniform(lower, upper, (n, d))
    centres = rng.uniform(0.0, 1.0, (k, d))
    Y = np.stack([np.sum((X - c) ** 2, axis=1) + 0.3 * np.sin(3 * X[:, 0] + o) for o, c in enumerate(centres)], 1)
    models = [GPState(X, Y[:, o], rng.uniform(0.8, 1.6, d), float(np.var(Y[:, o])) + 0.5) for o in range(k)]
    return models, Y, lower, upper


def _host_picks(score):
    taken, picks, avail = np.zeros(score.shape[1], bool), [], []
    for row in score:
        avail.append(~taken.copy())
        i = int(np.argmin(np.where(taken, np.inf, row)))
        picks.append(i)
        taken[i] = True
    return np.array(picks), avail


def _setup(n, d, k, seed):
    from optimobo_amd.acquisition import engine_for
    models, Y, lower, upper = _models(n, d, k, seed)
    eng = engine_for(models)
    if k == 1:
        PF = r = None
        eng.plan_ei(float(Y.min()), 0.0)
    else:
        PF, r = pareto.calc_pf(Y), Y.max(axis=0) + 0.1
        eng.plan_ehvi_exact(r, PF)
    return eng, Y, lower, upper, PF, r


@pytest.mark.parametrize("n,d,k,q", [(40, 3, 2, 5), (30, 2, 3, 3), (25, 2, 1, 4)])
def test_paths_batch_against_the_host(n, d, k, q):
    seed = 100 + k
    eng, Y, lower, upper, PF, r = _setup(n, d, k, seed)
    Xprobe = torch.as_tensor(np.random.default_rng(1).uniform(lower, upper, (50, d)), device=eng.device)
    plan0 = eng.ctx.eval(Xprobe).cpu().numpy()

    X, info = eng.thompson_batch(q, lower, upper, PF=PF, max_point=r, n_candidates=N_C, seed=seed, sampler="paths",
                                 n_features=256)
    idx = info["indices"]
    assert X.shape == (q, d) and len(set(idx.tolist())) == q and info["n_candidates"] == N_C
    assert info["sampler"] == "paths" and info["n_features"] == 256 and info["refined"] == []
    assert info["jitter"] == [0.0] * k
    assert np.all(X >= lower) and np.all(X <= upper)

    # the same draws again: the Sobol' points of that seed, the paths of sample_paths(q) from default_rng(seed)
    eng.ctx.set_sobol(d, lower, upper, seed=seed)
    Xc = eng.ctx.sobol(0, N_C)
    assert np.array_equal(bits(Xc.cpu().numpy()[idx]), bits(X))
    eng.sample_paths(q, n_features=256, seed=seed, lower=lower, upper=upper)
    draws = eng.path_values(Xc).cpu().numpy()                  # (k, q, N_C)
    assert draws.shape == (k, q, N_C)
    if k == 1:
        score = value = draws[0]
        assert info["zero_draws"] == 0
    else:
        coords, _, boxes = pareto.box_decomposition(PF, r)
        value = hvi_numpy(draws.reshape(k, -1).T, coords, boxes).reshape(q, N_C)
        score = -value
        assert info["zero_draws"] == int(np.sum(value.max(axis=1) <= 0))
        assert np.mean(value > 0) > 0.02
    host, avail = _host_picks(score)
    distinct = True
    for b in range(q):
        best = score[b][avail[b]].min()
        assert avail[b][idx[b]]
        if k == 1:
            assert score[b, idx[b]] == best
        else:
            assert value[b, idx[b]] >= (1 - 1e-10) * (-best)
            close = np.sum(value[b][avail[b]] >= (1 - 1e-10) * (-best))
            distinct &= close == 1 or best == 0
        np.testing.assert_allclose(info["values"][b], value[b, idx[b]], rtol=1e-10, atol=0)
    if distinct:
        assert np.array_equal(idx, host), (idx, host)
    print(f"k={k}: picks {idx.tolist()} host {host.tolist()} zero draws {info['zero_draws']}")

    assert np.array_equal(bits(eng.ctx.eval(Xprobe).cpu().numpy()), bits(plan0))       # plan and states untouched
    X2, info2 = eng.thompson_batch(q, lower, upper, PF=PF, max_point=r, n_candidates=N_C, seed=seed, sampler="paths",
                                   n_features=256)
    assert np.array_equal(bits(X2), bits(X)) and np.array_equal(bits(info2["values"]), bits(info["values"]))


@pytest.mark.parametrize("n,d,k,q", [(40, 3, 2, 5), (30, 2, 3, 3), (25, 2, 1, 4)])
def test_refinement_moves_a_nominee_only_to_a_strictly_better_point(n, d, k, q):
    seed = 200 + k
    eng, Y, lower, upper, PF, r = _setup(n, d, k, seed)
    kw = dict(PF=PF, max_point=r, n_candidates=N_C, seed=seed, sampler="paths", n_features=256, n_refine=1024)
    X0, info0 = eng.thompson_batch(q, lower, upper, **kw)
    X2, info2 = eng.thompson_batch(q, lower, upper, refine_rounds=2, **kw)
    assert np.array_equal(info2["indices"], info0["indices"]) and len(info2["refined"]) == 2
    assert np.all(X2 >= lower) and np.all(X2 <= upper)
    moved = [b for b in range(q) if not np.array_equal(X2[b], X0[b])]
    assert 0 < len(moved) <= sum(info2["refined"]) <= 2 * q
    # the paths of the last call are still installed: both points under the draw that nominated them
    both = eng.path_values(np.vstack([X0, X2])).cpu().numpy()        # (k, q, 2q)
    if k > 1:
        coords, _, boxes = pareto.box_decomposition(PF, r)
    for b in range(q):
        y0, y2 = both[:, b, b], both[:, b, q + b]
        if k == 1:
            v0, v2 = -y0[0], -y2[0]
            np.testing.assert_array_equal(-info2["values"][b], v2)
        else:
            v0, v2 = hvi_numpy(np.stack([y0, y2]), coords, boxes)
            np.testing.assert_allclose(info2["values"][b], v2, rtol=1e-10, atol=0)
        if b in moved:
            assert v2 > v0, (b, v0, v2)
        else:
            assert v2 == v0
    print(f"k={k}: refined {info2['refined']}, moved draws {moved}")


def test_zero_draws_fall_back_to_the_sobol_order_and_are_not_refined():
    from optimobo_amd.acquisition import engine_for
    models, Y, lower, upper = _models(30, 2, 2, 7)
    eng = engine_for(models)
    PF, r = np.array([[-1e3, -1e3]]), np.array([100.0, 100.0])
    X, info = eng.thompson_batch(4, lower, upper, PF=PF, max_point=r, n_candidates=N_C, seed=3, sampler="paths",
                                 n_features=64, refine_rounds=2)
    assert info["zero_draws"] == 4 and info["indices"].tolist() == [0, 1, 2, 3]
    assert np.all(info["values"] == 0.0) and info["refined"] == [0, 0]
    eng.ctx.set_sobol(2, lower, upper, seed=3)
    assert np.array_equal(bits(eng.ctx.sobol(0, 4).cpu().numpy()), bits(X))


def test_degenerate_lengthscale_is_floored_for_the_features():
    """A fit whose lengthscale collapsed in one dimension (ℓ = 2.3e-16: no frequency keeps its argument inside the
    cosine's range) still gets paths: the features are drawn for the floor of paths.feature_lengthscale and the update
    term keeps the fitted kernel.  The other model's paths pass through its data as ever."""
    from optimobo_amd.acquisition import AcquisitionEngine
    from optimobo_amd.gp import GPState
    rng = np.random.default_rng(12)
    lower, upper = np.full(2, -2.0), np.full(2, 2.0)
    X = rng.uniform(lower, upper, (30, 2))
    Y = np.stack([np.sum(X ** 2, 1), np.sum((X - 1) ** 2, 1)], 1)
    models = [GPState(X, Y[:, 0], np.array([2.3e-16, 0.9]), 4.0), GPState(X, Y[:, 1], np.array([0.8, 1.1]), 4.0)]
    eng = AcquisitionEngine().load_models(models)
    eng.sample_paths(8, n_features=128, seed=1, lower=lower, upper=upper)
    assert eng.paths_floored == 1
    at_data = eng.path_values(X).cpu().numpy()                   # (2, 8, 30)
    assert np.all(np.isfinite(at_data))
    assert np.abs(at_data[1] - Y[:, 1]).max() < 1e-2             # ε = sqrt(1e-8)·z off the data, no more
    PF, r = pareto.calc_pf(Y), Y.max(axis=0) + 0.1
    Xb, info = eng.thompson_batch(4, lower, upper, PF=PF, max_point=r, n_candidates=N_C, seed=1, sampler="paths",
                                  n_features=128, refine_rounds=1, n_refine=512)
    assert info["floored"] == 1 and np.all(np.isfinite(info["values"])) and Xb.shape == (4, 2)
    assert np.all(Xb >= lower) and np.all(Xb <= upper)
    eng.ctx.close()


def test_argument_errors():
    from optimobo_amd.acquisition import engine_for
    models, Y, lower, upper = _models(20, 2, 2, 8)
    eng = engine_for(models)
    with pytest.raises(ValueError, match="16"):
        eng.thompson_batch(17, lower, upper, PF=Y, max_point=Y.max(0) + 1, n_candidates=N_C, sampler="paths")
    with pytest.raises(ValueError, match="sampler"):
        eng.thompson_batch(3, lower, upper, PF=Y, max_point=Y.max(0) + 1, n_candidates=N_C, sampler="rff")
    with pytest.raises(ValueError):
        eng.thompson_batch(3, lower, upper, n_candidates=N_C, sampler="paths")       # two models need a front


def test_gp_regression_sample_paths():
    """The GPy look-alike's wrapper: functions of the seed, near the posterior mean where the data pin them."""
    from optimobo_amd.gp import GPRegression, Matern52
    rng = np.random.default_rng(0)
    X = rng.uniform(0.0, 1.0, (30, 2))
    y = np.sin(3 * X).sum(1)[:, None]
    m = GPRegression(X, y, Matern52(2, variance=1.0, lengthscale=[0.5, 0.7], ARD=True), noise_var=0.0)
    Xn = rng.uniform(0.0, 1.0, (50, 2))
    a = m.posterior_sample_paths(Xn, size=6, seed=4).cpu().numpy()
    assert a.shape == (6, 50)
    assert np.array_equal(bits(m.posterior_sample_paths(Xn, size=6, seed=4).cpu().numpy()), bits(a))
    at_data = m.posterior_sample_paths(X, size=6, seed=4).cpu().numpy()
    assert np.abs(at_data - y.T).max() < 1e-2                  # ε = sqrt(1e-8)·z off the data, no more


# ------------------------------------------------------------------------------------------------ the drivers
def _problem(n_obj):
    from optimobo_amd.problem import ElementwiseProblem

    class Bowls(ElementwiseProblem):
        def __init__(self):
            super().__init__(n_var=2, n_obj=n_obj, xl=np.array([-2, -2]), xu=np.array([2, 2]))

        def _evaluate(self, x, out, *args, **kwargs):
            f = [x[0] ** 2 + x[1] ** 2, (x[0] - 1) ** 2 + x[1] ** 2, x[0] ** 2 + (x[1] - 1) ** 2]
            out["F"] = f[:n_obj]
    return Bowls(), [0.0] * n_obj, [10.0, 15.0, 15.0][:n_obj]


def _solve(kind, n_obj, seed=4):
    import optimobo_amd.algorithms.optimisers as opti
    import optimobo_amd.scalarisations as sc
    problem, ideal, mx = _problem(n_obj)
    np.random.seed(31)
    kw = dict(n_candidates=2048, seed=seed, batch_size=4, batch_strategy="thompson", thompson_sampler="paths")
    if kind == "multi":
        opt = opti.MultiSurrogateOptimiser(problem, ideal, mx, **kw)
        opt.thompson_candidates = 8192
        return opt, opt.solve(budget=8, n_init_samples=10)
    opt = opti.MonoSurrogateOptimiser(problem, ideal, mx, **kw)
    opt.thompson_candidates = 8192
    return opt, opt.solve(sc.Tchebicheff(ideal, mx), budget=8, n_init_samples=10)


@pytest.mark.parametrize("kind,n_obj", [("multi", 2), ("multi", 3), ("mono", 2)])
def test_driver_thompson_batches_from_paths(kind, n_obj):
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        opt, out = _solve(kind, n_obj)
    assert opt.thompson_fallbacks == 0
    assert not [w for w in caught if "believer" in str(w.message)]
    assert out.Xsample.shape == (18, 2) and out.ysample.shape == (18, n_obj)
    assert np.all(np.abs(out.Xsample) <= 2)
    hv = out.hypervolume_convergence
    assert len(hv) == 2 and hv[1] >= hv[0] > 0
    for s in (10, 14):
        B = out.Xsample[s:s + 4]
        assert len({tuple(x) for x in B}) == 4, B
    _, again = _solve(kind, n_obj)
    assert np.array_equal(bits(again.Xsample), bits(out.Xsample))
    assert np.array_equal(bits(again.ysample), bits(out.ysample))
    assert np.array_equal(bits(again.hypervolume_convergence), bits(hv))
    print(f"{kind} n_obj={n_obj}: hypervolume {hv}")
