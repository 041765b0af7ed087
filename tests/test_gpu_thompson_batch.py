"""GPU: Thompson-sampling batches — AcquisitionEngine.thompson_batch (posterior draws → omb_hvi_boxes →
omb_thompson_select) checked against a host recomputation from the device draws, and the drivers'
``batch_strategy="thompson"``."""
import warnings

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from _hvi_fixture import hvi_numpy  # noqa: E402

from optimobo_amd import pareto  # noqa: E402
from optimobo_amd._lib import OMB_ENOTPD, OMBError  # noqa: E402


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
    """TuRBO's greedy selection on the host: row b's arg-min (lowest index among equals) over the candidates no
    earlier row took; also the candidates still available at each pick."""
    taken, picks, avail = np.zeros(score.shape[1], bool), [], []
    for row in score:
        avail.append(~taken.copy())
        i = int(np.argmin(np.where(taken, np.inf, row)))
        picks.append(i)
        taken[i] = True
    return np.array(picks), avail


@pytest.mark.parametrize("n,d,k,n_c,q", [(40, 3, 2, 300, 5), (30, 2, 3, 130, 3), (25, 2, 1, 200, 4)])
def test_thompson_batch_against_the_host(n, d, k, n_c, q):
    from optimobo_amd.acquisition import engine_for
    seed = 100 + k
    models, Y, lower, upper = _models(n, d, k, seed)
    eng = engine_for(models)
    if k == 1:
        PF = r = None
        eng.plan_ei(float(Y.min()), 0.0)
    else:
        PF, r = pareto.calc_pf(Y), Y.max(axis=0) + 0.1
        eng.plan_ehvi_exact(r, PF)
    Xprobe = torch.as_tensor(np.random.default_rng(1).uniform(lower, upper, (50, d)), device=eng.device)
    plan0 = eng.ctx.eval(Xprobe).cpu().numpy()

    X, info = eng.thompson_batch(q, lower, upper, PF=PF, max_point=r, n_candidates=n_c, seed=seed)
    idx = info["indices"]
    assert X.shape == (q, d) and len(set(idx.tolist())) == q and info["n_candidates"] == n_c
    assert np.all(X >= lower) and np.all(X <= upper)
    assert len(info["jitter"]) == k and all(j >= 0 for j in info["jitter"])

    # the same draws again: the Sobol' points of that seed, z per model in model order from default_rng(seed)
    eng.ctx.set_sobol(d, lower, upper, seed=seed)
    Xc = eng.ctx.sobol(0, n_c)
    assert np.array_equal(bits(Xc.cpu().numpy()[idx]), bits(X))
    rng = np.random.default_rng(seed)
    draws = np.stack([eng.ctx.posterior_samples(o, Xc, torch.as_tensor(rng.standard_normal((q, n_c)),
                                                                       device=eng.device))[0].cpu().numpy()
                      for o in range(k)])                     # (k, q, n_c)
    if k == 1:
        score = draws[0]
        value = score
        assert info["zero_draws"] == 0
    else:
        coords, _, boxes = pareto.box_decomposition(PF, r)
        value = hvi_numpy(draws.reshape(k, -1).T, coords, boxes).reshape(q, n_c)
        score = -value
        assert info["zero_draws"] == int(np.sum(value.max(axis=1) <= 0))
        assert np.mean(value > 0) > 0.02                      # the draws do improve on the front somewhere
    host, avail = _host_picks(score)
    distinct = True
    for b in range(q):
        best = score[b][avail[b]].min()
        assert avail[b][idx[b]]
        if k == 1:
            assert score[b, idx[b]] == best                   # the draws themselves are selected: no rounding gap
        else:
            # device and numpy HVI differ by rounding: the pick's host HVI is within 1e-10 of the best available
            assert value[b, idx[b]] >= (1 - 1e-10) * (-best)
            close = np.sum(value[b][avail[b]] >= (1 - 1e-10) * (-best))
            distinct &= close == 1 or best == 0
        np.testing.assert_allclose(info["values"][b], value[b, idx[b]], rtol=1e-10, atol=0)
    if distinct:                                              # no two candidates that close: the very same indices
        assert np.array_equal(idx, host), (idx, host)
    print(f"k={k}: picks {idx.tolist()} host {host.tolist()} zero draws {info['zero_draws']} "
          f"jitter {info['jitter']}")

    # the installed plan and the loaded states are as they were
    assert np.array_equal(bits(eng.ctx.eval(Xprobe).cpu().numpy()), bits(plan0))
    # and the batch is a function of its arguments
    X2, info2 = eng.thompson_batch(q, lower, upper, PF=PF, max_point=r, n_candidates=n_c, seed=seed)
    assert np.array_equal(bits(X2), bits(X)) and np.array_equal(bits(info2["values"]), bits(info["values"]))


def test_thompson_batch_all_zero_draws_fall_back_to_the_sobol_order():
    """A front no draw improves on: HVI ≡ 0 in every draw, so draw b nominates the lowest-index candidate not yet
    taken — the first q points of the Sobol' sequence."""
    from optimobo_amd.acquisition import engine_for
    models, Y, lower, upper = _models(30, 2, 2, 7)
    eng = engine_for(models)
    PF, r = np.array([[-1e3, -1e3]]), np.array([100.0, 100.0])
    X, info = eng.thompson_batch(4, lower, upper, PF=PF, max_point=r, n_candidates=128, seed=3)
    assert info["zero_draws"] == 4 and info["indices"].tolist() == [0, 1, 2, 3]
    assert np.all(info["values"] == 0.0)
    eng.ctx.set_sobol(2, lower, upper, seed=3)
    assert np.array_equal(bits(eng.ctx.sobol(0, 4).cpu().numpy()), bits(X))


def test_thompson_batch_argument_errors():
    from optimobo_amd.acquisition import engine_for
    models, Y, lower, upper = _models(20, 2, 2, 8)
    eng = engine_for(models)
    with pytest.raises(ValueError):
        eng.thompson_batch(3, lower, upper, n_candidates=64)             # two models need a front
    with pytest.raises(ValueError):
        eng.thompson_batch(65, lower, upper, PF=Y, max_point=Y.max(0) + 1, n_candidates=64)
    with pytest.raises(ValueError):
        eng.thompson_batch(0, lower, upper, PF=Y, max_point=Y.max(0) + 1, n_candidates=64)


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


def _solve(kind, n_obj, seed=4, **kw):
    import optimobo_amd.algorithms.optimisers as opti
    import optimobo_amd.scalarisations as sc
    problem, ideal, mx = _problem(n_obj)
    np.random.seed(31)
    if kind == "multi":
        opt = opti.MultiSurrogateOptimiser(problem, ideal, mx, n_candidates=2048, seed=seed, batch_size=4,
                                           batch_strategy="thompson", **kw)
        return opt, opt.solve(budget=8, n_init_samples=10)
    opt = opti.MonoSurrogateOptimiser(problem, ideal, mx, n_candidates=2048, seed=seed, batch_size=4,
                                      batch_strategy="thompson", **kw)
    return opt, opt.solve(sc.Tchebicheff(ideal, mx), budget=8, n_init_samples=10)


@pytest.mark.parametrize("kind,n_obj", [("multi", 2), ("multi", 3), ("mono", 2), ("mono", 3)])
def test_driver_thompson_batches(kind, n_obj):
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        opt, out = _solve(kind, n_obj)
    assert opt.thompson_fallbacks == 0                        # no fallback on these well-conditioned runs
    assert not [w for w in caught if "believer" in str(w.message)]
    assert out.Xsample.shape == (18, 2) and out.ysample.shape == (18, n_obj)
    assert np.all(np.abs(out.Xsample) <= 2)
    hv = out.hypervolume_convergence
    assert len(hv) == 2 and hv[1] >= hv[0] > 0
    for s in (10, 14):
        B = out.Xsample[s:s + 4]
        assert len({tuple(x) for x in B}) == 4, B            # distinct proposals in a batch
    _, again = _solve(kind, n_obj)
    assert np.array_equal(bits(again.Xsample), bits(out.Xsample))
    assert np.array_equal(bits(again.ysample), bits(out.ysample))
    assert np.array_equal(bits(again.hypervolume_convergence), bits(hv))
    print(f"{kind} n_obj={n_obj}: hypervolume {hv}")


@pytest.mark.parametrize("exc", [OMBError(OMB_ENOTPD, "omb_posterior_samples: not positive definite"),
                                 pareto.BoxBudgetError("box_decomposition: more than 131072 boxes")])
def test_driver_falls_back_to_the_believer_batch(monkeypatch, exc):
    from optimobo_amd.acquisition import AcquisitionEngine

    def refuse(self, *a, **kw):
        raise exc
    monkeypatch.setattr(AcquisitionEngine, "thompson_batch", refuse)
    with pytest.warns(RuntimeWarning, match="believer"):
        opt, out = _solve("multi", 2)
    assert opt.thompson_fallbacks == 2                        # both iterations
    assert out.Xsample.shape == (18, 2)
    for s in (10, 14):
        assert len({tuple(x) for x in out.Xsample[s:s + 4]}) == 4
