"""CPU: what tests/test_gpu_constraints.py compares the device against, checked without a device.

  * the numpy product rule of a·F (tests/_constraints_fixture.pof_partials over tests/test_grad_reference.py's
    partials) against fourth-order (Richardson) differences of the oracle, at test_grad_reference's bar FD_BAR;
  * the condition on the constraint tests' inputs: on the oracle's posterior of the fixture's constraint surrogates
    a good share of the candidates has F strictly inside (0, 1), a share has F ≈ 1 and a larger one F ≈ 0;
  * the drivers' ValueErrors under constraints="pof" that need no device.
"""
import numpy as np
import pytest

import _constraints_fixture as cf
import test_grad_reference as ref

CASES = ref.acquisition_cases()


def con_gps(name, k, c):
    """case_gps(name, k)'s surrogates followed by c constraint models centred on 0 (Φ(−μ/σ) neither 0 nor 1)."""
    centre = ([0.5, 0.0, 0.0] if name == "constrained_ei" else [0.5] * k)[:k] + [0.0] * c
    gps = ref.acq_gps(k + c, centre=centre)
    base = ref.case_gps(name, k)
    assert all(np.array_equal(a.y, b.y) and np.array_equal(a.X, b.X) for a, b in zip(gps, base))
    return gps


@pytest.mark.parametrize("c", [1, 2])
@pytest.mark.parametrize("name", sorted(CASES))
def test_product_rule_vs_richardson(name, c):
    k, value, partials, _ = CASES[name]
    gps = con_gps(name, k, c)
    Xc = ref.make_candidates(gps[0], 33, train_point=False)
    wvalue, wpartials = cf.pof_value(value, k), cf.pof_partials(value, partials, k)

    def a_of_x(X):
        pm = [g.predict(X) for g in gps]
        mu = np.array([p[0][:, 0] for p in pm])
        var = np.array([p[1][:, 0] - g.noise for p, g in zip(pm, gps)])
        return wvalue(mu, var)

    grad, scale = ref.eval_grad(gps, Xc, wpartials)
    assert np.all(np.isfinite(a_of_x(Xc))) and np.all(np.isfinite(grad))
    err = ref.fd_error(grad, ref.richardson(a_of_x, Xc, ref.H_FD_ACQ), scale)
    # the constraint rows carry a share of the gradient: the test would pass on the objectives' rows alone otherwise
    g_obj, _ = ref.eval_grad(gps[:k], Xc, partials)
    share = np.abs(grad - g_obj * cf.pof(*_moments(gps[k:], Xc))[:, None]).max()
    print(f"{name} c={c}: worst |analytic - FD| / sum|terms| = {err:.2e}; |grad| up to {np.abs(grad).max():.3g}, "
          f"constraint rows' part up to {share:.3g}")
    assert err <= ref.FD_BAR
    assert (np.abs(grad).max(1) > 0).sum() >= 20
    assert share > 1e-3 * np.abs(grad).max()


def _moments(gps, Xc):
    pm = [g.predict(Xc) for g in gps]
    return (np.array([p[0][:, 0] for p in pm]), np.array([p[1][:, 0] - g.noise for p, g in zip(pm, gps)]))


def test_product_rule_is_finite_where_F_underflows():
    """Far inside the infeasible region F is exactly 0 while a > 0: the constraint rows are φ(z)·(…), not F/Φ(z)·(…)."""
    mu = np.array([[0.2, 0.2], [50.0, 0.1], [60.0, -0.2]])
    var = np.array([[0.04, 0.04], [1e-3, 0.05], [1e-3, 0.05]])
    value = lambda m, v: ref.oacq.ei(m[0], v[0], 0.55, 0.0)  # noqa: E731
    dm, dv = cf.pof_partials(value, lambda m, v: ref.ei_partials(m, v, 0.55, 0.0), 1)(mu, var)
    assert cf.pof(mu[1:], var[1:])[0] == 0.0 and value(mu[:1], var[:1])[0] > 0
    assert np.all(np.isfinite(dm)) and np.all(np.isfinite(dv))
    assert np.all(dm[:, 0] == 0.0) and np.any(dm[1:, 1] != 0.0)


@pytest.mark.parametrize("d", [2, 6, 12])
@pytest.mark.parametrize("n", [20, 100, 130, 520])
def test_feasibility_bands_on_the_oracle(n, d):
    """Two constraints, pof_eps 1e-5: the shares at these shapes and seeds are 11–39 % (middle), 12–20 % (F ≥ 0.99)
    and 47–71 % (F ≤ 0.01), and most cases have a few F exactly 0; the condition the tests need is the weaker one of
    assert_bands, which also holds with the first constraint alone."""
    _, _, _, mu, var = cf.problem(n, d, 1000 * n + d, 2, 2)
    F = cf.pof(mu[2:], var[2:])
    mid, top, bottom = cf.bands(F)
    print(f"n={n} d={d}: F in (0.01, 0.99) {mid:.1%}, >= 0.99 {top:.1%}, <= 0.01 {bottom:.1%}, "
          f"exactly 0: {(F == 0).sum()}")
    cf.assert_bands(F, (n, d))
    F1 = cf.pof(mu[2:3], var[2:3])
    print(f"  one constraint: {tuple(round(b, 3) for b in cf.bands(F1))}")
    cf.assert_bands(F1, (n, d, "c=1"))


# ------------------------------------------------------------------------------------------- drivers, no device
def _opti():
    import optimobo_amd.algorithms.optimisers as opti
    return opti


def test_constraints_none_is_the_default():
    opti = _opti()
    opt = opti.MultiSurrogateOptimiser(cf.driver_problem(), [0, 0], [2, 2])
    assert opt.constraints is None
    assert opti.MonoSurrogateOptimiser(cf.driver_problem(), [0, 0], [2, 2], constraints=None).constraints is None


def test_pof_value_errors():
    opti = _opti()
    from optimobo_amd.algorithms import cparego, emo, keep, parego
    M, S = opti.MultiSurrogateOptimiser, opti.MonoSurrogateOptimiser
    assert M(cf.driver_problem(), [0, 0], [2, 2], constraints="pof").n_con == 1
    assert S(cf.driver_problem(n_ieq_constr=7), [0, 0], [2, 2], constraints="pof").n_con == 7
    assert M(cf.driver_problem(n_ieq_constr=6), [0, 0], [2, 2], constraints="pof").n_con == 6
    for cls in (M, S):
        with pytest.raises(ValueError, match="n_ieq_constr"):
            cls(cf.driver_problem(n_ieq_constr=0), [0, 0], [2, 2], constraints="pof")
        with pytest.raises(ValueError, match="equality"):
            cls(cf.driver_problem(n_eq_constr=1), [0, 0], [2, 2], constraints="pof")
        with pytest.raises(ValueError, match="None or 'pof'"):
            cls(cf.driver_problem(), [0, 0], [2, 2], constraints="penalty")
    with pytest.raises(ValueError, match="8 models"):
        M(cf.driver_problem(n_ieq_constr=7), [0, 0], [2, 2], constraints="pof")        # 2 + 7
    with pytest.raises(ValueError, match="8 models"):
        M(cf.driver_problem(n_ieq_constr=3, n_obj=6), [0] * 6, [2] * 6, constraints="pof")
    with pytest.raises(ValueError, match="8 models"):
        S(cf.driver_problem(n_ieq_constr=8), [0, 0], [2, 2], constraints="pof")        # 1 + 8
    for cls in (emo.EMO, parego.ParEGO, keep.KEEP, cparego.ParEGO_C1, cparego.ParEGO_C2):
        with pytest.raises(ValueError, match="does not support"):
            cls(cf.driver_problem(), [0, 0], [2, 2], constraints="pof")
        assert cls(cf.driver_problem(), [0, 0], [2, 2], constraints=None).constraints is None


def test_pof_refuses_reference_ehvi_with_nonpositive_s01():
    """Reference-mode 2-D EHVI is ≤ 0 everywhere when its cache's s01 ≤ 0; the check comes before any evaluation."""
    opti = _opti()
    from optimobo_amd import pareto
    seed = next(s for s in range(200) if pareto.cache_stats(pareto.cached_samples(2, 5, seed=s))[1] <= 0)
    calls = []

    class Counting(type(cf.driver_problem())):
        def _evaluate(self, x, out, *args, **kwargs):
            calls.append(x)
            super()._evaluate(x, out, *args, **kwargs)

    opt = opti.MultiSurrogateOptimiser(Counting(), [0, 0], [2, 2], constraints="pof", mode="reference", seed=seed)
    with pytest.raises(ValueError, match="s01"):
        opt.solve(budget=1, n_init_samples=4)
    assert not calls
