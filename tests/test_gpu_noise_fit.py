"""GPU: the GP fit with the noise variance free (omb_gp_lml_grad_noise, omb_gp_lml_grad_noise_batch,
GPRegression.optimize / gp.fit_concurrently on the device, the drivers' noise="fit").

Reference: scikit-learn, ConstantKernel(var) * Matern(ls, nu=2.5) [or RBF] + WhiteKernel(noise), alpha = 1e-8
(tests/_noise_fixture.py; the host numpy formula agrees with it to 1e-10, tests/test_noise_fit_host.py).

Tolerances: log p(y) 1e-7 relative + 1e-6 absolute and the first d + 1 gradient entries 1e-5 of the largest
entry (tests/test_gpu_gpfit.py).  The noise entry ½ σ_n² (αᵀα − tr Ky⁻¹) is held to 1e-5 of its term sum
½ σ_n² (αᵀα + tr Ky⁻¹), the convention of tests/test_gpu_grad.py: at large n_var the entry is 1e-3 or less of the
largest gradient entry, so a bar relative to that entry would not test it.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from _noise_fixture import data, noise_term_sum, noisy_data, sklearn_reference  # noqa: E402


@pytest.fixture(scope="module")
def ctx():
    from optimobo_amd.device import AcqContext
    c = AcqContext(0)
    yield c
    c.close()


SMALL = [(1, 1), (20, 2), (96, 8), (128, 8)]          # one workgroup
BLOCKED = [(129, 3), (64, 9), (300, 6), (257, 30)]
WIDE = [(12, 100), (150, 100)]
CASES = ([(n, d, nz, "matern52") for n, d in SMALL + BLOCKED + WIDE for nz in (1e-2, 0.5)] +
         [(n, d, 1e-6, "matern52") for n, d in [(96, 8), (129, 3)]] +
         [(n, d, nz, "rbf") for n, d in [(96, 8), (129, 3)] for nz in (1e-6, 1e-2, 0.5)])


@pytest.mark.parametrize("n,d,noise,kernel", CASES)
def test_noise_lml_grad_vs_sklearn(ctx, n, d, noise, kernel):
    X, y, ls, var = noisy_data(n, d, noise)
    lml, g, jit = ctx.gp_lml_grad(X, y, ls, var, noise, kernel, noise_grad=True)
    lml_s, g_s = sklearn_reference(n, d, noise, kernel)
    terms = noise_term_sum(X, y, ls, var, noise, kernel)
    print(f"n={n} d={d} noise={noise} {kernel}: lml err {abs(lml - lml_s) / max(abs(lml_s), 1):.3g}, "
          f"grad err {np.max(np.abs(g[:d + 1] - g_s[:d + 1])) / np.max(np.abs(g_s)):.3g} of the largest entry, "
          f"noise entry {g[d + 1]:.6g} err {abs(g[d + 1] - g_s[d + 1]) / terms:.3g} of its term sum")
    assert g.shape == (d + 2,)
    assert jit == 0.0
    assert lml == pytest.approx(lml_s, rel=1e-7, abs=1e-6)
    np.testing.assert_allclose(g[:d + 1], g_s[:d + 1], rtol=1e-5, atol=1e-5 * np.max(np.abs(g_s)))
    assert abs(g[d + 1] - g_s[d + 1]) <= 1e-5 * terms


@pytest.mark.parametrize("n,d", [(96, 8), (128, 8), (129, 3), (64, 9), (150, 100)])
def test_noise_entry_changes_nothing_else(ctx, n, d):
    """One workgroup, blocked and wide: log p(y), the first d + 1 entries and the jitter are omb_gp_lml_grad's bits;
    noise = 0 gives a last entry of exactly 0; two calls give the same bits."""
    X, y, ls, var = noisy_data(n, d, 1e-2)
    for noise in (1e-2, 0.0):
        l0, g0, j0 = ctx.gp_lml_grad(X, y, ls, var, noise)
        l1, g1, j1 = ctx.gp_lml_grad(X, y, ls, var, noise, noise_grad=True)
        l2, g2, j2 = ctx.gp_lml_grad(X, y, ls, var, noise, noise_grad=True)
        assert g0.shape == (d + 1,) and g1.shape == (d + 2,)
        assert l1 == l0 and j1 == j0 and np.array_equal(g1[:d + 1], g0)
        assert l2 == l1 and j2 == j1 and np.array_equal(g2, g1)
        if noise == 0.0:
            assert g1[d + 1] == 0.0
        else:
            assert g1[d + 1] != 0.0 and np.isfinite(g1[d + 1])


@pytest.mark.parametrize("n,d", [(20, 2), (96, 8), (119, 2), (40, 12)])
def test_noise_batch_matches_single(ctx, n, d):
    """omb_gp_lml_grad_noise_batch with a noise per problem: every problem bitwise its own single call."""
    rng = np.random.default_rng(n + d)
    X = torch.as_tensor(rng.uniform(0, 1, (n, d)), device="cuda:0")
    k = 3
    ys = [torch.as_tensor(rng.normal(size=n), device="cuda:0") for _ in range(k)]
    ls = rng.uniform(0.3, 2.0, (k, d))
    var = rng.uniform(0.5, 2.0, k)
    noises = np.array([1e-3, 0.05, 0.7])
    lml, grad, jit, status = ctx.gp_lml_grad_batch(X, ys, ls, var, noises, noise_grad=True)
    assert grad.shape == (k, d + 2)
    assert (status == 0).all()
    for p in range(k):
        l1, g1, j1 = ctx.gp_lml_grad(X, ys[p], ls[p], float(var[p]), float(noises[p]), noise_grad=True)
        assert lml[p] == l1 and np.array_equal(grad[p], g1) and jit[p] == j1
    # a scalar noise is that value for every problem
    lml_s, grad_s, _, status_s = ctx.gp_lml_grad_batch(X, ys, ls, var, 0.05, noise_grad=True)
    assert (status_s == 0).all() and lml_s[1] == lml[1] and np.array_equal(grad_s[1], grad[1])


@pytest.mark.parametrize("n", [40, 150])
def test_noise_entry_after_jitter_retries(ctx, n):
    """Duplicated inputs with σ_f² = 1e10 and σ_n² = 1e-7 (below half an ulp of the diagonal): both paths take
    jitchol's retries; the sums are taken at the jitter they end on."""
    rng = np.random.default_rng(n)
    base = rng.uniform(0, 1, (6, 2))
    X = base[np.arange(n) % 6]
    y = np.sin(3 * X).sum(1)
    ls, var, noise = np.array([0.5, 0.8]), 1e10, 1e-7
    l0, g0, j0 = ctx.gp_lml_grad(X, y, ls, var, noise)
    lml, g, jit = ctx.gp_lml_grad(X, y, ls, var, noise, noise_grad=True)
    assert jit > 0.0 and jit == j0
    assert lml == l0
    assert g.shape == (4,) and np.all(np.isfinite(g))


def _free_noise_inputs():
    X, y, _, _ = data(100, 2, 3)
    return X, y + 0.1 * np.random.default_rng(1003).standard_normal(100)


def test_optimize_with_free_noise_stays_on_device(monkeypatch):
    from optimobo_amd.gp import GPRegression, Matern52

    def host(self, theta):
        raise AssertionError("the host numpy evaluation ran in a device fit")

    X, y = _free_noise_inputs()
    m = GPRegression(X, y[:, None], Matern52(2, ARD=True), device_fit=True)
    assert not m.Gaussian_noise.variance.fixed
    monkeypatch.setattr(GPRegression, "_neg_lml_and_grad", host)
    res = m.optimize(max_f_eval=300)
    assert np.isfinite(res.fun) and res.x.shape == (4,)
    assert float(m.Gaussian_noise.variance) > 0.0


def test_device_free_noise_fit_reaches_host_optimum():
    """The rule of test_device_optimize_reaches_host_optimum, and the noise the data were given (σ_n = 0.1; the
    host fit alone gives σ_n² = 0.0095)."""
    from optimobo_amd.gp import GPRegression, Matern52
    X, y = _free_noise_inputs()
    out, noises = [], []
    for dev_fit in (False, True):
        m = GPRegression(X, y[:, None], Matern52(2, ARD=True), device_fit=dev_fit)
        m.optimize(max_f_eval=300)
        out.append(m._neg_lml_and_grad(m._get_free())[0])
        noises.append(float(m.Gaussian_noise.variance))
    print(f"-log p(y): host fit {out[0]:.10g}, device fit {out[1]:.10g}; noise: host {noises[0]:.6g}, "
          f"device {noises[1]:.6g}")
    assert out[1] <= out[0] + 1e-4 * abs(out[0])
    assert 0.5 * 0.01 <= noises[1] <= 2 * 0.01


@pytest.mark.parametrize("n", [20, 60, 96, 119])
def test_concurrent_free_noise_fits_match_sequential(n):
    """gp.fit_concurrently on three models with free noise: bitwise the hyperparameters, noises and predictions of
    fitting them one after another."""
    from optimobo_amd.gp import GPRegression, Matern52, fit_concurrently
    rng = np.random.default_rng(n)
    X = rng.uniform(-2, 2, (n, 2))
    Y = np.column_stack([100 * (X ** 2).sum(1), ((X[:, 0] - 1) ** 2 + X[:, 1] ** 2), np.sin(3 * X).sum(1)])
    Y = Y + np.array([5.0, 0.1, 0.05]) * rng.standard_normal(Y.shape)

    def models():
        return [GPRegression(X, Y[:, i:i + 1], Matern52(2, ARD=True)) for i in range(Y.shape[1])]

    seq = models()
    for m in seq:
        assert m.device_fit and not m.Gaussian_noise.variance.fixed
        m.optimize(max_f_eval=1000)
    con = models()
    fit_concurrently(con, max_f_eval=1000)
    Xc = rng.uniform(-2, 2, (257, 2))
    for a, b in zip(seq, con):
        assert float(a.kern.variance) == float(b.kern.variance)
        assert np.array_equal(a.kern.lengthscale.values, b.kern.lengthscale.values)
        assert float(a.Gaussian_noise.variance) == float(b.Gaussian_noise.variance)
        ma, va = a.predict(Xc)
        mb, vb = b.predict(Xc)
        assert np.array_equal(ma, mb) and np.array_equal(va, vb)


def test_solve_multi_surrogate_with_fitted_noise():
    """MultiSurrogateOptimiser(noise="fit").solve() on a noisy 2-objective problem runs to budget with surrogates
    whose noise variance was fitted."""
    import optimobo_amd.algorithms.optimisers as opti
    from optimobo_amd.problem import ElementwiseProblem

    noise_rng = np.random.default_rng(11)

    class Noisy(ElementwiseProblem):
        def __init__(self):
            super().__init__(n_var=2, n_obj=2, xl=np.zeros(2), xu=np.ones(2))

        def _evaluate(self, x, out, *args, **kwargs):
            x = np.asarray(x, np.float64)
            f = np.array([x[0], 1 + x[1] - np.sqrt(x[0])])
            out["F"] = f + 0.05 * noise_rng.standard_normal(2)

    fitted = []

    class Opt(opti.MultiSurrogateOptimiser):
        def _fit_many(self, X, ys):
            models = super()._fit_many(X, ys)
            fitted.append(models)
            return models

    np.random.seed(4)
    opt = Opt(Noisy(), np.full(2, -0.5), np.full(2, 2.5), n_candidates=4096, seed=6, noise="fit")
    out = opt.solve(budget=3, n_init_samples=16)
    assert out.ysample.shape == (19, 2) and out.Xsample.shape == (19, 2)
    assert out.pf_approx.shape[1] == 2
    assert len(out.hypervolume_convergence) == 3
    assert np.all(np.diff(out.hypervolume_convergence) >= -1e-12)
    assert np.all((out.Xsample >= 0) & (out.Xsample <= 1))
    assert len(fitted) == 3 and len(fitted[-1]) == 2
    for m in fitted[-1]:
        assert not m.Gaussian_noise.variance.fixed and float(m.Gaussian_noise.variance) > 0.0
