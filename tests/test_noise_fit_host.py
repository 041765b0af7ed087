"""CPU: the host numpy log marginal likelihood with the noise variance free (optimobo_amd.gp, the
specification of the device path) against scikit-learn, and the drivers' ``noise`` option.

Tolerances (the project's own, tests/test_gpu_gpfit.py): log p(y) 1e-7 relative + 1e-6 absolute; gradient 1e-5
of its largest entry.
"""
import numpy as np
import pytest

from _noise_fixture import noisy_data, sklearn_reference

SHAPES = [(1, 1), (20, 2), (96, 8), (97, 2), (64, 9), (129, 3), (300, 6), (150, 50), (12, 100)]


@pytest.mark.parametrize("kernel", ["matern52", "rbf"])
@pytest.mark.parametrize("noise", [1e-6, 1e-2, 0.5])
@pytest.mark.parametrize("n,d", SHAPES)
def test_host_free_noise_lml_grad_vs_sklearn(n, d, noise, kernel):
    from optimobo_amd.gp import RBF, GPRegression, Matern52
    X, y, ls, var = noisy_data(n, d, noise)
    kern = (Matern52 if kernel == "matern52" else RBF)(d, variance=var, lengthscale=ls, ARD=True)
    m = GPRegression(X, y[:, None], kern, noise_var=noise, device_fit=False)
    assert not m.Gaussian_noise.variance.fixed
    theta = m._get_free()
    assert theta.shape == (d + 2,)
    f, g = m._neg_lml_and_grad(theta)
    lml_s, g_s = sklearn_reference(n, d, noise, kernel)
    print(f"n={n} d={d} noise={noise} {kernel}: lml err {abs(-f - lml_s) / max(abs(lml_s), 1):.3g}, "
          f"grad err {np.max(np.abs(-g - g_s)) / np.max(np.abs(g_s)):.3g} of the largest entry")
    assert -f == pytest.approx(lml_s, rel=1e-7, abs=1e-6)
    np.testing.assert_allclose(-g, g_s, rtol=1e-5, atol=1e-5 * np.max(np.abs(g_s)))


def _problem():
    from optimobo_amd.problem import ElementwiseProblem

    class P(ElementwiseProblem):
        def __init__(self):
            super().__init__(n_var=2, n_obj=2, xl=np.zeros(2), xu=np.ones(2))

        def _evaluate(self, x, out, *args, **kwargs):
            out["F"] = np.array([x[0], 1 + x[1] - np.sqrt(x[0])])

    return P()


def _drivers():
    from optimobo_amd.algorithms.optimisers import MultiSurrogateOptimiser
    from optimobo_amd.algorithms.turbo import TuRBO_1
    return [lambda **kw: MultiSurrogateOptimiser(_problem(), np.zeros(2), np.full(2, 2.0), **kw),
            lambda **kw: TuRBO_1(_problem(), 2, **kw)]


@pytest.mark.parametrize("which", [0, 1], ids=["MultiSurrogateOptimiser", "TuRBO_1"])
def test_driver_noise_option(which):
    make = _drivers()[which]
    rng = np.random.default_rng(0)
    X, y = rng.uniform(0, 1, (8, 2)), rng.normal(size=8)
    m = make()._model(X, y)
    assert m.Gaussian_noise.variance.fixed and float(m.Gaussian_noise.variance) == 0.0
    m = make(noise=0.01)._model(X, y)
    assert m.Gaussian_noise.variance.fixed and float(m.Gaussian_noise.variance) == 0.01
    m = make(noise="fit")._model(X, y)
    assert not m.Gaussian_noise.variance.fixed and float(m.Gaussian_noise.variance) == 1.0
    for bad in (-1, "x"):
        with pytest.raises(ValueError):
            make(noise=bad)
