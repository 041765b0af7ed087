"""CPU checks behind the log-space acquisitions, on exactly the inputs tests/test_gpu_logacq.py uses:

  * the fp64 restatement (tests/_logacq_reference.py) against the 60-digit mpmath references — a sanity cap of
    1e-12 on e = |x − ref| / max(1, |ref|); the figures it prints are the ones the GPU tests multiply by 8;
  * conditions on those inputs: the linear value in fp64 numpy is exactly 0 on at least a third of them and above
    1e-200 on at least a third — inputs on which the linear form works everywhere would show nothing;
  * the log-EI and log-PoF partials against fourth-order (Richardson) differences of the mpmath value, at
    test_grad_reference's bar FD_BAR of the term sum;
  * the drivers' ValueErrors for log_acquisition that need no device.
"""
import mpmath as mp
import numpy as np
import pytest
from scipy.special import ndtr

import _constraints_fixture as cf
import _logacq_reference as R
import test_grad_reference as ref

CAP = 1e-12


def test_log_h_restatement_over_the_whole_range():
    """t from −1e8 to 10, through both switch points and far past where h itself underflows."""
    ts = np.concatenate([np.linspace(-1e4, -40, 300), np.linspace(-40, 10, 2001), -np.logspace(2, 8, 40),
                         [-30.0, np.nextafter(-30.0, 0), np.nextafter(-30.0, -100), -1.0, np.nextafter(-1.0, 0),
                          np.nextafter(-1.0, -2)]])
    want = np.array([float(R.mp_log_h(t)) for t in ts])
    e = R.err(R.log_h(ts), want)
    print(f"log h: worst e {e.max():.3g} at t = {ts[e.argmax()]:.6g}")
    assert e.max() <= CAP
    with np.errstate(all="ignore"):
        naive = np.log(ts * ndtr(ts) + R._npdf(ts))
    assert not np.isfinite(naive[ts <= -39.0]).any() and np.isfinite(want).all()
    e = R.err(R.log_ndtr(ts), np.array([float(R.mp_log_ndtr(t)) for t in ts]))
    print(f"log Phi: worst e {e.max():.3g} at t = {ts[e.argmax()]:.6g}")
    assert e.max() <= CAP


def test_log_h_limits():
    assert R.log_h(np.array([-np.inf]))[0] == -np.inf and R.log_h(np.array([np.inf]))[0] == np.inf
    assert np.isnan(R.log_h(np.array([np.nan]))[0]) and np.isnan(R.log_ndtr(np.array([np.nan]))[0])
    assert R.log_ndtr(np.array([-np.inf]))[0] == -np.inf and R.log_ndtr(np.array([np.inf]))[0] == 0.0
    assert R.log1mexp(np.array([0.0]))[0] == -np.inf and R.log1mexp(np.array([-np.inf]))[0] == 0.0
    d = -np.logspace(-300, 2.8, 200)
    want = np.array([float(mp.log(-mp.expm1(mp.mpf(float(x))))) for x in d])
    assert R.err(R.log1mexp(d), want).max() <= 1e-15


@pytest.mark.parametrize("c", [0, 1, 3])
def test_log_ei_restatement_on_the_gpu_inputs(c):
    mu, var = R.ei_inputs()
    e = R.err(R.log_ei(mu[:1 + c], var[:1 + c], R.BEST, 0.0, R.CON_EPS), R.ei_reference(c))
    print(f"log EI, c = {c}: worst e {e.max():.3g} over {e.size} inputs")
    assert mu.shape[1] >= 1000 and np.isfinite(R.ei_reference(c)).all() and e.max() <= CAP


@pytest.mark.parametrize("c", [1, 3])
def test_log_pof_restatement_on_the_gpu_inputs(c):
    mu, var = R.pof_inputs()
    e = R.err(R.log_pof(mu[:c], var[:c], 0.0), R.pof_reference(c))
    print(f"log F, c = {c}: worst e {e.max():.3g} over {e.size} inputs")
    assert np.isfinite(R.pof_reference(c)).all() and e.max() <= CAP


@pytest.mark.parametrize("k,P", R.BOX_SHAPES + (R.BOX_BIG,))
def test_log_box_sum_restatement_on_the_gpu_inputs(k, P):
    coords, boxes, mu, var = R.box_case(k, P)
    want = R.box_reference(k, P)
    e = R.err(R.log_box_sum(coords, boxes, mu, var), want)
    print(f"log box sum, k = {k}, B = {len(boxes)}: worst e {e.max():.3g}; column 0: {want[0]:.6f}")
    assert np.isfinite(want).all() and e.max() <= CAP


def test_box_cases_are_the_stated_ones():
    assert [len(R.box_case(k, P)[1]) for k, P in R.BOX_SHAPES] == [6, 22, 72, 228]
    assert len(R.box_case(*R.BOX_BIG)[1]) > 1024
    # the candidate at μ = r + 0.3, σ = 0.01: the linear sum is exactly 0, the true logarithm is not small
    for (k, P), want in zip(R.BOX_SHAPES, (-4543, -6739, -9240, -10416)):
        coords, boxes, mu, var = R.box_case(k, P)
        assert R.linear_box_sum(coords, boxes, mu[:, :1], var[:, :1])[0] == 0.0
        assert round(R.box_reference(k, P)[0]) == want


def _shares(lin):
    return float(np.mean(lin == 0.0)), float(np.mean(lin > 1e-200))


def test_the_linear_form_is_zero_on_a_third_of_the_inputs_and_alive_on_a_third():
    mu, var = R.ei_inputs()
    z, a = _shares(R.linear_ei(mu[0], var[0], R.BEST))
    assert z >= 1 / 3 and a >= 1 / 3, ("EI", z, a)
    pm, pv = R.pof_inputs()
    with np.errstate(all="ignore"):
        z, a = _shares(ndtr(-pm[0] / np.sqrt(pv[0])))
    assert z >= 1 / 3 and a >= 1 / 3, ("PoF", z, a)
    for k, P in R.BOX_SHAPES + (R.BOX_BIG,):
        coords, boxes, m, v = R.box_case(k, P)
        z, a = _shares(R.linear_box_sum(coords, boxes, m, v))
        assert z >= 1 / 3 and a >= 1 / 3, (k, P, z, a)


# ----------------------------------------------------------------------------------------------- partials
def _richardson_mp(f, x, h):
    return (8 * (f(x + h) - f(x - h)) - (f(x + 2 * h) - f(x - 2 * h))) / (12 * h)


def _partial_points(n=60):
    """Columns of ei_inputs() with σ² ≥ 1e-12, γ < −40 among them."""
    mu, var = R.ei_inputs()
    g = (R.BEST - mu[0]) / (np.sqrt(var[0]) + 1e-10)
    keep = np.flatnonzero(var[0] >= 1e-12)
    far = keep[g[keep] < -40.0][:n // 3]
    rest = keep[g[keep] >= -40.0][:n - len(far)]
    idx = np.concatenate([far, rest])
    assert len(far) >= 10
    return mu[:, idx], var[:, idx], g[idx]


def test_log_ei_partials_vs_richardson_of_the_reference():
    mu, var, g = _partial_points()
    dm, dv = R.log_ei_partials(mu[:1], var[:1], R.BEST)
    worst = 0.0
    for i in range(mu.shape[1]):
        m, v = mp.mpf(float(mu[0, i])), mp.mpf(float(var[0, i]))
        fm = _richardson_mp(lambda x: R.mp_log_ei(x, v, R.BEST), m, mp.mpf(1e-6) * mp.sqrt(v))
        fv = _richardson_mp(lambda x: R.mp_log_ei(m, x, R.BEST), v, mp.mpf(1e-6) * v)
        sigma = np.sqrt(var[0, i])
        s1 = sigma + 1e-10
        rho = -dm[0, i] * s1
        scale_v = (abs(1.0 / sigma) + abs(rho * g[i] / s1)) / (2.0 * sigma)      # the two terms of ∂/∂σ²
        worst = max(worst, abs(dm[0, i] - float(fm)) / abs(float(fm)), abs(dv[0, i] - float(fv)) / scale_v)
    print(f"log EI partials: worst {worst:.3g} of the term sum")
    assert worst <= ref.FD_BAR
    # where the linear gradient is 0 this one is not
    lin_dm, _ = ref.ei_partials(mu[:1], var[:1], R.BEST)
    far = g < -40.0
    assert np.all(lin_dm[0, far] == 0.0) and np.all(dm[0, far] < 0.0) and np.all(np.isfinite(dv[0, far]))


def test_log_pof_partials_vs_richardson_of_the_reference():
    pm, pv = R.pof_inputs()
    keep = np.flatnonzero(pv[0] >= 1e-12)[:60]
    mu, var = pm[:1, keep], pv[:1, keep]
    eps = 1e-5
    dm, dv = R.log_pof_partials(mu, var, eps)
    worst = 0.0
    for i in range(mu.shape[1]):
        m, v = mp.mpf(float(mu[0, i])), mp.mpf(float(var[0, i]))
        h = mp.mpf(1e-6) * mp.sqrt(v + eps)
        fm = _richardson_mp(lambda x: R.mp_log_pof([x], [v], eps), m, h)
        fv = _richardson_mp(lambda x: R.mp_log_pof([m], [x], eps), v, mp.mpf(1e-6) * (v + eps))
        for an, fd in ((dm[0, i], float(fm)), (dv[0, i], float(fv))):
            worst = max(worst, abs(an - fd) / abs(fd) if fd != 0.0 else abs(an))
    print(f"log F partials: worst {worst:.3g} relative")
    assert worst <= ref.FD_BAR
    z = -mu[0] / np.sqrt(var[0] + eps)
    assert (z < -40.0).sum() >= 5 and np.all(dm[0, z < -40.0] < 0.0)


# ----------------------------------------------------------------------------------------------- drivers
def test_log_acquisition_value_errors():
    import optimobo_amd.algorithms.optimisers as opti
    from optimobo_amd.algorithms import cparego, emo, keep, parego
    M, S = opti.MultiSurrogateOptimiser, opti.MonoSurrogateOptimiser
    p = cf.driver_problem
    assert M(p(), [0, 0], [2, 2]).log_acquisition is False and S(p(), [0, 0], [2, 2]).log_acquisition is False
    assert M(p(), [0, 0], [2, 2], mode="textbook", log_acquisition=True).log_acquisition is True
    assert S(p(), [0, 0], [2, 2], log_acquisition=True).log_acquisition is True
    assert S(p(), [0, 0], [2, 2], log_acquisition=True, constraints="pof").log_acquisition is True
    with pytest.raises(ValueError, match="textbook"):
        M(p(), [0, 0], [2, 2], mode="reference", log_acquisition=True)
    with pytest.raises(ValueError, match="acquisition_func"):
        M(p(), [0, 0], [2, 2], mode="textbook", log_acquisition=True).solve(
            budget=1, acquisition_func=lambda y, w: float(np.dot(y, w)))
    with pytest.raises(ValueError, match="True or False"):
        S(p(), [0, 0], [2, 2], log_acquisition="yes")
    for cls in (parego.ParEGO, keep.KEEP, emo.EMO, cparego.ParEGO_C1, cparego.ParEGO_C2):
        with pytest.raises(ValueError, match="does not support log_acquisition"):
            cls(p(), [0, 0], [2, 2], log_acquisition=True)
        assert cls(p(), [0, 0], [2, 2], log_acquisition=False).log_acquisition is False
