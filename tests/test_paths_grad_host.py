"""CPU: the gradient restatements of tests/_paths_grad_reference.py against central differences of the value
restatements they differentiate (np.longdouble), the kink and y ≥ r conventions of the sampled-front improvement's
gradient, and ``polish_batch`` on a caller's value-and-gradient."""
import numpy as np
import pytest

import _nehvi_reference as nr
import _paths_grad_reference as gr
import _paths_reference as pr
from _posterior_xp import LD

from optimobo_amd import pareto, paths


@pytest.mark.parametrize("kernel", ["matern52", "rbf"])
@pytest.mark.parametrize("d", [1, 6, 9])
def test_path_gradient_against_central_differences(kernel, d):
    n, m, S, N = 12, 24, 3, 6
    rng = np.random.default_rng(10 * d + len(kernel))
    st = pr.make_state(n, d, kernel, seed=d, noise=1e-6)
    omega, phase, w, z = paths.draw_path_inputs(kernel, n, d, S, m, rng, np.zeros(d), np.ones(d), st.lengthscale)
    Xc = rng.uniform(0.1, 0.9, (N, d))
    Xc[0] = st.X[4]                                            # exactly on a training row: r = 0
    g, T = gr.path_gradient(st, kernel, omega, phase, w, z, 1e-6, Xc)
    g64, _ = gr.path_gradient(st, kernel, omega, phase, w, z, 1e-6, Xc, dtype=np.float64)
    assert g.dtype == LD and np.all(np.isfinite(g.astype(np.float64)))
    h = 2.0 ** -20                                              # exact in fp64 on [0.1, 1): x ± h are the points meant
    for j in range(d):
        Xp, Xm = Xc.copy(), Xc.copy()
        Xp[:, j] += h
        Xm[:, j] -= h
        fp, _, _ = pr.reference(st, kernel, omega, phase, w, z, 1e-6, Xp)
        fm, _, _ = pr.reference(st, kernel, omega, phase, w, z, 1e-6, Xm)
        fd = (fp - fm) / (Xp[:, j].astype(LD) - Xm[:, j].astype(LD))[None, :]
        # central differences: O(h²·f''') — the third derivative of a Matern-5/2 path is bounded away from r = 0 and
        # jumps at it, where the bound is O(h·|f''| jump); 1e-4 of the term sum covers both at h = 2^-20
        err = np.abs(fd - g[:, j, :]) / T[:, j, :]
        assert float(err.max()) < 1e-4, (j, float(err.max()))
    # the fp64 restatement is the same formula: a few hundred ulp of the term sum at most
    assert float(gr.normalised(g64, g, T).max()) < 1e-12


def _hvi_case(k, S, d, N, seed):
    """Path values at least 1e-3 from every grid coordinate (asserted), packed lists and path gradients."""
    rng = np.random.default_rng(seed)
    if k == 1:
        _, lists = nr.thresholds_for(S, rng)
        y = rng.normal(size=(1, S, N))
    else:
        _, lists = nr.lists_for(k, [3 + s for s in range(S)], rng)
        y = nr.candidates(k, S, N, rng)
    coords = lists[0]
    gap = min(float(np.abs(y[j, s][:, None] - coords[s, j][None, np.isfinite(coords[s, j])]).min())
              for j in range(k) for s in range(S))
    assert gap >= 1e-3, gap
    dy = rng.normal(size=(k, S, d, N))
    return y, dy, lists


@pytest.mark.parametrize("k,seed", [(1, 1), (2, 0), (3, 2)])
def test_hvi_gradient_against_differences(k, seed):
    S, d, N = 3, 2, 5
    y, dy, lists = _hvi_case(k, S, d, N, seed)
    ref = gr.hvi_gradient(y, dy, *lists)
    f64 = gr.hvi_gradient(y, dy, *lists, dtype=np.float64)
    assert np.array_equal(np.asarray(ref["v"], np.float64), np.asarray(nr.alpha(y, *lists, dtype=LD), np.float64))
    # move x along direction e_l: y changes by h·dy[:, :, l, :]; t_s is piecewise polynomial of degree ≤ k in y, and no
    # kink lies within 1e-3 while the step moves y by h·|dy| < 1e-4: central differences err by O(h²) alone
    h = 2.0 ** -16
    for l in range(d):
        vp = nr.alpha(y + h * dy[:, :, l, :], *lists, dtype=LD)
        vm = nr.alpha(y - h * dy[:, :, l, :], *lists, dtype=LD)
        fd = (vp - vm) / (2 * LD(h))
        assert float(np.abs(fd - ref["g"][:, l]).max()) < 1e-7, l
        tp = nr.path_values(y + h * dy[:, :, l, :], *lists, dtype=LD)
        tm = nr.path_values(y - h * dy[:, :, l, :], *lists, dtype=LD)
        assert float(np.abs((tp - tm) / (2 * LD(h)) - ref["tg"][:, :, l]).max()) < 1e-7, l
    assert float(np.abs(np.asarray(f64["g"] - ref["g"], np.float64)).max()) < 1e-12
    if k == 1:       # −1[y < b_s] through dy
        b = lists[0][:, 0, 1]
        want = -(y[0] < b[:, None]).astype(np.float64)[:, :, None] * dy[0].transpose(0, 2, 1)
        assert np.array_equal(np.asarray(ref["tg"], np.float64), want)


def test_kink_nan_and_past_the_reference_point_conventions():
    # two boxes that meet at y_0 = 0.5: (−∞, 0.5] × (−∞, 1] and (0.5, 1] × (−∞, 0.3].  At y = (0.5, 0.1) neither strict
    # inequality holds for objective 0: ∂t/∂y_0 = 0 (a step to the right gives −0.2), ∂t/∂y_1 = −0.5
    dec = (np.array([[-np.inf, 0.2, 0.5, 1.0], [-np.inf, 0.3, 0.6, 1.0]]), np.array([4, 4], np.int32),
           np.array([[0, 2, 0, 3], [2, 3, 0, 1]], np.uint16))
    one = pareto.pack_box_lists([dec])
    y = np.array([[[0.5, 0.5 + 2.0 ** -20]], [[0.1, 0.1]]])
    dy = np.zeros((2, 1, 2, 2))
    dy[0, 0, 0, :] = 1.0
    dy[1, 0, 1, :] = 1.0
    for dtype in (np.float64, LD):
        ref = gr.hvi_gradient(y, dy, *one, dtype=dtype)
        assert ref["v"][0] == dtype(0.5) * (dtype(0.3) - dtype(0.1))
        assert ref["g"][0, 0] == 0 and ref["g"][0, 1] == -dtype(0.5)
        assert ref["g"][1, 0] == -(dtype(0.3) - dtype(0.1))
    k, S, d, N = 2, 2, 3, 4
    rng = np.random.default_rng(3)
    _, lists = nr.lists_for(k, [4, 5], rng)
    y = nr.candidates(k, S, N, rng, lo=0.1, hi=0.9)
    dy = rng.normal(size=(k, S, d, N))
    # candidate 1: past the reference point in one objective in every path — exactly 0
    y[1, :, 1] = 1.1
    # candidate 2: a NaN in one path — that path's t and ∂t, the value and every gradient entry are NaN
    y[0, 1, 2] = np.nan
    ref = gr.hvi_gradient(y, dy, *lists, dtype=np.float64)
    assert np.all(ref["g"][1] == 0.0) and ref["v"][1] == 0.0 and np.all(ref["tg"][:, 1] == 0.0)
    assert np.isnan(ref["v"][2]) and np.all(np.isnan(ref["g"][2]))
    assert np.all(np.isnan(ref["tg"][1, 2])) and np.all(np.isfinite(ref["tg"][0, 2])) and np.isnan(ref["t"][1, 2])
    assert np.all(np.isfinite(ref["g"][[0, 1, 3]]))


def test_polish_batch_takes_a_callers_value_and_gradient():
    """−‖x − c‖² with c partly outside the box: the bounded maximiser is clip(c); no device is touched."""
    from optimobo_amd.acquisition import AcquisitionEngine
    eng = AcquisitionEngine.__new__(AcquisitionEngine)
    c = np.array([0.3, 1.4, -0.2])
    lower, upper = np.zeros(3), np.ones(3)
    calls = []

    def f(X):
        X = np.atleast_2d(X)
        calls.append(X.shape[0])
        return 5.0 - np.sum((X - c) ** 2, 1), -2.0 * (X - c)

    starts = np.array([[0.9, 0.1, 0.8], [0.5, 0.5, 0.5], [0.3, 1.0, 0.0]])
    res = eng.polish_batch(starts, lower, upper, value_and_grad=f)
    want = np.clip(c, lower, upper)
    for (x, v), x0 in zip(res, starts):
        assert np.allclose(x, want, atol=1e-6) and v == f(x)[0][0] and v >= f(x0)[0][0]
    assert np.array_equal(res[2][0], starts[2])          # already the maximiser: kept, not moved
    assert max(calls) <= 3
