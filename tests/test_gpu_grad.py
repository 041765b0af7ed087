"""GPU: analytic gradients on the device — omb_posterior_grad and omb_eval_grad against the numpy restatement of
tests/test_grad_reference.py (oracle ExactGP's L and α; validated there against finite differences), their
refusals, and the batched analytic polish (AcquisitionEngine.polish_batch, maximise(polish="analytic" / "auto")).

Tolerance of a gradient entry: |dev − ref| ≤ tol · Σ_i |a_i g_i s_ij|, the sum of the magnitudes of the terms it is
made of (for omb_eval_grad: over objectives and training rows, each weighted by |∂a/∂μ_o| or |∂a/∂σ²_o|).  tol is
1e-9, the exact-EHVI tests' bar, unless TOL below says otherwise with the measured maximum next to it.  Values (μ, σ²,
the acquisition) are bitwise omb_posterior's / omb_eval's.
"""
import os
import warnings

import numpy as np
import pytest
from scipy import linalg

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import test_grad_reference as ref  # noqa: E402
from _de_fixture import oracle_value as _oracle_value  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-9
# (n, d, kernel) → tolerance where 1e-9 is not reached: 4× the measured maximum, never above 1e-6
TOL_POSTERIOR = {}
TOL_EVAL = {}


@pytest.fixture(scope="module")
def ctx():
    from optimobo_amd.device import AcqContext
    c = AcqContext(0)
    yield c
    c.close()


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device="cuda:0")


def upload(ctx, gps):
    for o, g in enumerate(gps):
        Linv = linalg.solve_triangular(g.L, np.eye(len(g.L)), lower=True)
        ctx.set_gp(o, g.X, g.lengthscale, g.variance, g.alpha, Linv, g.kernel)


def bits(t):
    return t.cpu().numpy().view(np.int64)


# ------------------------------------------------------------------------------------------- omb_posterior_grad
@pytest.mark.parametrize("kernel", ["matern52", "rbf"])
@pytest.mark.parametrize("n,d", ref.SHAPES)
def test_posterior_grad(ctx, n, d, kernel):
    gps = [ref.make_gp(n, d, kernel, obj=o) for o in range(2)]
    upload(ctx, gps)
    tol = TOL_POSTERIOR.get((n, d, kernel), TOL)
    worst, bad = 0.0, False
    for N in ref.BATCHES:
        Xc = ref.make_candidates(gps[0], N)                       # row 0 is a training point
        assert np.array_equal(Xc[0], gps[0].X[n // 2])
        mu, var, dmu, dvar = ctx.posterior_grad(dev(Xc), 2)
        mu0, var0 = ctx.posterior(dev(Xc), 2)
        assert np.array_equal(bits(mu), bits(mu0)) and np.array_equal(bits(var), bits(var0))
        dmu, dvar = dmu.cpu().numpy(), dvar.cpu().numpy()
        assert dmu.shape == (2, N, d) and dvar.shape == (2, N, d)
        for o, g in enumerate(gps):
            _, _, rm, rv, sm, sv = ref.posterior_grad(g, Xc)
            em = np.abs(dmu[o] - rm) / np.where(sm > 0, sm, 1.0)
            ev = np.abs(dvar[o] - rv) / np.where(sv > 0, sv, 1.0)
            worst = max(worst, em.max(), ev.max())
            print(f"n={n} d={d} {kernel} N={N} obj={o}: |dev - ref| / sum|terms|: dmu {em.max():.2e} dvar {ev.max():.2e}"
                  f" (row 0, the training point: {em[0].max():.2e} {ev[0].max():.2e})")
            bad = bad or not (np.all(np.abs(dmu[o] - rm) <= tol * sm) and np.all(np.abs(dvar[o] - rv) <= tol * sv))
    print(f"n={n} d={d} {kernel}: worst = {worst:.3e} (tol {tol:g})")
    assert not bad, (worst, tol)


def test_posterior_grad_zero_candidates_and_bad_arguments(ctx):
    from optimobo_amd import _lib
    gps = [ref.make_gp(17, 3, obj=o) for o in range(2)]
    upload(ctx, gps)
    lib, h = ctx.lib, ctx._h
    Xc = dev(ref.make_candidates(gps[0], 7))
    buf = [torch.full((2 * 7 * 3,), -7.5, dtype=torch.float64, device="cuda:0") for _ in range(4)]
    p = [ctypes_ptr(b) for b in buf]
    assert lib.omb_posterior_grad(h, 2, ctypes_ptr(Xc), 0, *p) == _lib.OMB_OK       # N = 0 touches nothing
    assert lib.omb_posterior_grad(h, 2, None, 0, None, None, None, None) == _lib.OMB_OK
    for n_obj in (0, -1, 9):
        assert lib.omb_posterior_grad(h, n_obj, ctypes_ptr(Xc), 7, *p) == _lib.OMB_EINVAL
    for hole in range(5):
        args = [ctypes_ptr(Xc)] + p
        args[hole] = None
        assert lib.omb_posterior_grad(h, 2, args[0], 7, *args[1:]) == _lib.OMB_EINVAL
    assert lib.omb_posterior_grad(h, 2, ctypes_ptr(Xc), -1, *p) == _lib.OMB_EINVAL
    ctx.synchronize()
    assert all(bool((b == -7.5).all()) for b in buf)
    from optimobo_amd.device import AcqContext
    c2 = AcqContext(0)                                               # no GP at all: OMB_ESTATE, as omb_posterior
    assert c2.lib.omb_posterior_grad(c2._h, 1, ctypes_ptr(Xc), 7, *p) == _lib.OMB_ESTATE
    c2.close()


def ctypes_ptr(t):
    import ctypes
    return ctypes.c_void_p(t.data_ptr())


# ------------------------------------------------------------------------------------------- omb_eval_grad
CASES = ref.acquisition_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_eval_grad(ctx, name):
    k, _, partials, plan = CASES[name]
    gps = ref.case_gps(name, k)
    upload(ctx, gps)
    plan(ctx)
    Xc = ref.make_candidates(gps[0], 33, train_point=False)
    vals, grad = ctx.eval_grad(dev(Xc))
    assert np.array_equal(bits(vals), bits(ctx.eval(dev(Xc))))
    with np.errstate(all="ignore"):
        rg, scale = ref.eval_grad(gps, Xc, partials)
    g = grad.cpu().numpy()
    assert np.all(np.isfinite(g)) and np.all(np.isfinite(rg))
    tol = TOL_EVAL.get(name, TOL)
    err = np.abs(g - rg) / np.where(scale > 0, scale, 1.0)
    print(f"{name}: |dev - ref| / sum|terms| = {err.max():.3e} (tol {tol:g}); |grad| up to {np.abs(rg).max():.3g}")
    assert np.all(np.abs(g - rg) <= tol * scale), (err.max(), tol)
    assert (np.abs(g).max(1) > 0).sum() >= 20
    # batch independence: a candidate alone gives bitwise its row of the batch
    for c in (0, 5, 32):
        v1, g1 = ctx.eval_grad(dev(Xc[c:c + 1]))
        assert np.array_equal(bits(v1), bits(vals[c:c + 1])) and np.array_equal(bits(g1[0]), bits(grad[c]))


def test_eval_grad_nan_value_gives_nan_row_only(ctx):
    """A NaN value — EI's sqrt of a negative variance — makes the candidate's whole gradient row NaN and leaves the
    other rows as they are alone.  The negative variance comes from a state whose L⁻¹ is doubled on purpose:
    σ² = σ_f² − 4‖L⁻¹k‖² is below 0 at and near the training points and above it far from them."""
    g = ref.case_gps("ei", 1)[0]
    Linv = linalg.solve_triangular(g.L, np.eye(len(g.L)), lower=True)
    ctx.set_gp(0, g.X, g.lengthscale, g.variance, g.alpha, 2.0 * Linv, g.kernel)
    ctx.plan_ei(0.55, 0.0)
    far = 3.0 + np.random.default_rng(3).uniform(0, 1, (6, 3))
    Xc = np.concatenate([far[:3], g.X[4:5], far[3:]])
    _, var = ctx.posterior(dev(Xc), 1)
    var = var[0].cpu().numpy()
    assert var[3] < 0 and np.all(np.delete(var, 3) > 0)
    vals, grad = ctx.eval_grad(dev(Xc))
    assert bool(torch.isnan(vals[3])) and bool(torch.isnan(grad[3]).all())
    for c in (0, 1, 2, 4, 5, 6):
        v1, g1 = ctx.eval_grad(dev(Xc[c:c + 1]))
        assert bool(torch.isfinite(grad[c]).all())
        assert np.array_equal(bits(v1), bits(vals[c:c + 1])) and np.array_equal(bits(g1[0]), bits(grad[c]))


def _expdec_plan(ctx, k=2):
    rng = np.random.default_rng(5)
    ctx.plan_expdec(rng.normal(size=(32, k)), 1, [], np.full(k, 1.0 / k), np.zeros(k), np.ones(k), 0.4)


def test_eval_grad_refusals(ctx):
    from optimobo_amd import _lib
    from optimobo_amd.device import AcqContext
    gps = ref.case_gps("boxes_k2", 2)
    upload(ctx, gps)
    Xc = dev(ref.make_candidates(gps[0], 7, train_point=False))
    rng = np.random.default_rng(2)
    plans = {
        "Monte-Carlo EHVI": lambda: ctx.plan_ehvi_mc(rng.normal(size=(32, 2)), [1.2, 1.2], 0.3),
        "expected decomposition": lambda: _expdec_plan(ctx),
        "HV-PoI": lambda: ctx.plan_hvpoi(np.array([[[1.2, 1.2], [0.4, 0.5]], [[0.4, 1.2], [0.1, 0.8]]])),
    }
    for what, plan in plans.items():
        plan()
        assert not ctx.plan_has_gradient()
        vals = torch.full((7,), -7.5, dtype=torch.float64, device="cuda:0")
        grad = torch.full((7, 3), -7.5, dtype=torch.float64, device="cuda:0")
        rc = ctx.lib.omb_eval_grad(ctx._h, ctypes_ptr(Xc), 7, ctypes_ptr(vals), ctypes_ptr(grad))
        assert rc == _lib.OMB_EUNSUP and what in ctx.lib.omb_last_error(ctx._h).decode()
        ctx.synchronize()
        assert bool((vals == -7.5).all()) and bool((grad == -7.5).all())
        assert ctx.eval(Xc).shape == (7,)                          # the plan is still set
        with pytest.raises(_lib.OMBError):
            ctx.eval_grad(Xc)
    # null pointers, N < 0, N = 0 with a plan that has a gradient
    ctx.plan_ei(0.55, 0.0)
    assert ctx.plan_has_gradient()
    vals = torch.full((7,), -7.5, dtype=torch.float64, device="cuda:0")
    grad = torch.full((7, 3), -7.5, dtype=torch.float64, device="cuda:0")
    lib, h = ctx.lib, ctx._h
    assert lib.omb_eval_grad(h, None, 7, ctypes_ptr(vals), ctypes_ptr(grad)) == _lib.OMB_EINVAL
    assert lib.omb_eval_grad(h, ctypes_ptr(Xc), 7, None, ctypes_ptr(grad)) == _lib.OMB_EINVAL
    assert lib.omb_eval_grad(h, ctypes_ptr(Xc), 7, ctypes_ptr(vals), None) == _lib.OMB_EINVAL
    assert lib.omb_eval_grad(h, ctypes_ptr(Xc), -1, ctypes_ptr(vals), ctypes_ptr(grad)) == _lib.OMB_EINVAL
    assert lib.omb_eval_grad(h, ctypes_ptr(Xc), 0, ctypes_ptr(vals), ctypes_ptr(grad)) == _lib.OMB_OK
    ctx.synchronize()
    assert bool((vals == -7.5).all()) and bool((grad == -7.5).all())
    # no plan at all: OMB_ESTATE, as omb_eval
    c2 = AcqContext(0)
    upload(c2, gps)
    rc = c2.lib.omb_eval_grad(c2._h, ctypes_ptr(Xc), 7, ctypes_ptr(vals), ctypes_ptr(grad))
    assert rc == _lib.OMB_ESTATE and not c2.plan_has_gradient()
    c2.close()


# ------------------------------------------------------------------------------------------- the analytic polish
def _de_cases():
    z = np.load(os.path.join(GOLDEN, "de_proposals.npz"), allow_pickle=False)
    return [c for c in range(int(z["n_cases"])) if str(z[f"c{c}_kind"]) in ("ehvi", "ei")]


@pytest.mark.parametrize("c", _de_cases())
def test_analytic_polish_reaches_de_proposal(c):
    """maximise(polish="analytic", starts=16) against scipy DE's proposal on the golden surrogates: the bar
    test_gpu_polish.py holds the stencil polish to."""
    from optimobo_amd.acquisition import AcquisitionEngine
    from optimobo_amd.gp import GPState
    z = np.load(os.path.join(GOLDEN, "de_proposals.npz"), allow_pickle=False)
    k = f"c{c}"
    kind = str(z[f"{k}_kind"])
    X, Y, ls, var = z[f"{k}_X"], z[f"{k}_Y"], z[f"{k}_ls"], z[f"{k}_variances"]
    xl, xu = z[f"{k}_xl"], z[f"{k}_xu"]
    if kind == "ei":
        eng = AcquisitionEngine(0).load_models([GPState(X, z[f"{k}_yagg"], ls, float(z[f"{k}_agg_variance"]))])
        eng.plan_ei(float(z[f"{k}_best"]), 0.0)
    else:
        eng = AcquisitionEngine(0).load_models([GPState(X, Y[:, o], ls, float(var[o])) for o in range(Y.shape[1])])
        eng.plan_ehvi(z[f"{k}_r"], z[f"{k}_pf"], z[f"{k}_cache"], mode="reference")
    assert eng.has_gradient()
    x, v = eng.maximise(None, xl, xu, n_candidates=1 << 16, seed=c, polish="analytic", starts=16)
    v_de = float(z[f"{k}_value_de"])
    print(f"case {c} ({kind}, d={len(xl)}): analytic polish {v!r} vs DE {v_de!r}: (v - v_DE)/|v_DE| = {(v - v_de) / abs(v_de):.3e}")
    assert np.all(x >= xl) and np.all(x <= xu)
    assert v == float(eng.ctx.eval(dev(x[None, :])).cpu().numpy()[0])          # the value is omb_eval at x
    ref_v = _oracle_value(z, k, kind, x)
    assert abs(ref_v - v) <= 1e-6 * abs(ref_v) + 1e-14
    assert v >= v_de - 1e-6 * abs(v_de), (kind, x, v, z[f"{k}_x_de"], v_de)
    eng.ctx.close()


def _small_engine(k, n=24, d=4):
    from optimobo_amd.acquisition import AcquisitionEngine
    from optimobo_amd.gp import GPState
    gps = ref.acq_gps(k, n=n, d=d)
    eng = AcquisitionEngine(0).load_models([GPState(g.X, g.y[:, 0], g.lengthscale, g.variance) for g in gps])
    return eng, gps


def test_analytic_polish_k4_exact_ehvi_not_worse_than_stencil():
    eng, gps = _small_engine(4)
    pf, r = ref.front(4, 6)
    eng.plan_ehvi_exact(r, pf)
    assert eng.has_gradient()
    lo, hi = np.zeros(4), np.ones(4)
    starts = eng._starts(None, lo, hi, 1 << 14, seed=3, k=8)
    assert len(starts) >= 4
    stencil = [eng.polish(None, x, v, lo, hi) for x, v in starts]
    analytic = eng.polish_batch(starts, lo, hi)
    vs, va = max(v for _, v in stencil), max(v for _, v in analytic)
    print(f"k=4 exact EHVI, {len(starts)} starts: best stencil {vs!r}, best analytic {va!r}, (va - vs)/|vs| = {(va - vs) / abs(vs):.3e}")
    for (x0, v0), (x1, v1) in zip(starts, analytic):
        assert v1 >= v0 and np.all(x1 >= lo) and np.all(x1 <= hi)
        assert v1 == float(eng.ctx.eval(dev(x1[None, :])).cpu().numpy()[0])
    assert va >= vs - 1e-6 * abs(vs)
    # through maximise
    x, v = eng.maximise(None, lo, hi, n_candidates=1 << 14, seed=3, polish="analytic", starts=8)
    assert v >= vs - 1e-6 * abs(vs) and np.all(x >= lo) and np.all(x <= hi)
    assert v == float(eng.ctx.eval(dev(x[None, :])).cpu().numpy()[0])
    vg, gg = eng.value_and_grad(x[None, :])
    assert vg.shape == (1,) and gg.shape == (1, 4) and vg[0] == v
    eng.ctx.close()


def test_polish_modes_on_a_plan_without_gradient():
    from optimobo_amd import scalarisations as sc
    eng, gps = _small_engine(2)
    cache = np.random.default_rng(1).normal(size=(32, 2))
    eng.plan_expected_decomposition(np.array([0.5, 0.5]), sc.Tchebicheff([0.0, 0.0], [1.0, 1.0]), 0.6, cache)
    assert not eng.has_gradient()
    lo, hi = np.zeros(4), np.ones(4)
    with pytest.raises(ValueError):
        eng.maximise(None, lo, hi, n_candidates=1 << 12, seed=1, polish="analytic")
    with pytest.raises(ValueError):
        eng.maximise(None, lo, hi, n_candidates=1 << 12, seed=1, polish="newton")
    xa, va = eng.maximise(None, lo, hi, n_candidates=1 << 12, seed=1, polish="auto")
    xt, vt = eng.maximise(None, lo, hi, n_candidates=1 << 12, seed=1, polish=True)
    assert np.array_equal(xa, xt) and va == vt
    # a callable acquisition has no device gradient either
    eng.plan_ei(0.5, 0.0)
    with pytest.raises(ValueError):
        eng.maximise(lambda Xd: eng.ctx.eval(Xd), lo, hi, n_candidates=1 << 12, seed=1, polish="analytic")
    eng.ctx.close()


def test_solve_textbook_with_auto_polish():
    import optimobo_amd.algorithms.optimisers as opti
    from optimobo_amd.problem import ElementwiseProblem

    class MyProblem(ElementwiseProblem):        # the README's problem
        def __init__(self):
            super().__init__(n_var=2, n_obj=2, xl=np.array([-2, -2]), xu=np.array([2, 2]))

        def _evaluate(self, x, out, *args, **kwargs):
            out["F"] = [100 * (x[0] ** 2 + x[1] ** 2), (x[0] - 1) ** 2 + x[1] ** 2]

    np.random.seed(1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        opt = opti.MultiSurrogateOptimiser(MyProblem(), [0, 0], [700, 12], mode="textbook", n_candidates=4096, seed=2,
                                           polish="auto", starts=8)
        out = opt.solve(budget=3, n_init_samples=8)
    assert out.ysample.shape == (11, 2) and out.Xsample.shape == (11, 2)
    assert np.all(np.abs(out.Xsample) <= 2 + 1e-12)
