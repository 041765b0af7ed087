"""GPU: omb_gp_append (conditioning an installed GP state in place), AcquisitionEngine.condition and the drivers'
``batch_size`` — against oracle.gp.ExactGP refactorised on all points (cases, oracle states and the numpy
restatement of the update: tests/test_append_host.py, which also shows the cases are ones where the update itself
is accurate to 1e-5 of the tolerance used here).

Tolerances: the project's posterior bar (1e-6 relative, floors 1e-7·σ_f for μ and 1e-9·σ_f² for σ²) for
the posterior and for each appended point's predictive mean and δ²; the parity suites' own bars for the other
consumers of the state (kernel block 1e-12, covariance 1e-6 / 1e-9·σ_f², gradients 1e-9 of the summed term
magnitudes, the arg-max index identical).  Bitwise where stated.
"""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
# the shared cases are read-only arrays; torch warns when it wraps one on its way to the device
pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]

import test_append_host as ah  # noqa: E402
import test_grad_reference as gref  # noqa: E402
from optimobo_amd import _lib  # noqa: E402
from oracle import gp as ogp  # noqa: E402

VAR = ah.VARIANCE
GPU_CASES = ah.HOST_CASES + ah.EDGE_CASES + [(16, 8, 1, 0.0, "matern52"), (64, 9, 2, 0.0, "matern52"), (128, 8, 1, 0.0, "matern52"),
                             (129, 3, 1, 0.0, "matern52"), (12, 100, 2, 0.0, "matern52")]


@pytest.fixture(scope="module")
def ctx():
    from optimobo_amd.device import AcqContext
    c = AcqContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx2():
    from optimobo_amd.device import AcqContext
    c = AcqContext(0)
    yield c
    c.close()


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device="cuda:0")


def bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def install(ctx, case, how, m=None, obj=0):
    """The first m (default n) points of the case as objective obj: a host GPState, or the device fit.  Returns the
    noise to append with (the case's, plus the device fit's jitter)."""
    from optimobo_amd.gp import GPState
    n, d, q, noise, kernel = case
    X, y, ls, _ = ah.make_case(*case)
    m = n if m is None else m
    if how == "host":
        ctx.set_gp_state(obj, GPState(X[:m], y[:m], ls, VAR, kernel=kernel, noise=noise))
        return noise
    return noise + ctx.gp_fit_state(obj, X[:m], y[:m], ls, VAR, noise, kernel)


def posterior1(ctx, Xc):
    mu, var = ctx.posterior(dev(Xc), n_obj=1)
    return mu[0].cpu().numpy(), var[0].cpu().numpy()


def assert_moments(mu, var, mu_ref, var_ref):
    print(f"  worst error = {ah.tolerance_ratio(mu, var, mu_ref, var_ref, VAR):.2e} of the tolerance")
    np.testing.assert_allclose(mu, mu_ref, rtol=1e-6, atol=1e-7 * np.sqrt(VAR))
    np.testing.assert_allclose(var, var_ref, rtol=1e-6, atol=1e-9 * VAR)


# ----------------------------------------------------------------------------- parity
@pytest.mark.parametrize("how", ["host", "fit"])
@pytest.mark.parametrize("case", GPU_CASES, ids=lambda c: f"n{c[0]}-d{c[1]}-q{c[2]}-{c[4]}")
def test_append_matches_refit(ctx, case, how):
    n, d, q, noise, kernel = case
    X, y, ls, Xc = ah.make_case(*case)
    nz = install(ctx, case, how)
    mu_out, d2 = ctx.gp_append(0, X[n:], y[n:], nz)
    assert ctx.gp_info[0]["n"] == n + q
    mu, var = posterior1(ctx, Xc)
    assert_moments(mu, var, *ah.oracle_refit(*case))
    seq_mu, seq_d2 = ah.oracle_sequential(*case)
    np.testing.assert_allclose(mu_out, seq_mu, rtol=1e-6, atol=1e-7 * np.sqrt(VAR))
    np.testing.assert_allclose(d2, seq_d2 + (nz - noise), rtol=1e-6, atol=1e-9 * VAR)


# ----------------------------------------------------------------------------- every consumer of the state
@pytest.mark.parametrize("case", [ah.HOST_CASES[2], ah.HOST_CASES[3], (1023, 6, 2, 0.0, "matern52")],
                         ids=lambda c: f"n{c[0]}-d{c[1]}-q{c[2]}-{c[4]}")
def test_every_consumer_sees_the_grown_state(ctx, ctx2, case):
    """Appended (ctx) against the same calls on a context that received the refit state (ctx2)."""
    n, d, q, noise, kernel = case
    X, y, ls, _ = ah.make_case(*case)
    rng = np.random.default_rng(5)
    Xc = dev(rng.uniform(0.0, 1.0, (40, d)))
    Xbig = dev(rng.uniform(0.0, 1.0, (4096, d)))
    best = float(np.min(y))
    install(ctx, case, "host")
    ctx.plan_ei(best, 0.0)                          # set before the append: it must survive it
    ctx.gp_append(0, X[n:], y[n:], noise)
    install(ctx2, case, "host", m=n + q)
    ctx2.plan_ei(best, 0.0)
    g = ah.oracle_gp(*case, n + q)

    np.testing.assert_allclose(ctx.kernel_block(0, Xc).cpu().numpy(), ctx2.kernel_block(0, Xc).cpu().numpy(),
                               rtol=1e-12, atol=1e-14)
    mu_a, cov_a = ctx.posterior_cov(0, Xc)
    mu_b, cov_b = ctx2.posterior_cov(0, Xc)
    np.testing.assert_allclose(mu_a.cpu().numpy(), mu_b.cpu().numpy(), rtol=1e-6, atol=1e-7 * np.sqrt(VAR))
    np.testing.assert_allclose(cov_a.cpu().numpy(), cov_b.cpu().numpy(), rtol=1e-6, atol=1e-9 * VAR)
    _, _, dmu_a, dvar_a = ctx.posterior_grad(Xc, 1)
    _, _, dmu_b, dvar_b = ctx2.posterior_grad(Xc, 1)
    _, _, _, _, sm, sv = gref.posterior_grad(g, Xc.cpu().numpy())
    em = np.abs(dmu_a[0].cpu().numpy() - dmu_b[0].cpu().numpy()) / np.where(sm > 0, sm, 1.0)
    ev = np.abs(dvar_a[0].cpu().numpy() - dvar_b[0].cpu().numpy()) / np.where(sv > 0, sv, 1.0)
    print(f"  gradients: |appended - refit| / sum|terms|: dmu {em.max():.2e} dvar {ev.max():.2e}")
    assert em.max() <= 1e-9 and ev.max() <= 1e-9
    pa = ctx.eval_argmax(Xbig).cpu().numpy()
    pb = ctx2.eval_argmax(Xbig).cpu().numpy()
    assert pa[1] == pb[1] and pa[1] >= 0
    np.testing.assert_allclose(pa[0], pb[0], rtol=1e-5, atol=1e-9)


# ----------------------------------------------------------------------------- the Kriging believer
@pytest.mark.parametrize("case", [ah.HOST_CASES[1], (129, 3, 1, 0.0, "matern52"), (1023, 6, 2, 0.0, "matern52")],
                         ids=lambda c: f"n{c[0]}-d{c[1]}-q{c[2]}")
def test_believer_keeps_the_mean_and_shrinks_the_variance(ctx, case):
    n, d, q, noise, kernel = case
    X, y, ls, Xc = ah.make_case(*case)
    install(ctx, case, "host")
    mu0, var0 = posterior1(ctx, Xc)
    mu_pt, _ = posterior1(ctx, X[n:])
    mu_out, d2 = ctx.gp_append(0, X[n:], None, noise)
    mu1, var1 = posterior1(ctx, Xc)
    print(f"  |mu change| {np.abs(mu1 - mu0).max():.2e}  max var growth {np.max(var1 - var0):.2e}")
    assert np.abs(mu1 - mu0).max() <= 1e-12 * np.sqrt(VAR)
    assert np.all(var1 <= var0 + 1e-12 * VAR)
    _, var_pt = posterior1(ctx, X[n:])
    assert np.all(var_pt <= 1e-6 * VAR), var_pt
    np.testing.assert_allclose(mu_out[0], mu_pt[0], rtol=1e-6, atol=1e-7 * np.sqrt(VAR))
    assert np.all(d2 > 0)


# ----------------------------------------------------------------------------- sequencing and determinism
@pytest.mark.parametrize("case", [(15, 2, 3, 0.0, "matern52"), (63, 6, 3, 0.0, "matern52"),
                                  (1023, 6, 3, 0.0, "matern52")], ids=lambda c: f"n{c[0]}")
def test_one_call_equals_single_calls_bitwise(ctx, case):
    n, d, q, noise, kernel = case
    X, y, ls, Xc = ah.make_case(*case)
    runs = []
    for split in (False, True, False):
        install(ctx, case, "host")
        if split:
            outs = [ctx.gp_append(0, X[n + j:n + j + 1], y[n + j:n + j + 1], noise) for j in range(q)]
            mu_out, d2 = np.concatenate([o[0] for o in outs]), np.concatenate([o[1] for o in outs])
        else:
            mu_out, d2 = ctx.gp_append(0, X[n:], y[n:], noise)
        mu, var = ctx.posterior(dev(Xc), n_obj=1)
        K = ctx.kernel_block(0, dev(Xc[:8]))
        runs.append((bits(mu_out), bits(d2), bits(mu), bits(var), bits(K)))
    for a, b, c in zip(*runs):
        assert np.array_equal(a, b), "q points in one call differ from q calls of one point"
        assert np.array_equal(a, c), "two identical runs differ"


# ----------------------------------------------------------------------------- refusals
def _rc(ctx, obj, q, Xnew, noise=0.0):
    Xd = dev(Xnew)
    ctx._stream()
    return ctx.lib.omb_gp_append(ctx._h, obj, q, Xd.data_ptr() or None, None, float(noise), None, None)


def test_refusals(ctx):
    case = ah.HOST_CASES[0]
    n, d, q, noise, kernel = case
    X, y, ls, Xc = ah.make_case(*case)
    install(ctx, case, "host")
    before = posterior1(ctx, Xc)
    assert _rc(ctx, 7, 1, X[n:n + 1]) == _lib.OMB_ESTATE              # objective 7 was never set
    assert _rc(ctx, -1, 1, X[n:n + 1]) == _lib.OMB_ESTATE
    assert _rc(ctx, 0, 0, X[n:n + 1]) == _lib.OMB_EINVAL
    assert ctx.lib.omb_gp_append(ctx._h, 0, 1, None, None, 0.0, None, None) == _lib.OMB_EINVAL
    assert _rc(ctx, 0, 1, X[n:n + 1], noise=-1.0) == _lib.OMB_EINVAL
    assert _rc(ctx, 0, 1, X[n:n + 1], noise=float("nan")) == _lib.OMB_EINVAL
    assert _rc(ctx, 0, 1, X[n:n + 1], noise=float("inf")) == _lib.OMB_EINVAL
    with pytest.raises(_lib.OMBError) as e:
        ctx.gp_append(0, np.zeros((0, d)))
    assert e.value.code == _lib.OMB_EINVAL
    # n + q = 16385: refused from the arguments alone (one row of input stands behind q: nothing may be read)
    free0 = torch.cuda.mem_get_info()[0]
    assert _rc(ctx, 0, _lib.MAX_TRAIN_DENSE + 1 - n, X[n:n + 1]) == _lib.OMB_EUNSUP
    assert torch.cuda.mem_get_info()[0] >= free0 - (1 << 20)
    after = posterior1(ctx, Xc)
    assert np.array_equal(bits(before[0]), bits(after[0])) and np.array_equal(bits(before[1]), bits(after[1]))
    assert ctx.gp_info[0]["n"] == n


@pytest.mark.parametrize("case", [ah.HOST_CASES[0], ah.HOST_CASES[1], (129, 3, 1, 0.0, "matern52")],
                         ids=lambda c: f"n{c[0]}")
def test_duplicate_of_a_training_row(ctx, case):
    """δ² of an exact duplicate at noise 0 is the jitter minus rounding: either it succeeds with δ² > 0, or it is
    OMB_ENOTPD and the installed state is bitwise what it was."""
    n, d, q, noise, kernel = case
    X, y, ls, Xc = ah.make_case(*case)
    install(ctx, case, "host")
    before = ctx.posterior(dev(Xc), n_obj=1)
    dup = np.vstack((X[n:n + 1], X[n // 2:n // 2 + 1]))          # a good point first: all or nothing
    try:
        _, d2 = ctx.gp_append(0, dup, None, 0.0)
    except _lib.OMBError as e:
        assert e.code == _lib.OMB_ENOTPD and "point 2" in str(e)
        after = ctx.posterior(dev(Xc), n_obj=1)
        assert np.array_equal(bits(before[0]), bits(after[0])) and np.array_equal(bits(before[1]), bits(after[1]))
        assert ctx.gp_info[0]["n"] == n
        print("  duplicate refused (OMB_ENOTPD), state unchanged")
    else:
        assert np.all(d2 > 0) and ctx.gp_info[0]["n"] == n + 2
        mu, var = posterior1(ctx, Xc)
        assert np.all(np.isfinite(mu)) and np.all(np.isfinite(var))
        print(f"  duplicate accepted, delta^2 = {d2[1]:.3e}")


# ----------------------------------------------------------------------------- engine and drivers
def test_condition_then_load_models_restores_the_fit():
    from optimobo_amd.acquisition import engine_for
    from optimobo_amd.gp import GPState
    case = ah.HOST_CASES[1]
    n, d, q, noise, kernel = case
    X, y, ls, Xc = ah.make_case(*case)
    models = [GPState(X[:n], y[:n], ls, VAR, kernel=kernel), GPState(X[:n], np.cos(y[:n]), ls, 0.9, kernel=kernel)]
    eng = engine_for(models)
    mu0, var0 = eng.posterior(dev(Xc))
    mus = eng.condition(X[n:])
    assert mus.shape == (q, 2) and eng.ctx.gp_info[0]["n"] == n + q
    mu1, var1 = eng.posterior(dev(Xc))
    assert np.abs((mu1 - mu0).cpu().numpy()).max() <= 1e-12 * np.sqrt(VAR)
    assert bool((var1 < var0).any())
    eng2 = engine_for(models)                      # the same objects: stale, so uploaded again
    assert eng2 is eng and eng.ctx.gp_info[0]["n"] == n
    mu2, var2 = eng.posterior(dev(Xc))
    assert np.array_equal(bits(mu2), bits(mu0)) and np.array_equal(bits(var2), bits(var0))
    # true values: every objective conditioned on its own column
    Y = np.column_stack((y[n:], np.cos(y[n:])))
    eng.condition(X[n:], Y)
    mu3, var3 = eng.posterior(dev(Xc))
    for o, vv in enumerate((VAR, 0.9)):
        m, v = ogp.ExactGP(X, np.append(models[o].y[:, 0], Y[:, o]), ls, vv, kernel=kernel).predict(Xc)
        np.testing.assert_allclose(mu3[o].cpu().numpy(), m[:, 0], rtol=1e-6, atol=1e-7 * np.sqrt(vv))
        np.testing.assert_allclose(var3[o].cpu().numpy(), v[:, 0], rtol=1e-6, atol=1e-9 * vv)
    engine_for(models)


def _readme_state(golden_dir):
    """tests/golden/append_notpd_state.npz: the surrogates of a README-run iteration (n = 20; objective 1 fitted to
    σ_f² = 2.1e9 with ℓ ≈ 630 on a 4 × 4 box, so K is σ_f² times a matrix of nearly equal entries), two believer
    picks of that iteration and the third, on which omb_gp_append returned OMB_ENOTPD on an MI355X: the posterior
    variance is ~1e-12 of σ_f² there, below the rounding of vᵀv."""
    z = np.load(os.path.join(golden_dir, "append_notpd_state.npz"), allow_pickle=False)
    return z["X"], z["Y"], z["ls"], z["var"], np.vstack((z["earlier"], z["xnew"]))


def test_not_positive_definite_is_all_or_nothing(ctx, golden_dir):
    """Either every δ² is positive and the state grows, or the call is OMB_ENOTPD naming the point and the installed
    state — though the points before it were already in the bordered copy — is bitwise what it was."""
    X, Y, ls, var, Xnew = _readme_state(golden_dir)
    rng = np.random.default_rng(3)
    Xc = rng.uniform(-2.0, 2.0, (64, 2))
    jit = ctx.gp_fit_state(0, X, Y[:, 1], ls[1], var[1], 0.0, "matern52")
    before = ctx.posterior(dev(Xc), n_obj=1)
    try:
        _, d2 = ctx.gp_append(0, Xnew, None, jit)
    except _lib.OMBError as e:
        assert e.code == _lib.OMB_ENOTPD and any(f"point {k}:" in str(e) for k in (1, 2, 3)), str(e)
        after = ctx.posterior(dev(Xc), n_obj=1)
        assert np.array_equal(bits(before[0]), bits(after[0])) and np.array_equal(bits(before[1]), bits(after[1]))
        assert ctx.gp_info[0]["n"] == len(X)
        print(f"  refused ({str(e).split(':')[2].strip()}), state unchanged")
        _, d2 = ctx.gp_append(0, Xnew, None, jit + var[1] * 1e-6)      # jitchol's first step on the new points
        assert np.all(d2 > 0)
    else:
        print(f"  accepted, delta^2 = {d2}")
        assert np.all(d2 > 0)
    assert ctx.gp_info[0]["n"] == len(X) + 3


def test_condition_escalates_the_jitter_where_the_update_needs_it(golden_dir):
    """The same iteration through the engine: condition succeeds on every pick, with jitchol's escalation on the new
    point where the update is OMB_ENOTPD at the state's own noise (condition_jitter says how much); the mean stays."""
    from optimobo_amd.acquisition import engine_for
    from optimobo_amd.gp import GPRegression, Matern52
    X, Y, ls, var, Xnew = _readme_state(golden_dir)
    models = [GPRegression(X, Y[:, o:o + 1], Matern52(2, variance=var[o], lengthscale=ls[o], ARD=True), noise_var=0.0,
                           device_fit=True) for o in range(2)]
    Xc = dev(np.random.default_rng(3).uniform(-2.0, 2.0, (64, 2)))
    eng = engine_for(models)
    mu0, _ = eng.posterior(Xc)
    used = []
    for x in Xnew:
        mus = eng.condition(x[None, :])
        assert mus.shape == (1, 2) and np.all(np.isfinite(mus))
        used.append(eng.condition_jitter)
        assert used[-1] in [0.0] + [v * 1e-6 * 10.0 ** t for v in var for t in range(5)]
    print(f"  condition_jitter per pick: {used}")
    assert eng.ctx.gp_info[0]["n"] == eng.ctx.gp_info[1]["n"] == len(X) + 3
    mu1, var1 = eng.posterior(Xc)
    assert np.all(np.isfinite(var1.cpu().numpy()))
    # believer: ζ = 0 whatever the jitter, so α keeps its bits and the new rows weigh exactly 0
    assert np.all(np.abs((mu1 - mu0).cpu().numpy()) <= 1e-12 * np.sqrt(var)[:, None])
    engine_for(models)
    assert eng.ctx.gp_info[0]["n"] == len(X)


def _myproblem():
    from optimobo_amd.problem import ElementwiseProblem

    class MyProblem(ElementwiseProblem):        # the 2-objective problem of tests/test_gpu_surface.py
        def __init__(self):
            super().__init__(n_var=2, n_obj=2, xl=np.array([-2, -2]), xu=np.array([2, 2]))

        def _evaluate(self, x, out, *args, **kwargs):
            out["F"] = [100 * (x[0] ** 2 + x[1] ** 2), (x[0] - 1) ** 2 + x[1] ** 2]
    return MyProblem()


def _check_batches(out, n_init, budget, q):
    assert out.Xsample.shape == (n_init + budget, 2) and out.ysample.shape == (n_init + budget, 2)
    assert len(out.hypervolume_convergence) == -(-budget // q)
    assert np.all(np.abs(out.Xsample) <= 2 + 1e-12)
    for s in range(n_init, n_init + budget, q):
        B = out.Xsample[s:min(s + q, n_init + budget)]
        for i in range(len(B)):
            for j in range(i + 1, len(B)):
                assert np.max(np.abs(B[i] - B[j])) > 1e-9, (s, B)


@pytest.mark.parametrize("acq", ["ehvi", "tch"])
def test_multi_surrogate_batches(acq):
    import optimobo_amd.algorithms.optimisers as opti
    import optimobo_amd.scalarisations as sc
    np.random.seed(21)
    opt = opti.MultiSurrogateOptimiser(_myproblem(), [0, 0], [700, 12], n_candidates=4096, seed=2, batch_size=3)
    fn = None if acq == "ehvi" else sc.Tchebicheff([0, 0], [700, 12])
    out = opt.solve(budget=7, n_init_samples=8, **({} if fn is None else dict(sample_exponent=3, acquisition_func=fn)))
    _check_batches(out, 8, 7, 3)


def test_mono_surrogate_batches():
    import optimobo_amd.algorithms.optimisers as opti
    import optimobo_amd.scalarisations as sc
    np.random.seed(22)
    opt = opti.MonoSurrogateOptimiser(_myproblem(), [0, 0], [700, 12], n_candidates=2048, seed=3, batch_size=3)
    out = opt.solve(sc.Tchebicheff([0, 0], [700, 12]), budget=7, n_init_samples=8)
    _check_batches(out, 8, 7, 3)


def test_batch_size_one_is_the_earlier_run_bitwise(golden_dir):
    """Xsample of the runs recorded before ``batch_size`` existed (tests/golden/batch1_solve.npz)."""
    import optimobo_amd.algorithms.optimisers as opti
    import optimobo_amd.scalarisations as sc
    z = np.load(os.path.join(golden_dir, "batch1_solve.npz"), allow_pickle=False)
    np.random.seed(11)
    opt = opti.MultiSurrogateOptimiser(_myproblem(), [0, 0], [700, 12], n_candidates=4096, seed=2, batch_size=1)
    X = opt.solve(budget=3, n_init_samples=8).Xsample
    assert np.array_equal(bits(X), bits(z["multi_X"]))
    np.random.seed(12)
    opt = opti.MonoSurrogateOptimiser(_myproblem(), [0, 0], [700, 12], n_candidates=2048, seed=3, batch_size=1)
    X = opt.solve(sc.Tchebicheff([0, 0], [700, 12]), budget=3, n_init_samples=8).Xsample
    assert np.array_equal(bits(X), bits(z["mono_X"]))


def _batched_and_pof_runs():
    """Xsample and hypervolume_convergence of one run of each loop shape beyond batch 1: believer batches and
    constraints="pof", on both drivers.  Budget 4 in batches of 3 (one full, one truncated) or 2."""
    import _constraints_fixture as cf
    import optimobo_amd.algorithms.optimisers as opti
    import optimobo_amd.scalarisations as sc
    kw = dict(n_candidates=2048)
    pof = dict(constraints="pof", mode="textbook", seed=1, batch_size=2, **kw)
    runs = {}
    np.random.seed(21)
    opt = opti.MultiSurrogateOptimiser(_myproblem(), [0, 0], [700, 12], seed=2, batch_size=3, **kw)
    runs["multi_q3"] = opt.solve(budget=4, n_init_samples=8)
    np.random.seed(31)
    opt = opti.MultiSurrogateOptimiser(cf.driver_problem(), [0, 0], [2.5, 2.0], **pof)
    runs["multi_pof_q2"] = opt.solve(budget=4, n_init_samples=8)
    np.random.seed(22)
    opt = opti.MonoSurrogateOptimiser(_myproblem(), [0, 0], [700, 12], seed=3, batch_size=3, **kw)
    runs["mono_q3"] = opt.solve(sc.Tchebicheff([0, 0], [700, 12]), budget=4, n_init_samples=8)
    np.random.seed(33)
    opt = opti.MonoSurrogateOptimiser(cf.driver_problem(), [0, 0], [2.5, 2.0], **pof)
    runs["mono_pof_q2"] = opt.solve(sc.Tchebicheff([0, 0], [2.5, 2.0]), budget=4, n_init_samples=8)
    out = {}
    for name, res in runs.items():
        out[name + "_X"] = res.Xsample
        out[name + "_hv"] = np.asarray(res.hypervolume_convergence, np.float64)
    return out


def test_batched_and_pof_runs_are_the_earlier_runs_bitwise(golden_dir):
    """The runs recorded while ``solve`` still had a loop of its own for batches and one for constraints="pof"
    (tests/golden/batched_solve.npz; OMB_TEST_RECORD=<file> writes this run's arrays there before comparing)."""
    z = np.load(os.path.join(golden_dir, "batched_solve.npz"), allow_pickle=False)
    got = _batched_and_pof_runs()
    if os.environ.get("OMB_TEST_RECORD"):
        np.savez(os.environ["OMB_TEST_RECORD"], **got)
    assert sorted(got) == sorted(z.files)
    for name in z.files:
        assert got[name].shape == z[name].shape and np.array_equal(bits(got[name]), bits(z[name])), name


def test_batch_size_is_checked():
    import optimobo_amd.algorithms.optimisers as opti
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            opti.MultiSurrogateOptimiser(_myproblem(), [0, 0], [700, 12], batch_size=bad)
