"""GPU: the probability-of-feasibility weight as a modifier of any plan — omb_feasibility, omb_plan_constraints, the
constrained fused chain and its gradient, the believer on constraint models, and the drivers' constraints="pof".

Surrogates and the numpy restatements come from tests/_constraints_fixture.py (validated without a device by
tests/test_constraints_host.py).  Every case first asserts, on the oracle's posterior, that its weight is neither all
0 nor all 1 (fixture.assert_bands): a condition on the inputs, not a measurement.

Gradient tolerance: tests/test_gpu_grad.py's — |dev − ref| ≤ tol · Σ|terms|, tol 1e-9 unless TOL_EVAL names the case
with 4× its measured maximum (never above 1e-6) and the measured value beside it.
"""
import ctypes

import numpy as np
import pytest
from scipy import linalg

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _constraints_fixture as cf  # noqa: E402
import test_grad_reference as ref  # noqa: E402
from oracle import acquisition as oacq  # noqa: E402
from oracle import pareto as opar  # noqa: E402

EPS = cf.POF_EPS
TOL = 1e-9
TOL_EVAL = {}          # (case name, c) → tolerance, by tests/test_gpu_grad.py's rule
N_GEO = 40             # observations the plans' fronts are built from


@pytest.fixture(scope="module")
def ctx():
    from optimobo_amd.device import AcqContext
    c = AcqContext(0)
    yield c
    for what, v in (("posterior_all_var", 0), ("posterior_mean_kernel", 1), ("fused_chain", 0)):
        c.debug_set(what, v)
    c.close()


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device="cuda:0")


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def host(t):
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same(a, b):
    """Bit for bit, NaN matching NaN."""
    a, b = np.asarray(a), np.asarray(b)
    na = np.isnan(a)
    return a.shape == b.shape and np.array_equal(na, np.isnan(b)) and np.array_equal(bits(a[~na]), bits(b[~na]))


_STATES = {}


def set_slots(ctx, gps):
    """gps [(X, y, ℓ, σ_f²)] into context slots 0..len−1."""
    from optimobo_amd.gp import GPState
    for o, g in enumerate(gps):
        key = (id(g[0]), id(g[1]))
        if key not in _STATES:
            _STATES[key] = (g, GPState(*g))
        ctx.set_gp_state(o, _STATES[key][1])


@pytest.fixture(scope="module")
def base():
    """n = 130, d = 6 (counter ring, n_var ≤ 8): four objectives and seven constraints on the same inputs."""
    gps, Y, Xc, mu, var = cf.problem(130, 6, 130006, 4, 7)
    return dict(obj=gps[:4], con=gps[4:], Y=Y[:N_GEO], Xc=Xc, mu=mu, var=var)


def ref_cache():
    cache = np.random.default_rng(11).normal(size=(64, 2))
    cache[:, 1] = 0.6 * cache[:, 0] + 0.8 * cache[:, 1]     # reference mode uses Cov(cache)01 as a σ: keep it > 0
    return cache


def plans(ctx, Y):
    """(name, k, set_plan()) of every plan kind."""
    from optimobo_amd import pareto
    rng = np.random.default_rng(0)
    pf2, r2 = opar.calc_pf(Y[:, :2]), Y[:, :2].max(0) + 0.1
    s00, s01 = oacq.cache_stats(ref_cache())
    stripes = pareto.stripes_2d(pf2)
    r3 = Y[:, :3].max(0) + 0.2
    cache3 = rng.standard_normal((32, 3))
    hv_mc = opar.hypervolume(opar.calc_pf(Y[:2, :3]), r3)     # an early, small front: many candidates score above 0
    box = {k: pareto.box_decomposition(opar.calc_pf(Y[:12, :k]), Y[:, :k].max(0) + 0.2) for k in (2, 3, 4)}
    cells = opar.decompose_into_cells(pf2, Y[:, :2].min(0), Y[:, :2].max(0))
    w3 = np.array([0.2, 0.5, 0.3])
    out = [(f"ehvi2d-{m}", 2, lambda m=m: ctx.plan_ehvi2d(stripes, r2, s00, s01, mode=m))
           for m in ("reference", "textbook", "sigma")]
    out.append(("ehvi3d-mc", 3, lambda: ctx.plan_ehvi3d_mc(cache3, r3, hv_mc)))
    for k in (2, 3, 4):
        out.append((f"boxes{k}", k, lambda k=k: ctx.plan_ehvi_boxes(box[k][0], box[k][2])))
    out.append(("hvpoi", 2, lambda: ctx.plan_hvpoi(cells)))
    out.append(("expdec-tch", 3, lambda: ctx.plan_expdec(cache3, 1, [], w3, Y[:, :3].min(0), Y[:, :3].max(0), 0.4)))
    out.append(("ei", 1, lambda: ctx.plan_ei(0.3, 1e-6)))
    out.append(("pareto-ei", 2, lambda: ctx.plan_ei_ext("pareto", 2, 0.3, 1e-6)))
    out.append(("constrained-ei", 2, lambda: ctx.plan_ei_ext("constrained", 2, 0.3, 0.0, 1e-5)))
    return out


def chain(ctx, Xd, offset=7):
    vals = host(ctx.eval(Xd))
    ctx.synchronize()                     # raises if a kernel marked the fault word
    pair = host(ctx.eval_argmax(Xd, offset=offset))
    ctx.synchronize()
    return vals, pair


# ------------------------------------------------------------------------------------------- 1. constrained EI, bitwise
@pytest.mark.parametrize("c", [1, 2, 7])
def test_ei_plus_constraints_is_constrained_ei_bitwise(ctx, base, c):
    cf.assert_bands(cf.pof(base["mu"][4:4 + c], base["var"][4:4 + c]), c)
    set_slots(ctx, base["obj"][:1] + base["con"][:c])
    Xd = dev(base["Xc"])
    best = float(np.median(base["obj"][0][1]))
    ctx.plan_ei_ext("constrained", 1 + c, best, 0.0, EPS)
    want_v, want_p = chain(ctx, Xd)
    ctx.plan_ei(best, 0.0)
    plain = host(ctx.eval(Xd))
    ctx.plan_constraints(c, EPS)
    got_v, got_p = chain(ctx, Xd)
    assert (want_v > 0).sum() >= 50 and not same(plain, want_v)
    assert same(got_v, want_v) and same(got_p, want_p)


# ------------------------------------------------------------------------------------------- 2. every plan kind
@pytest.mark.parametrize("c", [1, 2])
def test_every_plan_times_feasibility_bitwise(ctx, base, c):
    F_o = cf.pof(base["mu"][4:4 + c], base["var"][4:4 + c])
    cf.assert_bands(F_o, c)
    Xd = dev(base["Xc"])
    seen_nan = False
    for name, k, plan in plans(ctx, base["Y"]):
        set_slots(ctx, base["obj"][:k] + base["con"][:c])
        plan()
        plain = ctx.eval(Xd)
        mu, var = ctx.posterior(Xd, k + c)
        F = ctx.feasibility(mu[k:], var[k:], EPS)
        want = host(plain) * host(F)
        assert same(host(ctx.feasibility(mu[k:], var[k:], EPS, acq=plain)), want), name
        np.testing.assert_allclose(host(F), cf.pof(host(mu[k:]), host(var[k:])), rtol=1e-7, atol=1e-11, err_msg=name)
        plan()
        ctx.plan_constraints(c, EPS)
        got, pair = chain(ctx, Xd)
        assert same(got, want), (name, c)
        assert (pair[0], int(pair[1])) == oacq.argmax(got, offset=7), name
        live = np.isfinite(want) & (want != 0)
        assert live.sum() >= 20 and not same(got, host(plain)), (name, live.sum())
        if name == "ehvi3d-mc":
            seen_nan = bool(np.isnan(want).any()) and same(np.isnan(got), np.isnan(host(plain)))
    assert seen_nan          # the Monte-Carlo plan's NaN rows stay NaN under the weight


def test_feasibility_in_place_and_alone(ctx, base):
    set_slots(ctx, base["obj"][:1] + base["con"][:2])
    Xd = dev(base["Xc"])
    mu, var = ctx.posterior(Xd, 3)
    F = host(ctx.feasibility(mu[1:], var[1:], EPS))
    acq = torch.linspace(-1.0, 2.0, cf.N_CAND, dtype=torch.float64, device="cuda:0")
    acq[5] = float("nan")
    want = host(acq) * F
    out = ctx.feasibility(mu[1:], var[1:], EPS, acq=acq, out=acq)
    assert out is acq and same(host(acq), want) and np.isnan(want[5])
    # σ² + pof_eps < 0: NaN, as in the constrained EI
    neg = var.clone()
    neg[1, 3] = -1.0
    assert np.isnan(host(ctx.feasibility(mu[1:], neg[1:], EPS))[3])


# ------------------------------------------------------------------------------------------- 3. dispatch branches
# (n_train, n_var, seed): every fused-posterior branch, the dense path (n = 1040) and the wide one (n_var = 70).  With
# 40 points in 70 dimensions the posterior is wide and under one constraint about a quarter of the candidates has
# F ≤ 0.01 (16–35 % over seeds); the seed here gives 35 %, and assert_bands holds every case to the condition.
SHAPES = [(n, d, 1000 * n + d) for n in (20, 100, 130, 520) for d in (2, 6, 12)] + [(1040, 6, 1040006), (40, 70, 40072)]


@pytest.mark.parametrize("n,d,seed", SHAPES)
def test_dispatch_branches_agree_bitwise(ctx, n, d, seed):
    """Reference EHVI-2D plus one constraint: objective 1's σ² is masked, the constraint's (slot 2) is not."""
    from optimobo_amd import pareto
    gps, Y, Xc, mu_o, var_o = cf.problem(n, d, seed, 2, 1)
    cf.assert_bands(cf.pof(mu_o[2:], var_o[2:]), (n, d))
    set_slots(ctx, gps)
    Y = Y[:N_GEO]
    s00, s01 = oacq.cache_stats(ref_cache())
    stripes, r2 = pareto.stripes_2d(opar.calc_pf(Y[:, :2])), Y[:, :2].max(0) + 0.1
    Xd, Xother = dev(Xc), dev(Xc[::-1])
    ctx.plan_ehvi2d(stripes, r2, s00, s01, mode="reference")
    plain = host(ctx.eval(Xd))
    mu, var = ctx.posterior(Xd, 3)
    want = plain * host(ctx.feasibility(mu[2:], var[2:], EPS))
    ctx.plan_ehvi2d(stripes, r2, s00, s01, mode="reference")
    ctx.plan_constraints(1, EPS)
    try:
        first = None
        for all_var, mean_kernel in ((0, 1), (1, 1), (0, 0), (0, 2), (1, 0)):
            ctx.debug_set("posterior_all_var", 1)
            ctx.eval(Xother).cpu()            # the workspace holds other candidates' moments
            ctx.debug_set("posterior_all_var", all_var)
            ctx.debug_set("posterior_mean_kernel", mean_kernel)
            vals, pair = chain(ctx, Xd)
            if first is None:
                first = (vals, pair)
                assert same(vals, want)
            assert same(vals, first[0]) and same(pair, first[1]), (n, d, all_var, mean_kernel)
    finally:
        ctx.debug_set("posterior_all_var", 0)
        ctx.debug_set("posterior_mean_kernel", 1)


# ------------------------------------------------------------------------------------------- 4. arg-max
def test_argmax_sobol_and_fused_modes(ctx, base):
    from optimobo_amd import pareto
    Y = base["Y"]
    set_slots(ctx, base["obj"][:2] + base["con"][:2])
    s00, s01 = oacq.cache_stats(ref_cache())
    stripes, r2 = pareto.stripes_2d(opar.calc_pf(Y[:, :2])), Y[:, :2].max(0) + 0.1
    ctx.set_sobol(6, np.zeros(6), np.ones(6), seed=3)
    X = ctx.sobol(5, 4099)
    try:
        for mode in ("reference", "textbook"):
            ctx.debug_set("fused_chain", 0)
            ctx.plan_ehvi2d(stripes, r2, s00, s01, mode=mode)
            ctx.plan_constraints(2, EPS)
            vals = host(ctx.eval(X))
            pair = host(ctx.eval_argmax(X, offset=5))
            assert (pair[0], int(pair[1])) == oacq.argmax(vals, offset=5)
            i = int(np.flatnonzero(vals == np.nanmax(vals))[0])
            assert int(pair[1]) == 5 + i and pair[0] == vals[i]
            assert same(host(ctx.eval_argmax_sobol(5, 4099)), pair)
            for fused in (1, 2):
                ctx.debug_set("fused_chain", fused)
                assert same(host(ctx.eval_argmax(X, offset=5)), pair), (mode, fused)
                assert same(host(ctx.eval_argmax_sobol(5, 4099)), pair), (mode, fused)
            ctx.synchronize()
    finally:
        ctx.debug_set("fused_chain", 0)


# ------------------------------------------------------------------------------------------- 5. lifecycle, return codes
def test_plan_lifecycle_and_return_codes(ctx, base):
    from optimobo_amd import _lib
    from optimobo_amd.device import AcqContext
    set_slots(ctx, base["obj"][:1] + base["con"][:7])
    Xd = dev(base["Xc"][:257])
    lib, h = ctx.lib, ctx._h
    best = float(np.median(base["obj"][0][1]))
    ctx.plan_ei(best, 0.0)
    plain = host(ctx.eval(Xd))
    ctx.plan_constraints(1, EPS)
    con1 = host(ctx.eval(Xd))
    assert not same(plain, con1)
    # a failed call changes nothing
    for n_con, eps, rc in ((-1, EPS, _lib.OMB_EINVAL), (1, -1.0, _lib.OMB_EINVAL), (1, float("nan"), _lib.OMB_EINVAL),
                           (1, float("inf"), _lib.OMB_EINVAL), (8, EPS, _lib.OMB_EUNSUP),
                           (2 ** 31 - 1, EPS, _lib.OMB_EUNSUP)):
        assert lib.omb_plan_constraints(h, n_con, eps) == rc, (n_con, eps)
        assert lib.omb_last_error(h)
        assert same(host(ctx.eval(Xd)), con1), (n_con, eps)
    with pytest.raises(_lib.OMBError) as e:
        ctx.plan_constraints(8, EPS)
    assert e.value.code == _lib.OMB_EUNSUP
    # the most the context holds: 1 + 7
    ctx.plan_constraints(7, EPS)
    assert not same(host(ctx.eval(Xd)), con1)
    # n_con = 0 clears; so does a new plan
    ctx.plan_constraints(0, EPS)
    assert same(host(ctx.eval(Xd)), plain)
    ctx.plan_constraints(1, EPS)
    assert same(host(ctx.eval(Xd)), con1)
    ctx.plan_ei(best, 0.0)
    assert same(host(ctx.eval(Xd)), plain)
    # k + n_con > OMB_MAX_OBJ at k = 2
    ctx.plan_ei_ext("pareto", 2, best, 1e-6)
    assert lib.omb_plan_constraints(h, 7, EPS) == _lib.OMB_EUNSUP
    assert lib.omb_plan_constraints(h, 6, EPS) == _lib.OMB_OK
    # no plan: OMB_ESTATE; a constraint slot with no GP: OMB_ESTATE from the eval calls
    c2 = AcqContext(0)
    try:
        assert c2.lib.omb_plan_constraints(c2._h, 1, EPS) == _lib.OMB_ESTATE
        set_slots(c2, base["obj"][:1])
        c2.plan_ei(best, 0.0)
        assert host(c2.eval(Xd)).shape == (257,)
        c2.plan_constraints(1, EPS)
        vals = torch.full((257,), -7.5, dtype=torch.float64, device="cuda:0")
        grad = torch.full((257, 6), -7.5, dtype=torch.float64, device="cuda:0")
        res = torch.full((2,), -7.5, dtype=torch.float64, device="cuda:0")
        assert c2.lib.omb_eval(c2._h, ptr(Xd), 257, ptr(vals)) == _lib.OMB_ESTATE
        assert c2.lib.omb_eval_argmax(c2._h, ptr(Xd), 257, 0, ptr(res)) == _lib.OMB_ESTATE
        assert c2.lib.omb_eval_grad(c2._h, ptr(Xd), 257, ptr(vals), ptr(grad)) == _lib.OMB_ESTATE
        c2.set_sobol(6, np.zeros(6), np.ones(6), seed=1)
        assert c2.lib.omb_eval_argmax_sobol(c2._h, 0, 257, ptr(res)) == _lib.OMB_ESTATE
        c2.synchronize()
        assert bool((vals == -7.5).all()) and bool((grad == -7.5).all()) and bool((res == -7.5).all())
    finally:
        c2.close()


def test_feasibility_bad_arguments_write_nothing(ctx):
    from optimobo_amd import _lib
    lib, h = ctx.lib, ctx._h
    N = 33
    mu = torch.zeros((2, N), dtype=torch.float64, device="cuda:0")
    var = torch.ones((2, N), dtype=torch.float64, device="cuda:0")
    out = torch.full((N,), -7.5, dtype=torch.float64, device="cuda:0")
    ok = (2, ptr(mu), ptr(var), N, N, EPS, None, ptr(out))
    bad = [(0,) + ok[1:], (-1,) + ok[1:], (9,) + ok[1:],
           ok[:5] + (-1.0,) + ok[6:], ok[:5] + (float("nan"),) + ok[6:], ok[:5] + (float("inf"),) + ok[6:],
           (2, None) + ok[2:], ok[:2] + (None,) + ok[3:], ok[:7] + (None,),
           ok[:3] + (N - 1,) + ok[4:], ok[:4] + (-1,) + ok[5:]]
    for args in bad:
        assert lib.omb_feasibility(h, *args) == _lib.OMB_EINVAL, args
    assert lib.omb_feasibility(h, 2, None, None, 0, 0, EPS, None, None) == _lib.OMB_OK      # N = 0 touches nothing
    assert lib.omb_feasibility(h, *(ok[:4] + (0,) + ok[5:])) == _lib.OMB_OK
    ctx.synchronize()
    assert bool((out == -7.5).all())
    assert lib.omb_feasibility(h, *ok) == _lib.OMB_OK
    ctx.synchronize()
    assert bool((out == 0.25).all())                                                     # Φ(0)²


# ------------------------------------------------------------------------------------------- 6. eval_grad
CASES = ref.acquisition_cases()


def con_gps(name, k, c):
    centre = ([0.5, 0.0, 0.0] if name == "constrained_ei" else [0.5] * k)[:k] + [0.0] * c
    return ref.acq_gps(k + c, centre=centre)


def upload(ctx, gps):
    for o, g in enumerate(gps):
        Linv = linalg.solve_triangular(g.L, np.eye(len(g.L)), lower=True)
        ctx.set_gp(o, g.X, g.lengthscale, g.variance, g.alpha, Linv, g.kernel)


# every case with 1 and 2 constraint models behind its objectives, as far as the context's 8 slots (OMB_MAX_OBJ) go
CASES_CON = [(name, c) for name in sorted(CASES) for c in (1, 2) if CASES[name][0] + c <= 8]


@pytest.mark.parametrize("name,c", CASES_CON, ids=[f"{name}-{c}" for name, c in CASES_CON])
def test_eval_grad_with_constraints(ctx, name, c):
    k, value, partials, plan = CASES[name]
    gps = con_gps(name, k, c)
    upload(ctx, gps)
    plan(ctx)
    ctx.plan_constraints(c, EPS)
    assert ctx.plan_has_gradient()
    Xc = ref.make_candidates(gps[0], 33, train_point=False)
    vals, grad = ctx.eval_grad(dev(Xc))
    assert same(host(vals), host(ctx.eval(dev(Xc))))
    with np.errstate(all="ignore"):
        rg, scale = ref.eval_grad(gps, Xc, cf.pof_partials(value, partials, k))
    g = host(grad)
    assert np.all(np.isfinite(g)) and np.all(np.isfinite(rg))
    tol = TOL_EVAL.get((name, c), TOL)
    err = np.abs(g - rg) / np.where(scale > 0, scale, 1.0)
    print(f"{name} c={c}: |dev - ref| / sum|terms| = {err.max():.3e} (tol {tol:g}); |grad| up to {np.abs(rg).max():.3g}")
    assert np.all(np.abs(g - rg) <= tol * scale), (err.max(), tol)
    assert (np.abs(g).max(1) > 0).sum() >= 20
    # the unconstrained plan's gradient is another one: the constraint rows and the scaling are in
    plan(ctx)
    assert not same(host(ctx.eval_grad(dev(Xc))[1]), g)
    plan(ctx)
    ctx.plan_constraints(c, EPS)
    for i in (0, 5, 32):          # batch independence: a candidate alone gives bitwise its row of the batch
        v1, g1 = ctx.eval_grad(dev(Xc[i:i + 1]))
        assert same(host(v1), host(vals[i:i + 1])) and same(host(g1[0]), host(grad[i]))


@pytest.mark.parametrize("name", ["hvpoi", "ehvi3d-mc", "expdec-tch", "ehvi2d-sigma"])
def test_eval_grad_still_refuses_plans_without_gradient(ctx, base, name):
    from optimobo_amd import _lib
    k, plan = next((k, p) for n, k, p in plans(ctx, base["Y"]) if n == name)
    set_slots(ctx, base["obj"][:k] + base["con"][:1])
    plan()
    ctx.plan_constraints(1, EPS)
    with pytest.raises(_lib.OMBError) as e:
        ctx.eval_grad(dev(base["Xc"][:7]))
    assert e.value.code == _lib.OMB_EUNSUP
    assert ctx.eval(dev(base["Xc"][:7])).shape == (7,)


def test_eval_grad_is_finite_where_F_is_exactly_zero(ctx):
    """A constraint model centred on 50: near its data μ ≈ 50 and Φ(−μ/s) underflows to exactly 0 while EI > 0; far
    from the data μ → 0 and F is about a half.  The rows with F == 0 are finite (zero), not 0/0."""
    gps = ref.acq_gps(2, centre=[0.5, 50.0])
    upload(ctx, gps)
    ctx.plan_ei(0.55, 0.0)
    near = ref.make_candidates(gps[0], 9, train_point=False)
    far = 3.0 + np.random.default_rng(3).uniform(0, 1, (4, 3))
    Xc = np.concatenate([near[:5], far, near[5:]])
    a = host(ctx.eval(dev(Xc)))
    ctx.plan_constraints(1, EPS)
    vals, grad = ctx.eval_grad(dev(Xc))
    vals, g = host(vals), host(grad)
    zero = np.r_[0:5, 9:13]
    assert np.all(a[zero] > 0) and np.all(vals[zero] == 0.0) and np.all(vals[5:9] > 0)
    assert np.all(np.isfinite(g)) and np.all(g[zero] == 0.0) and np.all(np.abs(g[5:9]).max(1) > 0)
    rg, scale = ref.eval_grad(gps, Xc, cf.pof_partials(lambda m, v: oacq.ei(m[0], v[0], 0.55, 0.0),
                                                       lambda m, v: ref.ei_partials(m, v, 0.55, 0.0), 1))
    assert np.all(np.abs(g - rg) <= TOL * scale)


@pytest.mark.parametrize("slot", [0, 1])
def test_eval_grad_nan_row_rule_with_constraints(ctx, slot):
    """A negative variance — L⁻¹ doubled on purpose, as in tests/test_gpu_grad.py — in the objective (EI is NaN) or
    in the constraint model (σ² + pof_eps < 0: F is NaN): that candidate's row is NaN, the others are as alone."""
    gps = ref.acq_gps(2, centre=[0.5, 0.0])
    upload(ctx, gps)
    g = gps[slot]
    Linv = linalg.solve_triangular(g.L, np.eye(len(g.L)), lower=True)
    ctx.set_gp(slot, g.X, g.lengthscale, g.variance, g.alpha, 2.0 * Linv, g.kernel)
    ctx.plan_ei(0.55, 0.0)
    ctx.plan_constraints(1, EPS)
    far = 3.0 + np.random.default_rng(3).uniform(0, 1, (6, 3))
    Xc = np.concatenate([far[:3], g.X[4:5], far[3:]])
    _, var = ctx.posterior(dev(Xc), 2)
    var = host(var[slot])
    assert var[3] < -EPS and np.all(np.delete(var, 3) > 0)
    vals, grad = ctx.eval_grad(dev(Xc))
    assert bool(torch.isnan(vals[3])) and bool(torch.isnan(grad[3]).all())
    for i in (0, 1, 2, 4, 5, 6):
        v1, g1 = ctx.eval_grad(dev(Xc[i:i + 1]))
        assert bool(torch.isfinite(grad[i]).all())
        assert same(host(v1), host(vals[i:i + 1])) and same(host(g1[0]), host(grad[i]))


# ------------------------------------------------------------------------------------------- 7. believer
def test_believer_conditions_the_constraint_models_too(base):
    from optimobo_amd.acquisition import AcquisitionEngine
    from optimobo_amd.gp import GPState
    from optimobo_amd import pareto
    eng = AcquisitionEngine(0).load_models([GPState(*g) for g in base["obj"][:2] + base["con"][:1]])
    Y = base["Y"]
    x = base["Xc"][11:12]
    Xd = dev(base["Xc"])
    mu0, var0 = eng.posterior(Xd)
    m_pt0, v_pt0 = eng.posterior(dev(x))
    F0 = host(eng.feasibility(Xd, 1, EPS))
    np.testing.assert_allclose(F0, cf.pof(host(mu0[2:]), host(var0[2:])), rtol=1e-7, atol=1e-11)
    mus = eng.condition(x)
    assert mus.shape == (1, 3)
    mu1, var1 = eng.posterior(Xd)
    m_pt1, v_pt1 = eng.posterior(dev(x))
    vf = base["con"][0][3]
    print(f"constraint model at x: var {float(v_pt0[2, 0]):.3e} -> {float(v_pt1[2, 0]):.3e}; "
          f"|mu change| over the batch {float((mu1[2] - mu0[2]).abs().max()):.2e}")
    assert float(v_pt1[2, 0]) <= float(v_pt0[2, 0]) and float(v_pt1[2, 0]) <= 1e-6 * vf
    assert float((mu1[2] - mu0[2]).abs().max()) <= 1e-12 * np.sqrt(vf)          # DESIGN §16's bound
    assert bool((var1[2] <= var0[2] + 1e-12 * vf).all())
    # the constrained chain on the conditioned states runs clean and is still plan × feasibility
    s00, s01 = oacq.cache_stats(ref_cache())
    plan = lambda: eng.ctx.plan_ehvi2d(pareto.stripes_2d(opar.calc_pf(Y[:, :2])), Y[:, :2].max(0) + 0.1, s00, s01,  # noqa: E731
                                       mode="textbook")
    plan()
    plain = host(eng.ctx.eval(Xd))
    eng.plan_constraints(1, EPS)
    vals, pair = chain(eng.ctx, Xd)
    assert same(vals, plain * host(eng.feasibility(Xd, 1, EPS)))
    assert (pair[0], int(pair[1])) == oacq.argmax(vals, offset=7)
    with pytest.raises(ValueError):
        eng.feasibility(Xd, 4, EPS)
    eng.ctx.close()


# ------------------------------------------------------------------------------------------- 8. drivers
def _check_result(out, n_init, budget, q, min_feasible=5):
    from optimobo_amd.result import Constrained_Res
    assert isinstance(out, Constrained_Res)
    X, Y = out.Xsample, out.ysample
    assert X.shape == (n_init + budget, 2) and Y.shape == (n_init + budget, 2)
    assert np.all(X >= 0.0) and np.all(X <= 1.0)                                   # proposals in bounds
    feas = 1.5 - X[:, 0] - X[:, 1] <= 0
    assert len(out.X_feasible) == feas.sum() and len(out.X_infeasible) == (~feas).sum()
    yf = Y[feas]
    assert all(any(np.array_equal(p, y) for y in yf) for p in np.atleast_2d(out.pf_approx))
    hv = np.asarray(out.hypervolume_convergence)
    assert len(hv) == -(-budget // q) and np.all(np.diff(hv) >= 0)
    n_feas = int(feas[n_init:].sum())
    print(f"q={q}: {n_feas} of {budget} proposals feasible ({int(feas[:n_init].sum())} of the {n_init} initial); "
          f"hypervolume {hv[0]:.4f} -> {hv[-1]:.4f}")
    assert n_feas >= min_feasible            # 5: uniform sampling expects 1.25 of 10; P(>= 5) < 0.5 %
    return 1.5 - X[n_init:, 0] - X[n_init:, 1]


@pytest.mark.parametrize("q", [1, 4])
def test_multi_surrogate_pof(q):
    import optimobo_amd.algorithms.optimisers as opti
    np.random.seed(31)
    opt = opti.MultiSurrogateOptimiser(cf.driver_problem(), [0, 0], [2.5, 2.0], constraints="pof", mode="textbook",
                                       seed=1, n_candidates=1 << 12, batch_size=q)
    _check_result(opt.solve(budget=10, n_init_samples=12), 12, 10, q)


def test_multi_surrogate_pof_expected_decomposition():
    import optimobo_amd.algorithms.optimisers as opti
    import optimobo_amd.scalarisations as sc
    np.random.seed(32)
    opt = opti.MultiSurrogateOptimiser(cf.driver_problem(), [0, 0], [2.5, 2.0], constraints="pof", mode="textbook",
                                       seed=1, n_candidates=1 << 12, batch_size=4)
    out = opt.solve(budget=10, n_init_samples=12, sample_exponent=3, acquisition_func=sc.Tchebicheff([0, 0], [2.5, 2.0]))
    # A fresh random weight vector per pick: for most of them the scalarisation's constrained optimum is on the edge
    # of the triangle, where a·F peaks at F ≈ ½ and the sign of g is a coin flip (fixture.driver_problem), so no count
    # of feasible proposals is asked here.  What the weight does guarantee is that no pick strays into the infeasible
    # region: g is linear, its model on ≥ 12 points has a posterior sd far below 0.01 near the edge, so at g = 0.05
    # F is below Φ(−5) < 3e-7 — the acquisition, bounded by the objectives' range of 2.3, cannot make that up.
    g = _check_result(out, 12, 10, 4, min_feasible=0)
    print("g of the proposals:", np.array2string(g, precision=4))
    assert g.max() <= 0.05


@pytest.mark.parametrize("q", [1, 4])
def test_mono_surrogate_pof(q):
    import optimobo_amd.algorithms.optimisers as opti
    import optimobo_amd.scalarisations as sc
    np.random.seed(33)
    opt = opti.MonoSurrogateOptimiser(cf.driver_problem(), [0, 0], [2.5, 2.0], constraints="pof", mode="textbook",
                                      seed=1, n_candidates=1 << 12, batch_size=q)
    _check_result(opt.solve(sc.Tchebicheff([0, 0], [2.5, 2.0]), budget=10, n_init_samples=12), 12, 10, q)


def test_pof_value_errors_on_the_device_side():
    """The ValueErrors of tests/test_constraints_host.py hold with a device present as well, and an unsupported
    driver refuses rather than ignoring the keyword."""
    import optimobo_amd.algorithms.optimisers as opti
    from optimobo_amd.algorithms import cparego, emo
    for cls in (emo.EMO, cparego.ParEGO_C2):
        with pytest.raises(ValueError):
            cls(cf.driver_problem(), [0, 0], [2.5, 2.0], constraints="pof")
    with pytest.raises(ValueError):
        opti.MultiSurrogateOptimiser(cf.driver_problem(n_ieq_constr=0), [0, 0], [2.5, 2.0], constraints="pof")
    with pytest.raises(ValueError):
        opti.MonoSurrogateOptimiser(cf.driver_problem(n_eq_constr=1), [0, 0], [2.5, 2.0], constraints="pof")
