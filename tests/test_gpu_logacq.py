"""GPU: the log-space acquisitions — omb_log_ei, omb_log_feasibility, omb_log_ehvi_boxes, omb_plan_log, the log
chain and its gradient, and the drivers' log_acquisition.

References and inputs come from tests/_logacq_reference.py; tests/test_logacq_host.py states, without a device, the
restatement's own error on exactly these inputs and the conditions on them (a third of the linear values exactly 0).

Accuracy bar: the worst e = |x − ref| / max(1, |ref|) of the device against the 60-digit reference is at most 8 × the
worst e of the fp64 numpy restatement on the same inputs (the device's log, exp and erfcx are the ROCm library's at a
couple of ulp against glibc's in numpy, and its sums run in another order).  Both figures are printed.  The accuracy
is taken on the largest batch of each input set; the smaller batches (N at and around the wave and the candidate
block) must give bitwise that batch's leading values — a candidate's value does not depend on N — which holds them
to the same bar.
Gradient bar: tests/test_gpu_grad.py's, |dev − ref| ≤ 1e-9 · Σ|terms|.
"""
import ctypes

import numpy as np
import pytest
from scipy import linalg

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _constraints_fixture as cf  # noqa: E402
import _logacq_reference as R  # noqa: E402
import test_grad_reference as ref  # noqa: E402
from oracle import gp as ogp  # noqa: E402

BAR = 8.0
TOL = 1e-9
SENT = -7.5


@pytest.fixture(scope="module")
def ctx():
    from optimobo_amd.device import AcqContext
    c = AcqContext(0)
    yield c
    c.close()


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device="cuda:0")


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def host(t):
    return t.cpu().numpy()


def same(a, b):
    """Bit for bit, NaN matching NaN."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    na = np.isnan(a)
    return a.shape == b.shape and np.array_equal(na, np.isnan(b)) and \
        np.array_equal(a[~na].view(np.int64), b[~na].view(np.int64))


def padded(a, N):
    """Rows of a[:, :N] at a pitch of N + 3, the padding NaN: (the (k, N) view, its storage)."""
    t = torch.full((a.shape[0], N + 3), float("nan"), dtype=torch.float64, device="cuda:0")
    t[:, :N] = dev(a[:, :N])
    return t[:, :N], t


def out_with_sentinel(N):
    return torch.full((N + 1,), SENT, dtype=torch.float64, device="cuda:0")


def upload(ctx, gps):
    for o, g in enumerate(gps):
        Linv = linalg.solve_triangular(g.L, np.eye(len(g.L)), lower=True)
        ctx.set_gp(o, g.X, g.lengthscale, g.variance, g.alpha, Linv, g.kernel)


def check_bar(tag, got, want, restated):
    e_dev, e_np = R.err(got, want).max(), R.err(restated, want).max()
    print(f"{tag}: device worst e {e_dev:.3g}, restatement worst e {e_np:.3g} (bar {BAR:g}x)")
    assert np.all(np.isfinite(got)) and e_dev <= BAR * e_np, (tag, e_dev, e_np)


# ------------------------------------------------------------------------------------------- 1. log EI, log F
N_FULL = 1000
N_SMALL = (1, 63, 64, 65)


@pytest.mark.parametrize("c", [0, 1, 3])
def test_log_ei_against_the_reference(ctx, c):
    mu, var = R.ei_inputs()
    kind = "constrained" if c else "plain"
    full = None
    for N in (N_FULL,) + N_SMALL:
        (m, _), (v, _) = padded(mu[:1 + c], N), padded(var[:1 + c], N)
        out = out_with_sentinel(N)
        ctx.log_ei(m, v, R.BEST, 0.0, R.CON_EPS, kind=kind, out=out)
        ctx.synchronize()
        got = host(out)
        assert got[N] == SENT
        if N == N_FULL:
            full = got[:N]
            check_bar(f"log EI c={c} N={N}", full, R.ei_reference(c)[:N],
                      R.log_ei(mu[:1 + c, :N], var[:1 + c, :N], R.BEST, 0.0, R.CON_EPS))
        else:
            assert same(got[:N], full[:N]), N
    # the linear kernel is exactly 0 on at least a third of these inputs; the log of it says nothing there
    lin = host(ctx.ei_ext(kind, dev(mu[:1 + c, :N_FULL]), dev(var[:1 + c, :N_FULL]), R.BEST, 0.0, R.CON_EPS))
    assert (lin == 0.0).mean() >= 1 / 3 and np.all(np.isfinite(full[lin == 0.0]))
    if c:      # the constrained kind is bitwise log_feasibility over the plain kind
        plain = ctx.log_ei(dev(mu[:1, :N_FULL]), dev(var[:1, :N_FULL]), R.BEST)
        assert same(host(ctx.log_feasibility(dev(mu[1:1 + c, :N_FULL]), dev(var[1:1 + c, :N_FULL]), R.CON_EPS,
                                             acq=plain)), full)


@pytest.mark.parametrize("c", [1, 3])
def test_log_feasibility_against_the_reference(ctx, c):
    mu, var = R.pof_inputs()
    full = None
    for N in (N_FULL,) + N_SMALL:
        (m, _), (v, _) = padded(mu[:c], N), padded(var[:c], N)
        out = out_with_sentinel(N)
        ctx.log_feasibility(m, v, 0.0, out=out)
        ctx.synchronize()
        got = host(out)
        assert got[N] == SENT
        if N == N_FULL:
            full = got[:N]
            check_bar(f"log F c={c} N={N}", full, R.pof_reference(c)[:N], R.log_pof(mu[:c, :N], var[:c, :N], 0.0))
        else:
            assert same(got[:N], full[:N]), N
    # in place equals out of place, bit for bit
    acq = dev(np.linspace(-900.0, 3.0, N_FULL))
    m, v = dev(mu[:c, :N_FULL]), dev(var[:c, :N_FULL])
    apart = host(ctx.log_feasibility(m, v, 0.0, acq=acq))
    x = acq.clone()
    assert ctx.log_feasibility(m, v, 0.0, acq=x, out=x) is x
    assert same(host(x), apart) and same(apart, host(acq) + full)


def test_log_ei_edges(ctx):
    """σ = 0 is −inf (the log of the linear 0); a negative σ² + var_eps and a NaN moment are NaN, each in its own
    column only; none of them wins the arg-max."""
    mu = np.array([[0.5, 0.5, np.nan, 0.5, 0.5]])
    var = np.array([[1e-2, 0.0, 1e-2, -1e-3, np.nan]])
    got = host(ctx.log_ei(dev(mu), dev(var), 0.3))
    assert np.isfinite(got[0]) and got[1] == -np.inf and np.all(np.isnan(got[2:]))
    assert host(ctx.ei(dev(mu[0]), dev(var[0]), 0.3))[1] == 0.0
    v, i = ctx.argmax(dev(got[::-1].copy()))
    assert i == 4 and v == got[0]
    lf = host(ctx.log_feasibility(dev(np.array([[0.0, np.nan, 1.0]])), dev(np.array([[1.0, 1.0, -1.0]])), 1e-5))
    assert abs(lf[0] - np.log(0.5)) < 1e-5          # z = 0 but for pof_eps
    assert np.all(np.isnan(lf[1:]))


# ------------------------------------------------------------------------------------------- 2. log exact EHVI
BOX_N = (1, 7, 8, 9, 33)


@pytest.mark.parametrize("k,P", R.BOX_SHAPES + (R.BOX_BIG,))
def test_log_ehvi_boxes_against_the_reference(ctx, k, P):
    coords, boxes, mu, var = R.box_case(k, P)
    n_all = mu.shape[1]
    cd, bd = dev(coords), ctx._boxes_dev(boxes)
    full = None
    for N in (n_all,) + BOX_N:
        (m, _), (v, _) = padded(mu, N), padded(var, N)
        out = out_with_sentinel(N)
        ctx.log_ehvi_boxes(m, v, cd, bd, out=out)
        ctx.synchronize()
        got = host(out)
        assert got[N] == SENT
        if N == n_all:
            full = got[:N]
            check_bar(f"log EHVI k={k} B={len(boxes)} N={N}", full, R.box_reference(k, P),
                      R.log_box_sum(coords, boxes, mu, var))
        else:
            assert same(got[:N], full[:N]), N       # N = 1 included: column 0 alone is column 0 of every batch
    # column 0 of the batch is column 17 of the batch shifted by 17, bit for bit
    sh = host(ctx.log_ehvi_boxes(dev(np.roll(mu, 17, axis=1)), dev(np.roll(var, 17, axis=1)), cd, bd))
    assert same(sh[17:18], full[:1]) and same(np.roll(sh, -17), full)
    # where the linear kernel's value is an ordinary number, exp(log) is that value within that kernel's own tolerance
    lin = host(ctx.ehvi_boxes(dev(mu), dev(var), cd, bd, kd=True))
    alive = lin > 1e-200
    assert alive.mean() >= 1 / 3 and (lin == 0.0).mean() >= 1 / 3 and lin[0] == 0.0
    np.testing.assert_allclose(np.exp(full[alive]), lin[alive], rtol=1e-9, atol=1e-13)
    assert np.all(np.isfinite(full[lin == 0.0]))


@pytest.mark.parametrize("k,P", [(2, 5), (6, 5)])
def test_log_ehvi_boxes_nan_stays_in_its_column(ctx, k, P):
    coords, boxes, mu, var = R.box_case(k, P)
    cd, bd = dev(coords), ctx._boxes_dev(boxes)
    clean = host(ctx.log_ehvi_boxes(dev(mu[:, :9]), dev(var[:, :9]), cd, bd))
    m, v = mu[:, :9].copy(), var[:, :9].copy()
    m[0, 2] = np.nan
    v[k - 1, 4] = np.nan
    v[1, 5] = 0.0
    v[0, 7] = -1e-3
    got = host(ctx.log_ehvi_boxes(dev(m), dev(v), cd, bd))
    bad = [2, 4, 5, 7]
    assert np.all(np.isnan(got[bad]))
    keep = np.setdiff1d(np.arange(9), bad)
    assert same(got[keep], clean[keep])


# ------------------------------------------------------------------------------------------- 3. chain
def _plan_boxes(ctx, coords, boxes, kd):
    c = np.ascontiguousarray(coords, dtype=np.float64)
    b = np.ascontiguousarray(boxes, dtype=np.uint16)
    from optimobo_amd import _lib
    ctx._plan("omb_plan_ehvi_boxes_k" if kd else "omb_plan_ehvi_boxes", c.shape[0], _lib.host_ptr(c), c.shape[1],
              _lib.host_ptr(b), b.shape[0])


@pytest.mark.parametrize("N", [1, 33])
def test_log_ei_chain_is_the_stand_alone_entries_bitwise(ctx, N):
    gps = ref.acq_gps(3, centre=[0.5, 0.0, 0.0])
    upload(ctx, gps)
    Xd = dev(ref.make_candidates(gps[0], N, train_point=False))
    mu, var = ctx.posterior(Xd, 3)
    want = host(ctx.log_ei(mu[:1], var[:1], 0.55))
    ctx.plan_ei(0.55, 0.0)
    linear = host(ctx.eval(Xd))
    ctx.plan_log()
    assert same(host(ctx.eval(Xd)), want) and not same(want, linear)
    for c in (1, 2):
        both = host(ctx.log_feasibility(mu[1:1 + c], var[1:1 + c], 1e-5, acq=dev(want)))
        ctx.plan_ei(0.55, 0.0)
        ctx.plan_log()
        ctx.plan_constraints(c, 1e-5)
        assert same(host(ctx.eval(Xd)), both)
        ctx.plan_ei(0.55, 0.0)
        ctx.plan_constraints(c, 1e-5)
        ctx.plan_log()
        assert same(host(ctx.eval(Xd)), both)
        pair = host(ctx.eval_argmax(Xd, offset=7))
        assert pair[0] == np.max(both) and int(pair[1]) == 7 + int(np.argmax(both))
    # the constrained kind as a plan: omb_log_ei's constrained value
    ctx.plan_ei_ext("constrained", 3, 0.55, 0.0, 1e-5)
    ctx.plan_log()
    assert same(host(ctx.eval(Xd)), host(ctx.log_ei(mu, var, 0.55, 0.0, 1e-5, kind="constrained")))
    ctx.plan_log(False)
    assert same(host(ctx.eval(Xd)), host(ctx.ei_ext("constrained", mu, var, 0.55, 0.0, 1e-5)))


@pytest.mark.parametrize("kd", [False, True])
@pytest.mark.parametrize("k", [2, 3])
def test_log_box_chain_is_the_stand_alone_entry_bitwise(ctx, k, kd):
    pf, r = ref.front(k, 6)
    coords, boxes, _, _ = ref.box_lists(pf, r)
    gps = ref.acq_gps(k + 1, centre=[0.5] * k + [0.0])
    upload(ctx, gps)
    Xd = dev(ref.make_candidates(gps[0], 33, train_point=False))
    mu, var = ctx.posterior(Xd, k + 1)
    want = host(ctx.log_ehvi_boxes(mu[:k], var[:k], coords, boxes))
    _plan_boxes(ctx, coords, boxes, kd)
    linear = host(ctx.eval(Xd))
    ctx.plan_log()
    assert same(host(ctx.eval(Xd)), want)
    np.testing.assert_allclose(np.exp(want), linear, rtol=1e-9, atol=1e-13)
    both = host(ctx.log_feasibility(mu[k:], var[k:], 1e-5, acq=dev(want)))
    ctx.plan_constraints(1, 1e-5)
    assert same(host(ctx.eval(Xd)), both)
    _plan_boxes(ctx, coords, boxes, kd)
    ctx.plan_constraints(1, 1e-5)
    ctx.plan_log()
    assert same(host(ctx.eval(Xd)), both)


def _mp_argmax(vals):
    order = np.argsort(-vals, kind="stable")
    assert vals[order[0]] - vals[order[1]] >= 1e-6          # a condition on the inputs: the reference's winner is clear
    return int(order[0])


def _linear_then_log(ctx, Xd, reference):
    """The linear plan that is set scores exactly 0 everywhere and its arg-max is index 0; its logarithm names the
    60-digit reference's winner (reference(mu, var) over the device's own moments)."""
    linear = host(ctx.eval(Xd))
    assert np.all(linear == 0.0)
    pair = host(ctx.eval_argmax(Xd))
    assert pair[0] == 0.0 and int(pair[1]) == 0
    ctx.plan_log()
    K = len(ctx.gp_info)
    mu, var = ctx.posterior(Xd, K)
    want = _mp_argmax(reference(host(mu), host(var)))
    vals = host(ctx.eval(Xd))
    pair = host(ctx.eval_argmax(Xd))
    assert np.all(np.isfinite(vals)) and want != 0
    assert int(pair[1]) == want and pair[0] == vals[want]


def test_argmax_where_linear_ei_is_zero_everywhere():
    """Candidates a hair off the training points of a GP whose σ² there is ~1e-12·σ_f²: γ < −38 on every one."""
    from optimobo_amd.device import AcqContext
    g0 = ref.make_gp(30, 3, seed=9)
    y = 0.5 + 0.3 * g0.y[:, 0]
    g = ogp.ExactGP(g0.X, y, g0.lengthscale, 1e4)
    best = float(y.min())
    idx = np.flatnonzero(y - best > 0.05)[::-1]        # in this order the reference's winner is not candidate 0
    Xc = g.X[idx] + 1e-6 * np.random.default_rng(4).standard_normal((len(idx), 3))
    c = AcqContext(0)
    try:
        upload(c, [g])
        _, var = c.posterior(dev(Xc), 1)
        assert 0.0 < float(var.min()) and float(var.max()) <= 1e-10 * 1e4
        c.plan_ei(best, 0.0)
        _linear_then_log(c, dev(Xc), lambda m, v: np.array([float(R.mp_log_ei(m[0, i], v[0, i], best))
                                                              for i in range(m.shape[1])]))
    finally:
        c.close()


def test_argmax_where_the_linear_box_sum_is_zero_everywhere():
    """Surrogates centred on r + 0.3 with σ_f = 0.01: near their data every candidate is ~30 σ beyond r in every
    objective."""
    from optimobo_amd.device import AcqContext
    coords, boxes, _, _ = R.box_case(2, 5)
    gps = []
    for o in range(2):
        g0 = ref.make_gp(17, 3, seed=5, obj=o)
        gps.append(ogp.ExactGP(g0.X, R.R_REF + 0.3 + 0.003 * g0.y[:, 0], g0.lengthscale, 1e-4, noise=1e-8))
    Xc = ref.make_candidates(gps[0], 33, train_point=False)
    c = AcqContext(0)
    try:
        upload(c, gps)
        c.plan_ehvi_boxes(coords, boxes)
        _linear_then_log(c, dev(Xc), lambda m, v: np.array([
            float(R.mp_log_box_sum(coords, boxes, m[:, i], np.sqrt(v[:, i]))) for i in range(m.shape[1])]))
    finally:
        c.close()


def test_argmax_where_the_feasibility_weight_is_zero_everywhere():
    """tests/test_gpu_constraints.py's constraint model centred on 50: F is exactly 0 near its data, so EI·F is."""
    from optimobo_amd.device import AcqContext
    gps = ref.acq_gps(2, centre=[0.5, 50.0])
    Xc = ref.make_candidates(gps[0], 33, train_point=False)
    c = AcqContext(0)
    try:
        upload(c, gps)
        c.plan_ei(0.55, 0.0)
        a = host(c.eval(dev(Xc)))
        assert np.all(a > 0.0)
        c.plan_constraints(1, 1e-5)
        _linear_then_log(c, dev(Xc), lambda m, v: np.array([
            float(R.mp_log_ei(m[0, i], v[0, i], 0.55) + R.mp_log_pof(m[1:, i], v[1:, i], 1e-5))
            for i in range(m.shape[1])]))
    finally:
        c.close()


# ------------------------------------------------------------------------------------------- 4. gradients
GRAD_CASES = {
    # name: (objective rows of the plan, constraint rows of omb_plan_constraints, best)
    "plain": (1, 0, 0.55), "plain-far": (1, 0, -3.0), "constrained": (3, 0, 0.55), "constrained-far": (3, 0, -3.0),
    "plain+1": (1, 1, 0.55), "plain+2-far": (1, 2, -3.0), "constrained+1": (3, 1, 0.55),
}


def _log_partials(k, c, best):
    def f(mu, var):
        dm, dv = np.zeros_like(mu), np.zeros_like(mu)
        dm[:k], dv[:k] = R.log_ei_partials(mu[:k], var[:k], best, 0.0, 1e-5)
        if c:
            dm[k:], dv[k:] = R.log_pof_partials(mu[k:], var[k:], 1e-5)
        return dm, dv
    return f


@pytest.mark.parametrize("name", sorted(GRAD_CASES))
def test_eval_grad_on_log_ei(ctx, name):
    k, c, best = GRAD_CASES[name]
    gps = ref.acq_gps(k + c, centre=[0.5] + [0.0] * (k + c - 1))
    upload(ctx, gps)
    ctx.plan_ei_ext("constrained" if k > 1 else "plain", k, best, 0.0, 1e-5)
    linear_grad = host(ctx.eval_grad(dev(ref.make_candidates(gps[0], 33, train_point=False)))[1])
    ctx.plan_log()
    if c:
        ctx.plan_constraints(c, 1e-5)
    assert ctx.plan_has_gradient()
    Xc = ref.make_candidates(gps[0], 33, train_point=False)
    vals, grad = ctx.eval_grad(dev(Xc))
    assert same(host(vals), host(ctx.eval(dev(Xc))))
    with np.errstate(all="ignore"):
        rg, scale = ref.eval_grad(gps, Xc, _log_partials(k, c, best))
    g = host(grad)
    assert np.all(np.isfinite(g)) and np.all(np.isfinite(rg))
    e = np.abs(g - rg) / np.where(scale > 0, scale, 1.0)
    print(f"log EI {name}: |dev - ref| / sum|terms| = {e.max():.3e} (tol {TOL:g}); |grad| up to {np.abs(rg).max():.3g}")
    assert np.all(np.abs(g - rg) <= TOL * scale), e.max()
    assert (np.abs(g).max(1) > 0).sum() == 33
    if name.endswith("far"):       # γ < −40: the linear gradient is exactly 0 there and this one is not
        mu, var = ctx.posterior(dev(Xc), 1)
        gam = (best - host(mu[0])) / (np.sqrt(host(var[0])) + 1e-10)
        far = gam < -40.0
        assert far.sum() >= 5 and np.all(linear_grad[far] == 0.0)
        assert np.all(np.abs(g[far]).max(1) > 0)
    for i in (0, 5, 32):           # N = 1 is that row of N = 33, bit for bit
        v1, g1 = ctx.eval_grad(dev(Xc[i:i + 1]))
        assert same(host(v1), host(vals[i:i + 1])) and same(host(g1[0]), host(grad[i]))


def test_eval_grad_nan_row_rule_on_a_log_plan(ctx):
    gps = ref.acq_gps(2, centre=[0.5, 0.0])
    upload(ctx, gps)
    g = gps[0]
    Linv = linalg.solve_triangular(g.L, np.eye(len(g.L)), lower=True)
    ctx.set_gp(0, g.X, g.lengthscale, g.variance, g.alpha, 2.0 * Linv, g.kernel)      # a negative σ² at the data
    ctx.plan_ei(0.55, 0.0)
    ctx.plan_log()
    ctx.plan_constraints(1, 1e-5)
    far = 3.0 + np.random.default_rng(3).uniform(0, 1, (6, 3))
    Xc = np.concatenate([far[:3], g.X[4:5], far[3:]])
    vals, grad = ctx.eval_grad(dev(Xc))
    assert bool(torch.isnan(vals[3])) and bool(torch.isnan(grad[3]).all())
    for i in (0, 1, 2, 4, 5, 6):
        v1, g1 = ctx.eval_grad(dev(Xc[i:i + 1]))
        assert bool(torch.isfinite(grad[i]).all())
        assert same(host(v1), host(vals[i:i + 1])) and same(host(g1[0]), host(grad[i]))


@pytest.mark.parametrize("kd", [False, True])
def test_eval_grad_refuses_the_log_box_plan(ctx, kd):
    from optimobo_amd import _lib
    pf, r = ref.front(2, 6)
    coords, boxes, _, _ = ref.box_lists(pf, r)
    gps = ref.acq_gps(2)
    upload(ctx, gps)
    Xd = dev(ref.make_candidates(gps[0], 7, train_point=False))
    _plan_boxes(ctx, coords, boxes, kd)
    assert ctx.plan_has_gradient()
    ctx.plan_log()
    assert not ctx.plan_has_gradient()
    want = host(ctx.eval(Xd))
    vals = torch.full((7,), SENT, dtype=torch.float64, device="cuda:0")
    grad = torch.full((7, 3), SENT, dtype=torch.float64, device="cuda:0")
    assert ctx.lib.omb_eval_grad(ctx._h, ptr(Xd), 7, ptr(vals), ptr(grad)) == _lib.OMB_EUNSUP
    assert b"log exact EHVI" in ctx.lib.omb_last_error(ctx._h)
    ctx.synchronize()
    assert bool((vals == SENT).all()) and bool((grad == SENT).all())
    assert same(host(ctx.eval(Xd)), want)                       # the plan is still set, and still the log plan
    ctx.plan_log(False)
    assert ctx.plan_has_gradient() and ctx.eval_grad(Xd)[1].shape == (7, 3)


# ------------------------------------------------------------------------------------------- 5. omb_plan_log's rules
def test_plan_log_refusals_leave_the_plan_as_it_was(ctx):
    import test_gpu_constraints as tgc
    from optimobo_amd import _lib
    gps, Y, Xc, _, _ = cf.problem(40, 3, 40003, 4, 1)
    tgc.set_slots(ctx, gps)
    Xd = dev(Xc[:65])
    refused = {"ehvi2d-reference": b"EHVI-2D", "ehvi2d-textbook": b"EHVI-2D", "ehvi2d-sigma": b"EHVI-2D",
               "ehvi3d-mc": b"Monte-Carlo EHVI", "hvpoi": b"HV-PoI", "expdec-tch": b"expected decomposition",
               "pareto-ei": b"Pareto EI"}
    seen = set()
    for name, k, plan in tgc.plans(ctx, Y[:tgc.N_GEO]):
        plan()
        before = host(ctx.eval(Xd))
        rc = ctx.lib.omb_plan_log(ctx._h, 1)
        if name in refused:
            seen.add(name)
            assert rc == _lib.OMB_EUNSUP and refused[name] in ctx.lib.omb_last_error(ctx._h), name
            assert same(host(ctx.eval(Xd)), before), name
            assert ctx.lib.omb_plan_log(ctx._h, 0) == _lib.OMB_EUNSUP            # refused whatever `on` is
        else:
            assert rc == _lib.OMB_OK, name
            assert not same(host(ctx.eval(Xd)), before), name
            assert ctx.lib.omb_plan_log(ctx._h, 2) == _lib.OMB_EINVAL and ctx.lib.omb_plan_log(ctx._h, -1) == _lib.OMB_EINVAL
            assert not same(host(ctx.eval(Xd)), before), name                    # a failed call keeps the flag
            plan()                                                               # a new plan clears it
            assert same(host(ctx.eval(Xd)), before), name
            assert ctx.lib.omb_plan_log(ctx._h, 1) == _lib.OMB_OK and ctx.lib.omb_plan_log(ctx._h, 0) == _lib.OMB_OK
            assert same(host(ctx.eval(Xd)), before), name
    assert seen == set(refused)


def test_new_entries_check_order(ctx):
    from optimobo_amd import _lib
    from optimobo_amd.device import AcqContext
    lib, h = ctx.lib, ctx._h
    E, U, S = _lib.OMB_EINVAL, _lib.OMB_EUNSUP, _lib.OMB_ESTATE
    N = 9
    mu = torch.zeros((3, N), dtype=torch.float64, device="cuda:0")
    var = torch.ones((3, N), dtype=torch.float64, device="cuda:0")
    out = torch.full((N,), SENT, dtype=torch.float64, device="cuda:0")
    # omb_plan_log: no plan (OMB_ESTATE) before the value of `on` (OMB_EINVAL) before the plan's kind (OMB_EUNSUP)
    c2 = AcqContext(0)
    try:
        assert c2.lib.omb_plan_log(c2._h, 7) == S and c2.lib.omb_plan_log(c2._h, 1) == S
        c2.plan_ei_ext("pareto", 2, 0.3, 1e-6)
        assert c2.lib.omb_plan_log(c2._h, 7) == E and c2.lib.omb_plan_log(c2._h, 1) == U
    finally:
        c2.close()
    # omb_log_ei: (kind, k, eps) as omb_ei_ext (OMB_EINVAL), then Pareto (OMB_EUNSUP), then the pointers
    ei = lambda kind, k, m, v, ld, n, eps, o: lib.omb_log_ei(h, kind, k, m, v, ld, n, 0.3, eps, 1e-5, o)  # noqa: E731
    assert ei(_lib.EI_PARETO, 3, None, None, N, N, 0.0, None) == E          # k does not fit the kind: before Pareto
    assert ei(_lib.EI_PARETO, 2, None, None, N, N, -1.0, None) == E
    assert ei(_lib.EI_PARETO, 2, None, None, N, N, 0.0, None) == U          # Pareto: before the null pointers
    assert ei(_lib.EI_PLAIN, 1, None, ptr(var), N, N, 0.0, ptr(out)) == E
    assert ei(_lib.EI_CONSTRAINED, 3, ptr(mu), ptr(var), N - 1, N, 0.0, ptr(out)) == E
    assert ei(7, 1, ptr(mu), ptr(var), N, N, 0.0, ptr(out)) == E
    assert ei(_lib.EI_PLAIN, 1, None, None, 0, 0, 0.0, None) == _lib.OMB_OK
    # omb_log_feasibility: omb_feasibility's
    lf = lambda c, m, v, ld, n, eps, o: lib.omb_log_feasibility(h, c, m, v, ld, n, eps, None, o)  # noqa: E731
    assert lf(0, None, None, N, N, -1.0, None) == E and lf(9, ptr(mu), ptr(var), N, N, 1e-5, ptr(out)) == E
    assert lf(2, ptr(mu), ptr(var), N, N, float("nan"), ptr(out)) == E
    assert lf(2, ptr(mu), ptr(var), N - 1, N, 1e-5, ptr(out)) == E and lf(2, ptr(mu), ptr(var), N, N, 1e-5, None) == E
    assert lf(2, None, None, 0, 0, 1e-5, None) == _lib.OMB_OK
    # omb_log_ehvi_boxes: omb_ehvi_boxes_k's — k (OMB_EINVAL), the grid (OMB_EUNSUP), B, then the pointers
    coords, boxes, _, _ = R.box_case(3, 6)
    cd, bd = dev(coords), ctx._boxes_dev(boxes)
    C, B = coords.shape[1], len(boxes)
    lb = lambda k, m, cc, Cc, bb, Bb, o: lib.omb_log_ehvi_boxes(h, k, m, ptr(var), N, N, cc, Cc, bb, Bb, o)  # noqa: E731
    assert lb(1, None, None, 1, None, 0, None) == E and lb(9, None, None, 1, None, 0, None) == E
    assert lb(3, None, None, 1, None, 0, None) == U and lb(3, None, None, 4000, None, 0, None) == U
    assert lb(3, None, None, C, None, 0, None) == E and lb(3, None, None, C, None, (1 << 24) + 1, None) == U
    assert lb(3, None, ptr(cd), C, ptr(bd), B, ptr(out)) == E and lb(3, ptr(mu), None, C, ptr(bd), B, ptr(out)) == E
    assert lb(3, ptr(mu), ptr(cd), C, ctypes.c_void_p(bd.data_ptr() + 2), B - 1, ptr(out)) == E      # not 4-byte aligned
    ctx.synchronize()
    assert bool((out == SENT).all())
    assert lb(3, ptr(mu), ptr(cd), C, ptr(bd), B, ptr(out)) == _lib.OMB_OK
    ctx.synchronize()
    assert bool(torch.isfinite(out).all())


# ------------------------------------------------------------------------------------------- 6. engine and drivers
def test_maximise_log_feasibility_where_feasibility_is_flat():
    """The constraint surrogate centred on 50: F is exactly 0 over the whole unit box, so maximising it returns the
    value 0.0 at whatever point; log F is finite and the maximiser climbs it."""
    from optimobo_amd.acquisition import AcquisitionEngine
    gps = ref.acq_gps(2, centre=[0.5, 50.0])
    eng = AcquisitionEngine(0)
    upload(eng.ctx, gps)
    eng.n_obj = 2
    try:
        lo, hi = np.zeros(3), np.ones(3)
        kw = dict(n_candidates=1 << 10, seed=3, refine_rounds=2, starts=1)
        _, v = eng.maximise(lambda Xd: eng.feasibility(Xd, 1), lo, hi, **kw)
        assert v == 0.0
        x, v = eng.maximise(lambda Xd: eng.log_feasibility(Xd, 1), lo, hi, **kw)
        assert np.isfinite(v) and v < -700.0 and np.all(x >= lo) and np.all(x <= hi)
        eng.ctx.set_sobol(3, lo, hi, seed=3)
        X0 = host(eng.ctx.sobol(0, 1 << 10))

        def host_log_f(X):
            m, s2 = gps[1].predict(X)
            return R.log_pof(m[:, 0][None] * 1.0, (s2[:, 0] - gps[1].noise)[None], 1e-5)
        top0 = host_log_f(X0).max()
        got = host_log_f(x[None, :])[0]
        print(f"log F: round 0's best {top0:.6f}, maximise's point {got:.6f} (device value {v:.6f})")
        assert got >= top0 - 1e-9 * abs(top0)
    finally:
        eng.ctx.close()


def _check(out, n_init, budget):
    X, Y = out.Xsample, out.ysample
    assert X.shape == (n_init + budget, 2) and Y.shape == (n_init + budget, 2)
    assert np.all(X >= 0.0) and np.all(X <= 1.0) and np.all(np.isfinite(Y))
    assert len(out.hypervolume_convergence) == budget


@pytest.mark.parametrize("constraints", [None, "pof"])
def test_mono_surrogate_log_acquisition(constraints):
    import optimobo_amd.algorithms.optimisers as opti
    import optimobo_amd.scalarisations as sc
    np.random.seed(41)
    opt = opti.MonoSurrogateOptimiser(cf.driver_problem(), [0, 0], [2.5, 2.0], constraints=constraints, seed=1,
                                      n_candidates=1 << 10, log_acquisition=True, polish="auto")
    _check(opt.solve(sc.Tchebicheff([0, 0], [2.5, 2.0]), budget=3, n_init_samples=8), 8, 3)


@pytest.mark.parametrize("constraints", [None, "pof"])
def test_multi_surrogate_log_acquisition(constraints):
    import optimobo_amd.algorithms.optimisers as opti
    np.random.seed(42)
    opt = opti.MultiSurrogateOptimiser(cf.driver_problem(), [0, 0], [2.5, 2.0], constraints=constraints, seed=1,
                                       mode="textbook", n_candidates=1 << 10, log_acquisition=True, polish="auto")
    _check(opt.solve(budget=3, n_init_samples=8), 8, 3)
