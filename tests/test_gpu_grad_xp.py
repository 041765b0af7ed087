"""GPU: the analytic gradients near the data — omb_posterior_grad and omb_eval_grad against the np.longdouble
evaluation of their contract on the installed bits (tests/_grad_xp.py), on the late-run states of
tests/_posterior_xp.py: clustered training rows, jitter only, cond 1e9–1e11, candidates on and between training rows.

Error measure: e = |device − reference| / (u·S), u = 2⁻⁵³, S the entry-wise first-order rounding scale of
``_grad_xp.scales_grad``.  Bar, per candidate group and per output: e ≤ T_group = 4 × the worst e of the plain fp64
numpy restatement on that group over the whole case table, computed at run time.  The bar is relative and per group
because the true gradient spans nine orders of magnitude of u·S near the data: a bound of a few worst-case roundings
would pass a wrong ∂σ²/∂x.  The cases of the table are also held, with the table's own candidates, to the same rule
taken over their own shape (``_grad_xp.case_bar``): the table's ∂σ² bar is set by the wide shapes and lies orders above
what the restatement reaches at n_var ≤ 30.  A case honest rounding cannot hold goes into OVERRIDE at 4 × the value measured on the
MI355X with its cause in DESIGN §32; no entry may exceed the first-order ceiling n + d + 16.

Far and ray candidates: for RBF every term is exactly 0 and so is the device's gradient; for Matern-5/2 they are held
to the reference in absolute terms (``_grad_xp.check_far``).
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]

import _grad_xp as gx  # noqa: E402
import _posterior_xp as xp  # noqa: E402

LD = np.longdouble
# (n, d, kernel) → {group: (T_∂μ, T_∂σ²)} where the bar is not reached by honest rounding
OVERRIDE = {}


@pytest.fixture(scope="module")
def ctx():
    from optimobo_amd.device import AcqContext
    c = AcqContext(0)
    yield c
    c.close()


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device="cuda:0")


def bits(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.int64)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def bar(n, d, kernel, own_candidates=False):
    """group → (T_∂μ, T_∂σ²): the table's bar; on a case of the table with the table's own candidates also the
    shape's own bar, which is calibrated on exactly those candidates (the tighter of the two per entry); OVERRIDE
    replaces both."""
    T = dict(gx.bar())
    if own_candidates:
        own = gx.case_bar(n, d)
        T = {g: (min(T[g][0], own[g][0]), min(T[g][1], own[g][1])) for g in T}
    T.update(OVERRIDE.get((n, d, kernel), {}))
    assert all(max(t) <= gx.ceiling(n, d) for t in T.values()), (T, gx.ceiling(n, d))
    return T


def check_grads(label, st, kernel, dmu, dvar, rg, S, sets=((0, None),), own_candidates=False):
    """∂μ, ∂σ² (N, d) of one objective against its reference.  ``sets``: (first row, group) of every stacked copy of
    the 44 candidates; group None holds each candidate group to its own bar, a name holds all 36 near rows to that
    group's (candidates that are not laid out around this objective's training rows)."""
    n, d = st.X.shape
    T = bar(n, d, kernel, own_candidates)
    e_mu, e_var = gx.normalised(dmu, rg.dmu, S[0]).max(1), gx.normalised(dvar, rg.dvar, S[1]).max(1)
    assert np.all(np.isfinite(dmu)) and np.all(np.isfinite(dvar)), label
    worst, failed = {"dmu": (0.0, "-", 0.0), "dvar": (0.0, "-", 0.0)}, []
    for r0, forced in sets:
        for name, lo, hi in gx.NEAR:
            t = T[forced or name]
            for what, e, tt in (("dmu", e_mu, t[0]), ("dvar", e_var, t[1])):
                w = float(e[r0 + lo:r0 + hi].max())
                if w / tt > worst[what][0] / max(worst[what][2], 1e-300) or worst[what][1] == "-":
                    worst[what] = (w, name, tt)
                if not w <= tt:
                    failed.append((what, name, r0, w, tt))
    full = gx.by_group(e_mu, gx.NEAR, sets[0][0]), gx.by_group(e_var, gx.NEAR, sets[0][0])
    print(f"{label}: closest to its bar: e_dmu {worst['dmu'][0]:.3g} ({worst['dmu'][1]}, T {worst['dmu'][2]:.3g})  "
          f"e_dvar {worst['dvar'][0]:.3g} ({worst['dvar'][1]}, T {worst['dvar'][2]:.3g})   per group dmu/dvar: "
          + " ".join(f"{g}={full[0][g]:.3g}/{full[1][g]:.3g}" for g, _, _ in gx.NEAR))
    assert not failed, (label, failed)
    for r0, _ in sets:
        for rows in (xp.FAR, xp.RAY):
            gx.check_far(label, st, kernel, dmu, dvar, rg, slice(r0 + rows.start, r0 + rows.stop))


# ----------------------------------------------------------------------------- omb_posterior_grad, every launch path
@pytest.mark.parametrize("kernel", xp.KERNELS)
@pytest.mark.parametrize("n,d", xp.CASES)
def test_posterior_grad_xp(ctx, n, d, kernel):
    cases = [gx.case(n, d, kernel, o) for o in range(2)]
    for o, c in enumerate(cases):
        ctx.set_gp_state(o, c[0])
    Xc = dev(cases[0][1])
    mu, var, dmu, dvar = ctx.posterior_grad(Xc, 2)
    mu0, var0 = ctx.posterior(Xc, 2)
    assert np.array_equal(bits(mu), bits(mu0)) and np.array_equal(bits(var), bits(var0))
    again = ctx.posterior_grad(Xc, 2)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip((mu, var, dmu, dvar), again))
    dmu, dvar = dmu.cpu().numpy(), dvar.cpu().numpy()
    assert dmu.shape == (2, xp.N_CAND, d) and dvar.shape == (2, xp.N_CAND, d)
    for o, (st, Xo, _, rg, S) in enumerate(cases):
        check_grads(f"n={n} d={d} {kernel} obj={o}", st, kernel, dmu[o], dvar[o], rg, S, own_candidates=True)
        # the older suites' unit (tests/test_gpu_grad.py): the error as a fraction of the plain term sum, on the 16
        # candidates on and next to training rows, for the device and for the fp64 restatement
        near = slice(0, 16)
        frac = lambda g: float(np.max(np.abs(g[near].astype(LD) - rg.dvar[near]) / rg.av[near]))  # noqa: E731
        print(f"n={n} d={d} {kernel} obj={o}: |dvar - reference| / sum|terms| on training rows: device {frac(dvar[o]):.2e}, "
              f"restatement {frac(gx.restatement_grad(st, Xo, kernel)[1]):.2e}")


# ----------------------------------------------------------------------------- mixed n_train in one call
@pytest.mark.parametrize("kernel", xp.KERNELS)
@pytest.mark.parametrize("pair", [((1040, 6), (20, 6)), ((300, 6), (50, 6))], ids=["dense-1040+20", "ring-300+50"])
def test_mixed_n_train_grad(ctx, pair, kernel):
    """Objectives of different n_train in one omb_posterior_grad call (n_max ≠ n of the smaller one: its rows of the
    chunk buffers are pitched by n_max), each held to its own reference on both objectives' candidate sets.  An
    objective's own set is held group by group; the other's candidates are points in general position to it, and
    are held to the ``uniform`` group's bar."""
    sts = [xp.late_run_state(n, d, kernel, obj=o) for o, (n, d) in enumerate(pair)]
    Xc = np.vstack([xp.candidates(st, np.random.default_rng(31 + o)) for o, st in enumerate(sts)])
    for o, st in enumerate(sts):
        ctx.set_gp_state(o, st)
    mu, var, dmu, dvar = ctx.posterior_grad(dev(Xc), 2)
    mu0, var0 = ctx.posterior(dev(Xc), 2)
    assert np.array_equal(bits(mu), bits(mu0)) and np.array_equal(bits(var), bits(var0))
    dmu, dvar = dmu.cpu().numpy(), dvar.cpu().numpy()
    for o, st in enumerate(sts):
        ref = xp.reference(st, Xc, kernel)
        rg = gx.reference_grad(st, Xc, kernel, ref)
        S = gx.scales_grad(st, Xc, kernel, ref, rg)
        sets = tuple((xp.N_CAND * q, None if q == o else "uniform") for q in range(2))
        check_grads(f"mixed {pair} {kernel} obj={o} (n={st.X.shape[0]})", st, kernel, dmu[o], dvar[o], rg, S, sets)


# ----------------------------------------------------------------------------- the second pass of the chain
def test_second_chunk(ctx):
    """The smallest call that makes the gradient chain take a second pass: 8 objectives of n_train 1040 and 130
    alternating, d = 6, N = chunk + 37 candidates.  The second pass has a shorter chunk, so another leading dimension
    of K*, V and W, and writes at candidate offset c0 > 0."""
    kernel, d, n_obj = "matern52", 6, 8
    shapes = [1040 if o % 2 == 0 else 130 for o in range(n_obj)]
    sts = [xp.late_run_state(n, d, kernel, obj=(o // 2) % 2) for o, n in enumerate(shapes)]
    # the header's rule: passes of at most 512 MiB of K*, V, W — (n_obj + 2)·n_max doubles per candidate
    chunk = min(max((512 << 20) // ((n_obj + 2) * max(shapes) * 8), 64), 1 << 20)
    assert chunk == 6452
    N = chunk + 37
    assert N > chunk
    rng = np.random.default_rng(5)
    Xc = rng.uniform(0.0, 1.0, (N, d))
    lo = chunk - 22
    Xc[lo:lo + xp.N_CAND] = xp.candidates(sts[0], np.random.default_rng(17))     # 22 rows on either side
    for o, st in enumerate(sts):
        ctx.set_gp_state(o, st)
    Xd = dev(Xc)
    guard, fill = 4096, -7.5
    sizes = [n_obj * N, n_obj * N, n_obj * N * d, n_obj * N * d]
    bufs = [torch.full((s + 2 * guard,), fill, dtype=torch.float64, device="cuda:0") for s in sizes]
    ctx._stream()
    ctx._check(ctx.lib.omb_posterior_grad(ctx._h, n_obj, ptr(Xd), N, *[ptr(b[guard:]) for b in bufs]),
               "omb_posterior_grad")
    ctx.synchronize()
    for b, s in zip(bufs, sizes):
        assert bool((b[:guard] == fill).all()) and bool((b[guard + s:] == fill).all())
        assert bool(torch.isfinite(b[guard:guard + s]).all()) and not bool((b[guard:guard + s] == fill).any())
    mu, var = (b[guard:guard + s].reshape(n_obj, N) for b, s in zip(bufs[:2], sizes[:2]))
    dmu, dvar = (b[guard:guard + s].reshape(n_obj, N, d) for b, s in zip(bufs[2:], sizes[2:]))
    # a candidate's results depend neither on N nor on its place in the batch
    for r in (0, chunk - 1, chunk, chunk + 1, N - 1):
        alone = ctx.posterior_grad(Xd[r:r + 1], n_obj)
        for name, a, b in zip(("mu", "var", "dmu", "dvar"), alone, (mu, var, dmu, dvar)):
            assert np.array_equal(bits(a[:, 0]), bits(b[:, r])), (name, r)
    # the 44 candidates across the boundary: objectives 0, 2, … are laid out around their own data
    Xb = Xc[lo:lo + xp.N_CAND]
    dmu_b, dvar_b = dmu[:, lo:lo + xp.N_CAND].cpu().numpy(), dvar[:, lo:lo + xp.N_CAND].cpu().numpy()
    refs = {}
    for o, st in enumerate(sts):
        key = (shapes[o], (o // 2) % 2)
        if key not in refs:
            ref = xp.reference(st, Xb, kernel)
            rg = gx.reference_grad(st, Xb, kernel, ref)
            refs[key] = (rg, gx.scales_grad(st, Xb, kernel, ref, rg))
        rg, S = refs[key]
        check_grads(f"second chunk obj={o} (n={shapes[o]})", st, kernel, dmu_b[o], dvar_b[o], rg, S,
                    ((0, None if shapes[o] == 1040 else "uniform"),))


# ----------------------------------------------------------------------------- the partial kernels, in isolation
PARTIAL_STATES = [(50, 4), (130, 6)]
PARTIAL_ROWS = np.r_[8:12, 16:24, 24:36]          # train+1e-6, cluster, uniform
POF_EPS = 1e-5


def _mp():
    import mpmath as mp
    mp.mp.dps = 50
    return mp


def _mp_ei(mp, mu, var, best, var_eps):
    """EI's partials and their terms' magnitudes at one candidate: (dm, dv, A_μ, A_σ², a, A_a), a the value."""
    sigma = mp.sqrt(mp.mpf(var) + mp.mpf(var_eps))
    s1 = sigma + mp.mpf(1e-10)
    gam = (mp.mpf(best) - mp.mpf(mu)) / s1
    P, p = mp.ncdf(gam), mp.npdf(gam)
    h = gam * P + p
    dm = -sigma * P / s1
    dv = (h - sigma * P * gam / s1) / (2 * sigma)
    A_v = (abs(gam * P) + p + abs(sigma * P * gam / s1)) / (2 * sigma)
    return dm, dv, abs(dm), A_v, sigma * h, sigma * (abs(gam * P) + p)


def _mp_ehvi2d(mp, mu, var, pf, r, s00, s01, mode):
    """omb_ehvi2d's partials as ehvi2d_grad_kernel's header states them, stripe by stripe."""
    f = mp.mpf
    m0, m1 = f(mu[0]), f(mu[1])
    if mode == "reference":
        sA, sB = f(var[0]) * f(s00), f(var[0]) * f(s01)
    else:
        sA, sB = mp.sqrt(f(var[0])), mp.sqrt(f(var[1]))
    E = lambda a, m, s: s * mp.npdf((a - m) / s) + (a - m) * mp.ncdf((a - m) / s)  # noqa: E731
    g = [f(0)] * 4          # gm0, gsA, gm1, gsB
    A = [f(0)] * 4
    P = len(pf)
    for i in range(1, P + 1):
        y1p = f(r[0]) if i == 1 else f(pf[i - 2, 0])
        y1i, y2i = f(pf[i - 1, 0]), f(pf[i - 1, 1])
        tp, t, u = (y1p - m0) / sA, (y1i - m0) / sA, (y2i - m1) / sB
        p2 = E(y2i, m1, sB)
        Ai = (y1p - y1i) * mp.ncdf(t) + E(y1p, m0, sA) - (sA * mp.npdf(t) + (y1p - m0) * mp.ncdf(t))
        terms = [(mp.ncdf(t) - mp.ncdf(tp)) * p2, (mp.npdf(tp) - mp.npdf(t)) * p2, -Ai * mp.ncdf(u), Ai * mp.npdf(u)]
        g = [a + b for a, b in zip(g, terms)]
        A = [a + abs(b) for a, b in zip(A, terms)]
    if mode == "textbook":
        y1P = f(pf[P - 1, 0])
        tP, u = (y1P - m0) / sA, (f(r[1]) - m1) / sB
        EA, EB = E(y1P, m0, sA), E(f(r[1]), m1, sB)
        terms = [-mp.ncdf(tP) * EB, mp.npdf(tP) * EB, -EA * mp.ncdf(u), EA * mp.npdf(u)]
        g = [a + b for a, b in zip(g, terms)]
        A = [a + abs(b) for a, b in zip(A, terms)]
        return ([g[0], g[2]], [g[1] / (2 * sA), g[3] / (2 * sB)], [A[0], A[2]],
                [A[1] / abs(2 * sA), A[3] / abs(2 * sB)])
    return ([g[0], g[2]], [g[1] * f(s00) + g[3] * f(s01), f(0)], [A[0], A[2]],
            [A[1] * abs(f(s00)) + A[3] * abs(f(s01)), f(0)])


def _mp_boxes(mp, mu, var, lo, hi):
    """Exact EHVI's partials over the boxes (lo, hi (B, k); lo may be −inf), box by box."""
    f = mp.mpf
    k = len(mu)
    m, sd = [f(x) for x in mu], [mp.sqrt(f(x)) for x in var]
    dm, ds, Am, As = [f(0)] * k, [f(0)] * k, [f(0)] * k, [f(0)] * k
    for b in range(lo.shape[0]):
        T, Tm, Ts = [], [], []
        for j in range(k):
            u = f(hi[b, j])
            be = (u - m[j]) / sd[j]
            if np.isfinite(lo[b, j]):
                l = f(lo[b, j])
                al = (l - m[j]) / sd[j]
                Pa, pa, first = mp.ncdf(al), mp.npdf(al), (u - l) * mp.ncdf(al)
            else:
                Pa, pa, first = f(0), f(0), f(0)
            T.append(first + (u - m[j]) * (mp.ncdf(be) - Pa) + sd[j] * (mp.npdf(be) - pa))
            Tm.append(-(mp.ncdf(be) - Pa))
            Ts.append(mp.npdf(be) - pa)
        for j in range(k):
            others = f(1)
            for i in range(k):
                if i != j:
                    others *= T[i]
            dm[j] += others * Tm[j]
            ds[j] += others * Ts[j]
            Am[j] += abs(others * Tm[j])
            As[j] += abs(others * Ts[j])
    return dm, [ds[j] / (2 * sd[j]) for j in range(k)], Am, [As[j] / (2 * sd[j]) for j in range(k)]


def _mp_constrained_ei(mp, mu, var, best, var_eps, pof_eps):
    """EI·F with one constraint model (row 1): the product rule of pof_grad_kernel's header."""
    dm0, dv0, Am0, Av0, a, Aa = _mp_ei(mp, mu[0], var[0], best, var_eps)
    s = mp.sqrt(mp.mpf(var[1]) + mp.mpf(pof_eps))
    z = -mp.mpf(mu[1]) / s
    F, p = mp.ncdf(z), mp.npdf(z)
    dm1, dv1 = a * p * (-1 / s), a * p * mp.mpf(mu[1]) / (2 * s ** 3)
    return ([dm0 * F, dm1], [dv0 * F, dv1], [Am0 * F, Aa * p / s], [Av0 * F, Aa * p * abs(mp.mpf(mu[1])) / (2 * s ** 3)])


def _ld(x):
    """An mpmath number as np.longdouble: its fp64 head plus the fp64 head of what is left."""
    h = float(x)
    return LD(h) + LD(float(x - h))


def _partial_plans(Y):
    """name → (family, K rows, plan(ctx), stand-alone value(ctx, mu, var), mp partials(mu, var) of one candidate,
    numpy partials(mu, var)) — the plans the drivers polish with, placed on the targets' range."""
    import test_grad_reference as ref
    from _constraints_fixture import pof_partials
    from oracle import acquisition as oacq
    mp = _mp()
    best = float(np.median(Y[:, 0]))
    lo_y, span = Y.min(0), Y.max(0) - Y.min(0)
    rng = np.random.default_rng(11)
    cache = rng.normal(size=(64, 2))
    cache[:, 1] = 0.6 * cache[:, 0] + 0.8 * cache[:, 1]
    s00, s01 = oacq.cache_stats(cache)
    plans = {}
    for eps in (0.0, 1e-6):
        plans[f"ei_eps{eps:g}"] = (
            "ei", 1,
            (lambda c: c.plan_ei(best, 0.0)) if eps == 0.0 else (lambda c, eps=eps: c.plan_ei_ext("plain", 1, best, eps)),
            (lambda c, m, v: c.ei(m[0], v[0], best, 0.0)) if eps == 0.0 else
            (lambda c, m, v, eps=eps: c.ei_ext("plain", m, v, best, eps)),
            lambda m, v, eps=eps: tuple([x] for x in _mp_ei(mp, m[0], v[0], best, eps)[:4]),
            lambda m, v, eps=eps: ref.ei_partials(m, v, best, eps))
    pf01, r01 = ref.front(2, 9)
    pf, r = lo_y[:2] + pf01 * span[:2], lo_y[:2] + r01 * span[:2]
    pf = pf[np.argsort(pf[:, 1])]
    for mode in ("reference", "textbook"):
        plans[f"ehvi2d_{mode}_P9"] = (
            "ehvi2d", 2, lambda c, mode=mode: c.plan_ehvi2d(pf, r, s00, s01, mode=mode),
            lambda c, m, v, mode=mode: c.ehvi2d(m, v, pf, r, s00, s01, mode=mode),
            lambda m, v, mode=mode: _mp_ehvi2d(mp, m, v, pf, r, s00, s01, mode),
            lambda m, v, mode=mode: ref.ehvi2d_partials(m, v, pf, r, s00, s01, mode))
    for k in (2, 3):
        pfk, rk = ref.front(k, 6)
        pfk, rk = lo_y[:k] + pfk * span[:k], lo_y[:k] + rk * span[:k]
        coords, boxes, lo, hi = ref.box_lists(pfk, rk)
        plans[f"boxes_k{k}"] = (
            "boxes", k, lambda c, coords=coords, boxes=boxes: c.plan_ehvi_boxes(coords, boxes),
            lambda c, m, v, coords=coords, boxes=boxes: c.ehvi_boxes(m, v, coords, boxes),
            lambda m, v, lo=lo, hi=hi: _mp_boxes(mp, m, v, lo, hi),
            lambda m, v, lo=lo, hi=hi: ref.boxes_partials(m, v, lo, hi))

    def plan_con(c):
        c.plan_ei(best, 0.0)
        c.plan_constraints(1, POF_EPS)

    plans["ei_constrained"] = (
        "constrained", 2, plan_con,
        lambda c, m, v: c.feasibility(m[1:], v[1:], POF_EPS, acq=c.ei(m[0], v[0], best, 0.0)),
        lambda m, v: _mp_constrained_ei(mp, m, v, best, 0.0, POF_EPS),
        pof_partials(lambda m, v: oacq.ei(m[0], v[0], best, 0.0), lambda m, v: ref.ei_partials(m, v, best, 0.0), 1,
                     POF_EPS))
    return plans


def _third_state(st):
    from optimobo_amd.gp import GPState
    y = np.sin(2.0 * st.X + 1.0).sum(1)
    return GPState(st.X, y, st.lengthscale, float(np.var(y) + 0.1), kernel=st.kernel)


def test_acquisition_partials_at_device_moments(ctx):
    """omb_eval_grad = Σ_o ∂a/∂μ_o·∂μ_o/∂x + ∂a/∂σ²_o·∂σ²_o/∂x with the device's own moments and posterior gradients
    taken as given: what is left is the partial kernels (omb_grad.hip) and the chain rule.  The partials are evaluated
    in mpmath at 50 digits at exactly the device's fp64 μ, σ², contracted in longdouble with the device's own ∂μ, ∂σ²,
    and omb_eval_grad is held to that within T·u·Σ_o (A_μ,o|∂μ_o| + A_σ²,o|∂σ²_o|), A the sum of the magnitudes of the
    stripe, box or factor terms of the partial.  T is 4 × the error of tests/test_grad_reference.py's numpy partials
    in the same units, per family, computed here, and at least 2K + 2: one rounding per product and sum of the chain
    rule over K rows."""
    kernel = "matern52"
    records = []
    for n, d in PARTIAL_STATES:
        sts = [xp.late_run_state(n, d, kernel, obj=o) for o in range(2)]
        sts.append(_third_state(sts[0]))
        Xc = xp.candidates(sts[0], np.random.default_rng(7000 * n + d))[PARTIAL_ROWS]
        for o, st in enumerate(sts):
            ctx.set_gp_state(o, st)
        Y = np.column_stack([st.y.reshape(-1) for st in sts])
        Xd = dev(Xc)
        for name, (family, K, plan, value, mp_partials, np_partials) in _partial_plans(Y).items():
            plan(ctx)
            mu, var = ctx.posterior(Xd, K)
            _, _, dmu, dvar = ctx.posterior_grad(Xd, K)
            vals, grad = ctx.eval_grad(Xd)
            assert np.array_equal(bits(vals), bits(ctx.eval(Xd)))
            assert np.array_equal(bits(value(ctx, mu, var)), bits(vals)), name
            mu, var, vals, grad = (t.cpu().numpy() for t in (mu, var, vals, grad))
            dmu, dvar = dmu.cpu().numpy().astype(LD), dvar.cpu().numpy().astype(LD)
            # a NaN value gives an all-NaN row, and nothing else does
            nan_v = np.isnan(vals)
            assert np.array_equal(nan_v, np.isnan(grad).all(1)) and np.array_equal(nan_v, np.isnan(grad).any(1)), name
            with np.errstate(all="ignore"):
                ndm, ndv = np_partials(mu, var)
            rows = np.flatnonzero(~nan_v)
            # every group is held: a plan whose near-data rows all had a NaN value (σ² < 0 under var_eps = 0, say)
            # would otherwise be checked on the uniform rows alone, without notice
            for group, lo, hi in (("train+1e-6", 0, 4), ("cluster", 4, 12), ("uniform", 12, 24)):
                assert not nan_v[lo:hi].all(), (name, n, d, group)
            assert len(rows) >= len(PARTIAL_ROWS) // 2, (name, n, d, len(rows))
            e_dev = e_np = 0.0
            for c in rows:
                dm, dv, Am, Av = mp_partials(mu[:, c], var[:, c])
                exact = sum(_ld(dm[o]) * dmu[o, c] + _ld(dv[o]) * dvar[o, c] for o in range(K))
                scale = sum(_ld(Am[o]) * np.abs(dmu[o, c]) + _ld(Av[o]) * np.abs(dvar[o, c]) for o in range(K))
                numpy_ = sum(LD(ndm[o][c]) * dmu[o, c] + LD(ndv[o][c]) * dvar[o, c] for o in range(K))
                zero = scale == 0
                assert np.all(grad[c][zero] == 0.0), (name, c)
                if zero.all():
                    continue
                unit = LD(xp.U) * np.where(zero, LD(1), scale)
                # Φ, φ and their products below fp64's range are 0 on the device and in numpy, not in mpmath: an
                # absolute 1e-290 per unit of |∂μ|, |∂σ²| (the floor the far rows get) comes off before the count
                floor = LD(1e-290) * sum(np.abs(dmu[o, c]) + np.abs(dvar[o, c]) for o in range(K))
                over = lambda g: np.where(zero, 0, np.maximum(np.abs(g - exact) - floor, 0) / unit)  # noqa: E731
                e_dev = max(e_dev, float(np.max(over(grad[c].astype(LD)))))
                if np.all(np.isfinite(np.asarray(numpy_, np.float64))):
                    e_np = max(e_np, float(np.max(over(numpy_))))
            records.append((family, K, f"n={n} d={d} {name}", e_dev, e_np, len(rows)))
    T = {}
    for family, K, _, _, e_np, _ in records:
        T[family] = max(T.get(family, 0.0), 4.0 * e_np)
    failed = []
    for family, K, label, e_dev, e_np, used in records:
        t = max(T[family], 2.0 * K + 2.0)
        print(f"{label}: eval_grad against the mpmath partials x device gradients: e {e_dev:.2f} roundings of the term "
              f"sum (numpy partials {e_np:.2f}; T {t:.2f}; {used} of {len(PARTIAL_ROWS)} rows with a value)")
        if not e_dev <= t:
            failed.append((label, e_dev, t))
    assert not failed, failed
