"""CPU: the numpy restatement of the analytic gradients (∂μ/∂x, ∂σ²/∂x of the exact GP posterior and the chain rule
through the closed-form acquisitions), validated against fourth-order (Richardson) central differences of the
oracle: ExactGP.predict and oracle.acquisition's ei / pareto_ei / constrained_ei / ehvi2d (both modes) /
ehvi_exact_boxes.  tests/test_gpu_grad.py imports the restatement as the reference of omb_posterior_grad and
omb_eval_grad.

Formulas: k_i = k(x, X_i), s_ij = (x_j − X_ij)/ℓ_j², ∂k_i/∂x_j = g_i s_ij with
g_i = −(5/3)σ_f²(1 + √5 r_i)e^{−√5 r_i} (Matern-5/2) or −k_i (RBF); ∂μ/∂x_j = Σ_i α_i g_i s_ij;
∂σ²/∂x_j = −2 Σ_i w_i g_i s_ij, w = L⁻ᵀ(L⁻¹k), with ExactGP's L and α.

Bar: |analytic − finite difference| ≤ 1e-6 · Σ_i |term_i| (the finite difference's own error is what limits it).
Surrogates have lengthscales of 0.3–1 of the unit box and cond(K + 1e-8 I + noise·I) ≤ 1e8 (asserted here), which
keeps the restatement's own rounding error — about cond·2^-53 of the term sum — far inside the GPU tests' bar.
"""
import functools

import numpy as np
import pytest
from scipy import linalg
from scipy.special import ndtr

from oracle import acquisition as oacq
from oracle import gp as ogp

SQRT5 = np.sqrt(5.0)
SHAPES = [(1, 1), (5, 2), (17, 3), (64, 6), (130, 30), (40, 70), (1040, 6)]
BATCHES = [1, 7, 33]
FD_BAR = 1e-6


# ----------------------------------------------------------------------------------------------- surrogates
def gp_noise(kernel, n, d):
    """Observation noise on the diagonal (part of Ky, so of L and α).  It keeps cond ≤ 1e8 (the RBF kernel at these
    lengthscales is numerically singular on its own in few dimensions), and it keeps the reference's own error
    inside the GPU tests' bar at a training point: there w = e_m − (noise + 1e-8)·Ky⁻¹e_m and s_mj = 0, so every
    term of ∂σ²/∂x is of the order of the noise while w carries an absolute rounding error of about
    2^-53·‖L⁻¹‖²‖k‖ in ANY fp64 evaluation through L — with the 1e-8 jitter alone the restatement and the device
    differ there by up to 6e-7 of the term sum (measured), which is noise against noise.  Neither of the
    two is the one in error: against the extended-precision reference of tests/_grad_xp.py on jitter-only late-run
    states, the restatement and the device are each that far from the exact value on training rows (from 1e-8 of the
    term sum at n_var ≤ 8 through 1e-4 at n_var = 40 to 2e-3 at n_var ≥ 70), and both stay within a fraction of one rounding of the first-order
    scale that prices W's cancellation.  That regime is tested there, with that scale, not here."""
    return 1e-4


def make_gp(n, d, kernel="matern52", seed=0, obj=0):
    """ExactGP on n points of the unit box [0, 1]^d, ARD lengthscales in [0.3, 1]."""
    rng = np.random.default_rng(1000 * seed + 10 * n + d + 7 * obj)
    X = rng.uniform(0.0, 1.0, (n, d))
    ls = rng.uniform(0.3, 1.0, d)
    w = rng.normal(size=d) / np.sqrt(d)
    y = np.sin(3.0 * X @ w + obj) + 0.5 * np.cos(2.0 * X.sum(1) / np.sqrt(d) + obj) + 0.1 * rng.normal(size=n)
    return ogp.ExactGP(X, y, ls, 0.8 + 0.3 * obj, kernel=kernel, noise=gp_noise(kernel, n, d))


def make_candidates(gp, N, seed=0, train_point=True):
    """N points of the unit box, each within 0.15 (per coordinate) of a training point — where a maximiser works,
    and where the posterior differs from the prior at every d; with train_point the first one is a training point."""
    rng = np.random.default_rng(77 + seed + N)
    n, d = gp.X.shape
    Xc = np.clip(gp.X[rng.integers(0, n, N)] + rng.uniform(-0.15, 0.15, (N, d)), 0.0, 1.0)
    if train_point:
        Xc[0] = gp.X[len(gp.X) // 2]
    return Xc


def cond_K(gp):
    s = np.linalg.svd(gp.L, compute_uv=False)
    return (s[0] / s[-1]) ** 2


# ----------------------------------------------------------------------------------------------- restatement
def kernel_terms(gp, Xc):
    """g (n, N) and s (n, N, d) of the header's formulas, from direct differences."""
    diff = Xc[None, :, :] - gp.X[:, None, :]                     # (n, N, d): x_j − X_ij
    r = np.sqrt(np.sum(np.square(diff / gp.lengthscale), axis=2))
    if gp.kernel == "matern52":
        k = gp.variance * (1.0 + SQRT5 * r + 5.0 / 3.0 * r ** 2) * np.exp(-SQRT5 * r)
        g = -(5.0 / 3.0) * gp.variance * (1.0 + SQRT5 * r) * np.exp(-SQRT5 * r)
    else:
        k = gp.variance * np.exp(-0.5 * r ** 2)
        g = -k
    return k, g, diff / gp.lengthscale ** 2


def posterior_grad(gp, Xc):
    """(mu, var, dmu, dvar, smu, svar): μ, σ² (N,), their gradients (N, d) and the sums of the term magnitudes
    Σ_i |α_i g_i s_ij|, Σ_i |2 w_i g_i s_ij| (N, d) the tolerances are stated in."""
    Xc = np.atleast_2d(np.asarray(Xc, np.float64))
    k, g, s = kernel_terms(gp, Xc)
    v = linalg.solve_triangular(gp.L, k, lower=True)
    w = linalg.solve_triangular(gp.L.T, v, lower=False)
    a = gp.alpha[:, 0]
    tm = (a[:, None] * g)[:, :, None] * s
    tv = -2.0 * (w * g)[:, :, None] * s
    mu = k.T @ a
    var = gp.variance - np.square(v).sum(0)
    return mu, var, tm.sum(0), tv.sum(0), np.abs(tm).sum(0), np.abs(tv).sum(0)


def _pdf(t):
    return np.exp(-0.5 * t * t) / np.sqrt(2.0 * np.pi)


def ei_partials(mu, var, best, var_eps=0.0, kind="plain", pof_eps=1e-5):
    """∂a/∂μ_o, ∂a/∂σ²_o (k, N) of the EI family (oracle.acquisition.ei / pareto_ei / constrained_ei)."""
    mu, var = np.atleast_2d(mu), np.atleast_2d(var)
    sigma = np.sqrt(var[0] + var_eps)
    s1 = sigma + 1e-10
    gam = (best - mu[0]) / s1
    P, p = ndtr(gam), _pdf(gam)
    h = gam * P + p
    ei = sigma * h
    dm0 = -sigma * P / s1
    dv0 = (h - sigma * P * gam / s1) / (2.0 * sigma)
    dm, dv = np.zeros_like(mu), np.zeros_like(mu)
    if kind == "plain":
        dm[0], dv[0] = dm0, dv0
    elif kind == "pareto":
        dm[0], dv[0], dm[1] = mu[1] * dm0, mu[1] * dv0, ei
    else:
        sc = np.sqrt(var[1:] + pof_eps)
        z = -mu[1:] / sc
        Pz = ndtr(z)
        dm[0], dv[0] = dm0 * Pz.prod(0), dv0 * Pz.prod(0)
        for c in range(len(z)):
            others = ei * np.prod(np.delete(Pz, c, axis=0), axis=0)
            dm[1 + c] = others * _pdf(z[c]) * (-1.0 / sc[c])
            dv[1 + c] = others * _pdf(z[c]) * mu[1 + c] / (2.0 * sc[c] ** 3)
    return dm, dv


def ehvi2d_partials(mu, var, pf, r, s00, s01, mode):
    """∂a/∂μ_o, ∂a/∂σ²_o (2, N) of oracle.acquisition.ehvi2d: with E(a; m, s) = sφ(t) + (a − m)Φ(t), t = (a − m)/s
    (∂E/∂m = −Φ, ∂E/∂s = φ), stripe i is A_i·E(y2_i; μ1, σB) with ∂A_i/∂μ0 = Φ(t_i) − Φ(t_{i−1}) and
    ∂A_i/∂σA = φ(t_{i−1}) − φ(t_i)."""
    y1, y2 = oacq.stripes_2d(pf, r)
    n = len(y1) - 2
    m0, m1 = mu
    if mode == "reference":
        sA, sB = var[0] * s00, var[0] * s01
    else:
        sA, sB = np.sqrt(var[0]), np.sqrt(var[1])
    E = lambda a, m, s: s * _pdf((a - m) / s) + (a - m) * ndtr((a - m) / s)  # noqa: E731
    gm0 = np.zeros_like(m0)
    gsA, gm1, gsB = gm0.copy(), gm0.copy(), gm0.copy()
    for i in range(1, n + 1):
        tp, t, u = (y1[i - 1] - m0) / sA, (y1[i] - m0) / sA, (y2[i] - m1) / sB
        p2 = E(y2[i], m1, sB)
        A = (y1[i - 1] - y1[i]) * ndtr(t) + E(y1[i - 1], m0, sA) - (sA * _pdf(t) + (y1[i - 1] - m0) * ndtr(t))
        gm0 += (ndtr(t) - ndtr(tp)) * p2
        gsA += (_pdf(tp) - _pdf(t)) * p2
        gm1 -= A * ndtr(u)
        gsB += A * _pdf(u)
    if mode == "textbook":
        tP, u = (y1[n] - m0) / sA, (r[1] - m1) / sB
        EA, EB = E(y1[n], m0, sA), E(r[1], m1, sB)
        gm0 -= ndtr(tP) * EB
        gsA += _pdf(tP) * EB
        gm1 -= EA * ndtr(u)
        gsB += EA * _pdf(u)
        return np.array([gm0, gm1]), np.array([gsA / (2.0 * sA), gsB / (2.0 * sB)])
    return np.array([gm0, gm1]), np.array([gsA * s00 + gsB * s01, np.zeros_like(gm0)])


def boxes_partials(mu, var, lo, hi):
    """∂a/∂μ_j, ∂a/∂σ²_j (k, N) of oracle.acquisition.ehvi_exact_boxes: T_j = E(u) − E(l),
    ∂T_j/∂μ_j = −(Φ(β) − Φ(α)), ∂T_j/∂σ_j = φ(β) − φ(α), ∂EHVI/∂μ_j = Σ_b (Π_{i≠j} T_i) ∂T_j/∂μ_j."""
    mu = np.asarray(mu, np.float64)
    k = mu.shape[0]
    sd = np.sqrt(np.asarray(var, np.float64))
    fin = np.isfinite(lo)
    lf = np.where(fin, lo, 0.0)
    T, Tm, Ts = [], [], []
    for j in range(k):
        l, u, f = lf[:, j, None], hi[:, j, None], fin[:, j, None]
        al, be = (l - mu[j]) / sd[j], (u - mu[j]) / sd[j]
        Pa, pa = np.where(f, ndtr(al), 0.0), np.where(f, _pdf(al), 0.0)
        T.append(np.where(f, (u - l) * Pa, 0.0) + (u - mu[j]) * (ndtr(be) - Pa) + sd[j] * (_pdf(be) - pa))
        Tm.append(-(ndtr(be) - Pa))
        Ts.append(_pdf(be) - pa)
    dm, dv = np.zeros_like(mu), np.zeros_like(mu)
    for j in range(k):
        others = np.prod([T[i] for i in range(k) if i != j], axis=0) if k > 1 else 1.0
        dm[j] = (others * Tm[j]).sum(0)
        dv[j] = (others * Ts[j]).sum(0) / (2.0 * sd[j])
    return dm, dv


def eval_grad(gps, Xc, partials):
    """(grad (N, d), scale (N, d)): the chain rule Σ_o ∂a/∂μ_o ∂μ_o/∂x + ∂a/∂σ²_o ∂σ²_o/∂x and the sum of its
    terms' magnitudes over objectives and training rows.  partials(mu, var) → (∂a/∂μ, ∂a/∂σ²) (k, N)."""
    pg = [posterior_grad(g, Xc) for g in gps]
    mu, var = np.array([p[0] for p in pg]), np.array([p[1] for p in pg])
    dm, dv = partials(mu, var)
    grad = sum(dm[o][:, None] * pg[o][2] + dv[o][:, None] * pg[o][3] for o in range(len(gps)))
    scale = sum(np.abs(dm[o])[:, None] * pg[o][4] + np.abs(dv[o])[:, None] * pg[o][5] for o in range(len(gps)))
    return grad, scale


# ----------------------------------------------------------------------------------------------- acquisitions
def front(k, P=6, seed=3):
    """A P-point non-dominated front on the unit sphere's positive orthant and r = 1.2."""
    from oracle import pareto as opar
    rng = np.random.default_rng(10 * k + P + seed)
    pts = rng.uniform(0.05, 1, (60 * P, k))
    pts /= np.linalg.norm(pts, axis=1, keepdims=True)
    pf = opar.calc_pf(pts)[:P]
    assert len(pf) == P
    return pf, np.full(k, 1.2)


def acq_gps(k, n=17, d=3, kernel="matern52", centre=0.5):
    """k surrogates with targets centre + 0.3·(make_gp's signal): around the fronts' range for centre = 0.5; the
    constraint models of constrained EI (objectives 1..) are centred on 0, so that Φ(−μ/σ) is neither 0 nor 1."""
    gps = []
    for o in range(k):
        g = make_gp(n, d, kernel, seed=5, obj=o)
        c = centre if np.isscalar(centre) else centre[o]
        gps.append(ogp.ExactGP(g.X, c + 0.3 * g.y[:, 0], g.lengthscale, 0.05 + 0.02 * o, kernel=kernel,
                               noise=g.noise))
    return gps


def case_gps(name, k):
    return acq_gps(k, centre=[0.5, 0.0, 0.0] if name == "constrained_ei" else 0.5)


def box_lists(pf, r):
    from optimobo_amd import pareto
    coords, _, boxes = pareto.box_decomposition(pf, r)
    k = coords.shape[0]
    lo = np.stack([coords[j][boxes[:, 2 * j]] for j in range(k)], 1)
    hi = np.stack([coords[j][boxes[:, 2 * j + 1]] for j in range(k)], 1)
    return coords, boxes, lo, hi


@functools.lru_cache(maxsize=None)
def acquisition_cases():
    """name → (k, value(mu, var) on the oracle, partials(mu, var), plan(ctx) for the GPU tests); built once and
    shared read-only."""
    rng = np.random.default_rng(11)
    cache = rng.normal(size=(64, 2))
    cache[:, 1] = 0.6 * cache[:, 0] + 0.8 * cache[:, 1]     # reference mode uses Cov(cache)01 as a σ: keep it > 0
    s00, s01 = oacq.cache_stats(cache)
    cases = {
        "ei": (1, lambda m, v: oacq.ei(m[0], v[0], 0.55, 0.0), lambda m, v: ei_partials(m, v, 0.55, 0.0),
               lambda c: c.plan_ei(0.55, 0.0)),
        "ei_eps": (1, lambda m, v: oacq.ei(m[0], v[0], 0.55, 1e-6), lambda m, v: ei_partials(m, v, 0.55, 1e-6),
                   lambda c: c.plan_ei_ext("plain", 1, 0.55, 1e-6)),
        "pareto_ei": (2, lambda m, v: oacq.pareto_ei(m, v, 0.55, 1e-6),
                      lambda m, v: ei_partials(m, v, 0.55, 1e-6, "pareto"),
                      lambda c: c.plan_ei_ext("pareto", 2, 0.55, 1e-6)),
        "constrained_ei": (3, lambda m, v: oacq.constrained_ei(m, v, 0.55, 0.0, 1e-5),
                           lambda m, v: ei_partials(m, v, 0.55, 0.0, "constrained", 1e-5),
                           lambda c: c.plan_ei_ext("constrained", 3, 0.55, 0.0, 1e-5)),
    }
    # P = 64, 65, 130: ehvi2d_grad_kernel strides the stripes by the 64 lanes of a wavefront — one full pass, one pass
    # and a single stripe, two passes and a ragged third
    for P in (1, 9, 64, 65, 130):
        pf, r = front(2, P)
        order = np.argsort(pf[:, 1])
        for mode in ("reference", "textbook"):
            cases[f"ehvi2d_{mode}_P{P}"] = (
                2, lambda m, v, pf=pf, r=r, mode=mode: oacq.ehvi2d(m, v, pf, r, cache, mode=mode),
                lambda m, v, pf=pf, r=r, mode=mode: ehvi2d_partials(m, v, pf, r, s00, s01, mode),
                lambda c, pf=pf, r=r, mode=mode, order=order: c.plan_ehvi2d(pf[order], r, s00, s01, mode=mode))
    # every instantiation of ehvi_boxes_grad_kernel<K>; "boxes_k2_long": a list the 256 threads of a workgroup need a
    # second, ragged pass over (thread t takes boxes t, t + 256, …)
    for name, k, P in [(f"boxes_k{k}", k, 6) for k in (2, 3, 4, 5, 6, 7, 8)] + [("boxes_k2_long", 2, 300)]:
        pf, r = front(k, P)
        coords, boxes, lo, hi = box_lists(pf, r)
        if name == "boxes_k2_long":
            assert len(boxes) > 256 and len(boxes) % 64 != 0, len(boxes)
        cases[name] = (k, lambda m, v, lo=lo, hi=hi: oacq.ehvi_exact_boxes(m, v, lo, hi),
                       lambda m, v, lo=lo, hi=hi: boxes_partials(m, v, lo, hi),
                       lambda c, coords=coords, boxes=boxes: c.plan_ehvi_boxes(coords, boxes))
    return cases


# ----------------------------------------------------------------------------------------------- finite differences
def richardson(f, X, h):
    """Fourth-order central differences of f: (N, d) → (N,) along every coordinate: (N, d)."""
    N, d = X.shape
    out = np.zeros((N, d))
    for j in range(d):
        e = np.zeros(d)
        e[j] = h
        out[:, j] = (8.0 * (f(X + e) - f(X - e)) - (f(X + 2 * e) - f(X - 2 * e))) / (12.0 * h)
    return out


def fd_error(an, fd, scale):
    """max |analytic − FD| / Σ|terms| over the entries with a non-zero term sum; where every term is exactly 0 the
    analytic gradient must be exactly 0."""
    z = scale == 0.0
    assert np.all(an[z] == 0.0)
    return float(np.max(np.where(z, 0.0, np.abs(an - fd) / np.where(z, 1.0, scale)), initial=0.0))


# The finite differences run at candidates away from the training set.  At a training point σ² ≈ 1e-8 is what is
# left of σ_f² − ‖L⁻¹k‖² after cancellation, its gradient and every term of it are of that order too, and a difference
# quotient of predict's σ² there is rounding alone; the restatement has no such cancellation (direct differences, r = 0
# is an ordinary point of g), and the GPU tests do include a training point.
H_FD = 1e-3        # posterior: truncation (∝ h⁴) and rounding (∝ 1/h) both below 1e-7 of the term sum at every shape
H_FD_ACQ = 6e-5    # acquisitions: Φ, φ of (· − μ)/σ with σ down to 0.01 near the data have large fifth derivatives
                   # (the error falls as h⁴ from 3e-5 of the term sum at h = 5e-4 to 6e-9 here; rounding ≈ 1e-10)


@pytest.mark.parametrize("kernel", ["matern52", "rbf"])
@pytest.mark.parametrize("n,d", SHAPES)
def test_surrogates_are_well_conditioned(n, d, kernel):
    gp = make_gp(n, d, kernel)
    assert np.all(gp.lengthscale >= 0.3) and np.all(gp.lengthscale <= 1.0)
    c = cond_K(gp)
    print(f"n={n} d={d} {kernel}: cond(K) = {c:.3g}")
    assert c <= 1e8


@pytest.mark.parametrize("kernel", ["matern52", "rbf"])
@pytest.mark.parametrize("n,d", SHAPES)
def test_posterior_gradient_vs_richardson(n, d, kernel):
    gp = make_gp(n, d, kernel)
    for N in BATCHES:
        Xc = make_candidates(gp, N, train_point=False)
        mu, var, dmu, dvar, smu, svar = posterior_grad(gp, Xc)
        pm, pv = gp.predict(Xc)
        np.testing.assert_allclose(mu, pm[:, 0], rtol=0, atol=1e-9 * np.abs(gp.alpha).sum() * gp.variance)
        np.testing.assert_allclose(var, pv[:, 0] - gp.noise, rtol=0, atol=1e-7 * gp.variance)
        em = fd_error(dmu, richardson(lambda X: gp.predict(X)[0][:, 0], Xc, H_FD), smu)
        ev = fd_error(dvar, richardson(lambda X: gp.predict(X)[1][:, 0], Xc, H_FD), svar)
        print(f"n={n} d={d} {kernel} N={N}: worst |analytic - FD| / sum|terms|: dmu {em:.2e} dvar {ev:.2e}")
        assert em <= FD_BAR and ev <= FD_BAR


@pytest.mark.parametrize("kernel", ["matern52", "rbf"])
@pytest.mark.parametrize("n,d", SHAPES)
def test_gradient_at_a_training_point_is_finite(n, d, kernel):
    gp = make_gp(n, d, kernel)
    out = posterior_grad(gp, make_candidates(gp, 7))
    assert all(np.all(np.isfinite(o)) for o in out)
    assert abs(out[1][0]) <= 1e-4 * gp.variance + 2 * gp.noise     # σ² at the training point


@pytest.mark.parametrize("name", sorted(acquisition_cases()))
def test_acquisition_gradient_vs_richardson(name):
    k, value, partials, _ = acquisition_cases()[name]
    gps = case_gps(name, k)
    Xc = make_candidates(gps[0], 33, train_point=False)

    def a_of_x(X):
        pm = [g.predict(X) for g in gps]
        mu = np.array([p[0][:, 0] for p in pm])
        var = np.array([p[1][:, 0] - g.noise for p, g in zip(pm, gps)])
        return value(mu, var)

    grad, scale = eval_grad(gps, Xc, partials)
    assert np.all(np.isfinite(a_of_x(Xc))) and np.all(np.isfinite(grad))
    err = fd_error(grad, richardson(a_of_x, Xc, H_FD_ACQ), scale)
    print(f"{name}: worst |analytic - FD| / sum|terms| = {err:.2e}, |grad| up to {np.abs(grad).max():.3g}, "
          f"{(np.abs(grad).max(1) > 0).sum()} of 33 rows non-zero")
    assert err <= FD_BAR
    assert (np.abs(grad).max(1) > 0).sum() >= 20
