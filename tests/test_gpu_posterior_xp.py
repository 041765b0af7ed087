"""GPU: the posterior near the data — omb_posterior, omb_posterior_cov and omb_gp_append against the np.longdouble
evaluation of their contract on the installed bits (tests/_posterior_xp.py), on late-run states:
clustered training rows, K + 1e-8·I as ill-conditioned as the jitter allows, candidates on and between training
rows where σ² is 1e-9 to 1e-12 of σ_f² — below the absolute tolerance of the parity suites.

Error measure: e = |device − reference| / (u·S), u = 2⁻⁵³, S the first-order rounding scale of the result
(``scales``): e counts roundings.  Bar: e ≤ T, T = 4 × the worst e of the plain fp64 numpy restatement over the
whole case table (computed at run time, ≈ 2.6 for μ and ≈ 10.3 for σ²).  A case that needs more from honest
rounding gets an entry in OVERRIDE (4 × the value measured on the MI355X, its cause in DESIGN §20); no entry may
exceed the ceiling n + d + 16, the first-order worst-case count of roundings.

Far candidates (50 + 100·U): σ² is σ_f² bitwise.  Their Matern kernel values are tiny but not 0 (the reference's
|μ| reaches 5e-125·Σ|α|), so μ is held to the reference there, within 1e-290·Σ|α| plus the relative error an fp64
exp(−√5 r) has at that depth; where every kernel value underflows (RBF) that is |μ| ≤ 1e-290·Σ|α|.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]

import _posterior_xp as xp  # noqa: E402

LD = np.longdouble
# (n, d, kernel) → (T_μ, T_σ²) where the bar is not reached by honest rounding
OVERRIDE = {}
CONSUMER_CASES = [(50, 4, "matern52"), (130, 6, "matern52"), (1040, 6, "matern52"), (40, 70, "matern52"),
                  (130, 6, "rbf")]
ids = lambda c: f"n{c[0]}-d{c[1]}-{c[2]}"  # noqa: E731


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


def bar(n, d, kernel):
    t = OVERRIDE.get((n, d, kernel), xp.bar())
    assert max(t) <= xp.ceiling(n, d), (t, xp.ceiling(n, d))
    return t


def worst(e):
    j = int(np.argmax(e))
    return float(e[j]), xp.group_of(j % xp.N_CAND)


def check_moments(label, st, mu, var, ref, S, t_mu, t_var, groups=1):
    """μ, σ² (N,) of one objective against its reference: the bar, finiteness, the far rows, the sign of σ²."""
    mu_r, var_r = ref[0], ref[1]
    s_mu, s_var = S
    e_mu, e_var = xp.normalised(mu, mu_r, s_mu), xp.normalised(var, var_r, s_var)
    (wm, gm), (wv, gv) = worst(e_mu), worst(e_var)
    print(f"{label}: worst e_mu {wm:.2f} ({gm})  worst e_var {wv:.2f} ({gv})   [T {t_mu:.2f} / {t_var:.2f}]")
    assert np.all(np.isfinite(mu)) and np.all(np.isfinite(var))
    n, d = st.X.shape
    sum_alpha = np.abs(st.alpha).sum()
    for g in range(groups):
        far = slice(g * xp.N_CAND + xp.FAR.start, g * xp.N_CAND + xp.FAR.stop)
        assert np.array_equal(var[far], np.full(4, st.variance)), var[far] - st.variance
        # |μ| ≤ 1e-290·Σ|α| where every kernel value underflows; where the reference's does not (Matern at these
        # distances: down to exp(−290)), μ is held to the reference within the relative error an fp64 exp(−√5 r)
        # has there: |x|·(d + 8)·u from r², |x| ≤ 895 before k is 0, twice for the polynomial and the sum
        rel = 2.0 * 895.0 * (d + 8) * xp.U
        k_sum = np.asarray(np.abs(np.asarray(st.alpha, np.float64).reshape(-1).astype(LD)) @ np.abs(ref[2][:, far]), np.float64)
        assert np.all(np.abs(np.asarray(mu[far].astype(LD) - mu_r[far], np.float64)) <= 1e-290 * sum_alpha + rel * k_sum), \
            (mu[far], mu_r[far])
    assert np.all(e_mu <= t_mu), (wm, gm)
    assert np.all(e_var <= t_var), (wv, gv)
    sure = np.asarray(var_r > LD(t_var) * LD(xp.U) * s_var)
    assert np.all(var[sure] > 0.0)
    return wm, wv


# ----------------------------------------------------------------------------- omb_posterior, every launch path
@pytest.mark.parametrize("kernel", xp.KERNELS)
@pytest.mark.parametrize("n,d", xp.CASES)
def test_posterior(ctx, n, d, kernel):
    t_mu, t_var = bar(n, d, kernel)
    cases = [xp.case(n, d, kernel, o) for o in range(2)]
    for o, c in enumerate(cases):
        ctx.set_gp_state(o, c[0])
    Xc = dev(cases[0][1])
    mu, var = ctx.posterior(Xc, 2)
    mu2, var2 = ctx.posterior(Xc, 2)
    assert np.array_equal(bits(mu), bits(mu2)) and np.array_equal(bits(var), bits(var2))
    mu, var = mu.cpu().numpy(), var.cpu().numpy()
    for o, (st, _, ref, S) in enumerate(cases):
        check_moments(f"n={n} d={d} {kernel} obj={o}", st, mu[o], var[o], ref, S, t_mu, t_var)


# ----------------------------------------------------------------------------- mixed n_train in one call
@pytest.mark.parametrize("kernel", xp.KERNELS)
@pytest.mark.parametrize("pair", [((1040, 6), (20, 6)), ((300, 6), (50, 6))], ids=["dense-1040+20", "ring-300+50"])
def test_mixed_n_train(ctx, pair, kernel):
    """Objectives of different n_train in one omb_posterior call, each held to its own reference, on both
    objectives' candidate sets (so each sees candidates on its own training rows)."""
    sts = [xp.late_run_state(n, d, kernel, obj=o) for o, (n, d) in enumerate(pair)]
    Xc = np.vstack([xp.candidates(st, np.random.default_rng(31 + o)) for o, st in enumerate(sts)])
    for o, st in enumerate(sts):
        ctx.set_gp_state(o, st)
    mu, var = ctx.posterior(dev(Xc), 2)
    mu2, var2 = ctx.posterior(dev(Xc), 2)
    assert np.array_equal(bits(mu), bits(mu2)) and np.array_equal(bits(var), bits(var2))
    mu, var = mu.cpu().numpy(), var.cpu().numpy()
    for o, st in enumerate(sts):
        n, d = st.X.shape
        t_mu, t_var = bar(n, d, kernel)
        ref = xp.reference(st, Xc, kernel)
        S = xp.scales(st, Xc, kernel, ref[2], ref[3])
        check_moments(f"mixed {pair} {kernel} obj={o} (n={n})", st, mu[o], var[o], ref, S, t_mu, t_var, groups=2)


# ----------------------------------------------------------------------------- other consumers of the same state
@pytest.mark.parametrize("case", CONSUMER_CASES, ids=ids)
def test_posterior_cov(ctx, case):
    n, d, kernel = case
    t_mu, t_var = bar(n, d, kernel)
    st, Xc, ref, S = xp.case(n, d, kernel)
    ctx.set_gp_state(0, st)
    mu, cov = ctx.posterior_cov(0, dev(Xc))
    mu, cov = mu.cpu().numpy(), cov.cpu().numpy()
    assert np.all(np.isfinite(cov))
    check_moments(f"cov n={n} d={d} {kernel}: mean and diagonal", st, mu, np.diag(cov).copy(), ref, S, t_mu, t_var)
    rows = np.arange(16)
    cov_r = xp.reference_cov(st, Xc, kernel, ref[3], rows)
    S_ij = xp.scales_cov(st, Xc, kernel, ref[2], ref[3], rows)
    for name, block in (("rows", cov[rows]), ("columns", cov[:, rows].T)):
        e = xp.normalised(block, cov_r, S_ij)
        i, j = np.unravel_index(int(np.argmax(e)), e.shape)
        print(f"cov n={n} d={d} {kernel}: {name} 0..15: worst e {e[i, j]:.2f} at ({xp.group_of(i)}, {xp.group_of(j)})"
              f"   [T {t_var:.2f}]")
        assert np.all(e <= t_var), (name, i, j, e[i, j])


@pytest.mark.parametrize("case", CONSUMER_CASES, ids=ids)
def test_gp_append(ctx, case):
    """omb_gp_append's predictive mean and δ² = σ² + 1e-8 of one point (q = 1, the Kriging believer, noise 0)."""
    n, d, kernel = case
    t_mu, t_var = bar(n, d, kernel)
    st, Xc, (mu_r, var_r, _, _), (s_mu, s_var) = xp.case(n, d, kernel)
    used = 0
    for j in (8, 16, 24):                          # a training row + 1e-6, an in-cluster point, a uniform point
        d2_r = var_r[j] + LD(1e-8)
        if not d2_r > 100 * LD(xp.U) * s_var[j]:     # OMB_ENOTPD must not be a rounding accident
            continue
        used += 1
        ctx.set_gp_state(0, st)
        mu_out, d2 = ctx.gp_append(0, Xc[j:j + 1], None, noise=0.0)
        assert ctx.gp_info[0]["n"] == n + 1
        e_mu = float(xp.normalised(mu_out, mu_r[j:j + 1], s_mu[j:j + 1])[0])
        e_d2 = float(xp.normalised(d2, np.array([d2_r]), s_var[j:j + 1])[0])
        print(f"append n={n} d={d} {kernel} point {j} ({xp.group_of(j)}): delta2 / sf2 {float(d2_r) / st.variance:.2e}  "
              f"e_mu {e_mu:.2f} e_delta2 {e_d2:.2f}   [T {t_mu:.2f} / {t_var:.2f}]")
        assert np.isfinite(mu_out[0]) and d2[0] > 0.0
        assert e_mu <= t_mu and e_d2 <= t_var
    assert used == 3
