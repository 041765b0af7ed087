"""GPU: μ of the objectives whose variance the planned acquisition never reads comes from posterior_mean_kernel, a
launch of its own (n_var ≤ 8, some n_train > 128), and keeps every bit.

For every ring instantiation of the fused posterior at n_var ≤ 8 (n_train 130 → 2 row tiles per wave, 257 and 300 → 4,
520 and 1000 → 8; 130, 300 and 1000 leave a part-filled last chunk) at n_var 2, 5 (d < DP), 6 and 8 in both covariance
kinds (_shapes), N = 7 (less than one column of 16 candidates), 17 and 1003, and for objectives of different sizes
(the masked objective smaller than, larger than and far smaller than the one whose variance is computed), with
reference-mode EHVI-2D and a 3-objective expected-decomposition plan:
  * the chain's values and arg-max pair are bit for bit the same with the mean kernel after the posterior launch
    (default), before it, switched off (debug switch "posterior_mean_kernel" = 0: the in-kernel mean-only path) and
    with every variance computed ("posterior_all_var" = 1).  Before each of them the chain runs on other candidates,
    so a μ the mean kernel failed to write would be a stale number;
  * the values match the oracle's acquisition on the oracle's own posterior at tests/test_gpu_fused.py's tolerance;
  * no call marks the context's fault word (synchronize raises on it).
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import acquisition as oacq  # noqa: E402
from oracle import gp as ogp  # noqa: E402
from oracle import pareto as opar  # noqa: E402
from oracle import scalarisations as osc  # noqa: E402

N_CANDS = (7, 17, 1003)
N_GEO = 40
N_TRAIN = (130, 257, 300, 520, 1000)
N_VAR = (2, 5, 6, 8)
KINDS = ("matern52", "rbf")
# (posterior_mean_kernel, posterior_all_var); the first is the default
CONFIGS = ((1, 0), (2, 0), (0, 0), (1, 1))


@pytest.fixture(scope="module")
def ctx():
    from optimobo_amd.device import AcqContext
    c = AcqContext(0)
    yield c
    c.debug_set("posterior_all_var", 0)
    c.debug_set("posterior_mean_kernel", 1)
    c.close()


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device="cuda:0")


def _objectives(X):
    f1 = X[:, 0]
    g = 1 + 9.0 / (X.shape[1] - 1) * X[:, 1:].sum(1)
    return np.column_stack([f1, g * (1 - np.sqrt(f1 / g)), (1 + X[:, 1]) * (1.2 - f1)])


def _lengthscales(rng, n, d, kind):
    """A few nearest-neighbour spacings of n uniform points in [0, 1]^d per dimension (tests/test_gpu_var_mask.py's
    choice for Matérn 5/2); the squared exponential gets half of that, since its K(X, X) loses rank far sooner:
    K stays well enough conditioned for the oracle's triangular solve and the device's L⁻¹ product to agree far
    inside the acquisition tolerance."""
    scale = 1.0 if kind == "matern52" else 0.5
    return scale * rng.uniform(1.0, 2.0, d) * np.sqrt(d) * n ** (-1.0 / d)


def _problem(ns, d, kind, seed):
    """Three objectives with n_train = ns[o] (their own inputs), candidates, and the oracle's posterior."""
    rng = np.random.default_rng(seed)
    Xc = rng.uniform(0, 1, (max(N_CANDS), d))
    gps, mu, var, Y0 = [], [], [], None
    for o, n in enumerate(ns):
        X = rng.uniform(0, 1, (n, d))
        Y = _objectives(X)
        if Y0 is None:
            Y0 = Y[:N_GEO]
        ls = _lengthscales(rng, n, d, kind)
        vf = float(np.var(Y[:, o]))
        gps.append((X, Y[:, o], ls, vf))
        m, v = ogp.ExactGP(X, Y[:, o], ls, vf, kernel=kind).predict(Xc)
        mu.append(m[:, 0])
        var.append(v[:, 0])
    return gps, Y0, Xc, np.array(mu), np.array(var)


def _set_gps(ctx, gps, kind):
    from optimobo_amd.gp import GPState
    for o, (X, y, ls, vf) in enumerate(gps):
        ctx.set_gp_state(o, GPState(X, y, ls, vf, kernel=kind))


def _plans(ctx, Y):
    """(name, k, set_plan(), oracle(mu, var) -> vals): both mask every objective but the first."""
    from optimobo_amd import pareto
    rng = np.random.default_rng(0)
    pf2 = opar.calc_pf(Y[:, :2])
    r2 = Y[:, :2].max(0) + 0.1
    cache2 = rng.standard_normal((32, 2))
    s00, s01 = oacq.cache_stats(cache2)
    stripes = pareto.stripes_2d(pf2)
    cache3 = rng.standard_normal((32, 3))
    tch = osc.Tchebicheff(Y.min(0), Y.max(0))
    w3 = np.array([0.2, 0.5, 0.3])
    return [
        ("ehvi2d-reference", 2, lambda: ctx.plan_ehvi2d(stripes, r2, s00, s01, mode="reference"),
         lambda mu, var: oacq.ehvi2d(mu[:2], var[:2], pf2, r2, cache2, mode="reference")),
        ("expdec-tch", 3, lambda: ctx.plan_expdec(cache3, 1, [], w3, Y.min(0), Y.max(0), 0.4),
         lambda mu, var: oacq.expected_decomposition(mu, var, cache3, tch, w3, 0.4)),
    ]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _chain(ctx, Xd, Xstale, mean_kernel, all_var):
    """Values and arg-max pair of the planned chain under one configuration, after a chain on other candidates that
    computes everything; synchronize raises if a call marked the fault word."""
    ctx.debug_set("posterior_all_var", 1)
    ctx.eval(Xstale).cpu()
    ctx.debug_set("posterior_mean_kernel", mean_kernel)
    ctx.debug_set("posterior_all_var", all_var)
    vals = ctx.eval(Xd).cpu().numpy()
    ctx.synchronize()
    pair = ctx.eval_argmax(Xd, offset=7).cpu().numpy()
    ctx.synchronize()
    return vals, pair


def _check(ctx, Y, Xc, mu_o, var_o, n_cands, tag):
    try:
        for name, k, plan, oracle in _plans(ctx, Y):
            plan()
            for N in n_cands:
                Xd, Xstale = dev(Xc[:N]), dev(Xc[::-1][:N])
                vals, pair = _chain(ctx, Xd, Xstale, *CONFIGS[0])
                for cfg in CONFIGS[1:]:
                    vals_c, pair_c = _chain(ctx, Xd, Xstale, *cfg)
                    assert np.array_equal(_bits(vals), _bits(vals_c)), (tag, name, N, cfg)
                    assert np.array_equal(_bits(pair), _bits(pair_c)), (tag, name, N, cfg, pair, pair_c)
                v, i = oacq.argmax(vals, offset=7)
                assert (pair[0], int(pair[1])) == (v, i), (tag, name, N)
                np.testing.assert_allclose(vals, oracle(mu_o[:k, :N], var_o[:k, :N]), rtol=1e-7, atol=1e-11,
                                           equal_nan=True, err_msg=f"{tag} {name} N={N}")
    finally:
        ctx.debug_set("posterior_all_var", 0)
        ctx.debug_set("posterior_mean_kernel", 1)


def _shapes():
    """Every (ring instantiation, padded n_var, kind): both kinds at n_train 130; the kinds alternating over n_var
    at 257 against 300 and at 520 against 1000, the costliest size (its oracle takes a second) at n_var 5 and 8 only."""
    out = [(130, d, kind) for d in N_VAR for kind in KINDS]
    for i, d in enumerate(N_VAR):
        out += [(257, d, KINDS[i % 2]), (300, d, KINDS[(i + 1) % 2]), (520, d, KINDS[i % 2])]
        out += [(520, d, KINDS[(i + 1) % 2])] if d in (2, 6) else [(1000, d, KINDS[(i + 1) % 2])]
    return out


@pytest.mark.parametrize("n,d,kind", _shapes())
def test_mean_kernel_keeps_every_bit(ctx, n, d, kind):
    gps, Y, Xc, mu_o, var_o = _problem((n, n, n), d, kind, 1000 * n + d)
    _set_gps(ctx, gps, kind)
    _check(ctx, Y, Xc, mu_o, var_o, N_CANDS, f"n={n} d={d} {kind}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ns", [(300, 130, 130), (130, 520, 100), (520, 20, 100)])
def test_mean_kernel_mixed_training_sizes(ctx, ns, kind):
    """The ring instantiation follows the largest n_train of all objectives, masked ones included; each masked
    objective's mean runs over its own chunks."""
    gps, Y, Xc, mu_o, var_o = _problem(ns, 6, kind, sum(ns))
    _set_gps(ctx, gps, kind)
    _check(ctx, Y, Xc, mu_o, var_o, (17, 1003), f"ns={ns} {kind}")
