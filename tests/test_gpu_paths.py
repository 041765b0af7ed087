"""GPU: posterior sample paths (omb_paths_set / omb_paths_eval) against the np.longdouble restatement of
tests/_paths_reference.py on the installed bits, the mean path, the bitwise properties, the paths' statistics, and the
return codes and coherence rule of the two entry points."""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _paths_reference as pr  # noqa: E402

from optimobo_amd import _lib, paths  # noqa: E402
from optimobo_amd._lib import OMB_EINVAL, OMB_ESTATE, OMB_EUNSUP, OMBError  # noqa: E402

# (n, d, m, S, N, kernel, k, reach): the tile and padding edges of every size, each at least once; reach: one
# frequency row scaled until its argument reaches about that over the candidates (inside the 2^20 contract)
CASES = [
    (1, 1, 1, 1, 1, "matern52", 1, None),
    (15, 2, 4, 3, 15, "rbf", 1, None),
    (16, 6, 17, 16, 17, "matern52", 2, None),
    (17, 8, 1024, 3, 1000, "matern52", 1, None),
    (63, 9, 17, 1, 17, "rbf", 1, None),
    (65, 30, 4, 16, 15, "matern52", 1, None),
    (130, 64, 17, 3, 17, "matern52", 1, None),
    (300, 6, 1024, 16, 1000, "matern52", 3, None),
    (130, 6, 1024, 16, 17, "rbf", 2, None),
    (300, 2, 1, 3, 1, "rbf", 1, None),
    (17, 1, 1024, 16, 15, "rbf", 1, None),
    (1, 8, 17, 3, 17, "matern52", 1, None),
    (63, 30, 1024, 1, 17, "rbf", 1, None),
    (65, 64, 4, 16, 1, "rbf", 1, None),
    (16, 9, 4, 1, 1000, "matern52", 2, None),
    (15, 6, 17, 16, 17, "matern52", 3, None),
    (130, 2, 1024, 3, 15, "matern52", 1, None),
    (300, 8, 17, 1, 17, "rbf", 1, None),
    (40, 2, 64, 3, 17, "matern52", 1, 1e3),
    (40, 6, 64, 3, 17, "rbf", 1, 1e5),
]
NOISE = 1e-6


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def case(i):
    """Inputs and references of case i, computed once and shared read-only: per objective the state and the draws,
    the candidates, the longdouble values and term sums (k, S, N), and the fp64 restatement's normalised error."""
    n, d, m, S, N, kernel, k, reach = CASES[i]
    rng = np.random.default_rng(9000 + i)
    Xc = rng.uniform(0.0, 1.0, (N, d))
    states, draws, ref, T, worst = [], [], [], [], 0.0
    for o in range(k):
        st = pr.make_state(n, d, kernel, seed=100 * i + o, noise=NOISE, obj=o)
        omega, phase, w, z = paths.draw_path_inputs(kernel, n, d, S, m, rng, np.zeros(d), np.ones(d), st.lengthscale)
        if reach is not None:
            omega[0] *= reach / np.abs((Xc / st.lengthscale) @ omega[0]).max()
            assert paths.worst_argument(omega, np.zeros(d), np.ones(d), st.lengthscale).max() <= paths.MAX_ARGUMENT
        f, t, _ = pr.reference(st, kernel, omega, phase, w, z, NOISE, Xc)
        f64, _ = pr.restatement(st, kernel, omega, phase, w, z, NOISE, Xc)
        worst = max(worst, float(pr.normalised(f64, f, t).max()))
        states.append(st)
        draws.append((omega, phase, w, z))
        ref.append(f)
        T.append(t)
    Xc.setflags(write=False)
    return states, draws, Xc, np.stack(ref), np.stack(T), worst


@functools.lru_cache(maxsize=None)
def bar():
    """4 × the worst normalised error of the plain-fp64 numpy evaluation over the whole table."""
    return 4.0 * max(case(i)[5] for i in range(len(CASES)))


@pytest.fixture(scope="module")
def ctx():
    from optimobo_amd.device import AcqContext
    c = AcqContext(0)
    yield c
    c.close()


def _install(ctx, states, draws, kernel, noise=NOISE):
    for o, (st, (omega, phase, w, z)) in enumerate(zip(states, draws)):
        ctx.set_gp(o, st.X, st.lengthscale, st.variance, st.alpha, st.Linv, kernel=kernel)
        ctx.paths_set(o, omega, phase, w, z, noise=noise)


@pytest.mark.parametrize("i", range(len(CASES)))
def test_values_against_the_longdouble_restatement(ctx, i):
    n, d, m, S, N, kernel, k, reach = CASES[i]
    states, draws, Xc, ref, T, worst = case(i)
    _install(ctx, states, draws, kernel)
    out = torch.full((k, S, N + 3), -7.25, dtype=torch.float64, device=ctx.device)
    got = ctx.paths_eval(torch.as_tensor(np.array(Xc), device=ctx.device), k, out=out).cpu().numpy()
    assert np.all(got[:, :, N:] == -7.25)                      # ld = N + 3: nothing past N is written
    err = float(pr.normalised(got[:, :, :N], ref, T).max())
    print(f"case {i} n={n} d={d} m={m} S={S} N={N} {kernel} k={k} reach={reach}: device {err:.3e}, fp64 numpy "
          f"{worst:.3e}, bar {bar():.3e} (term-sum units); device / table-worst numpy = {4 * err / bar():.3f}")
    assert np.all(np.isfinite(got[:, :, :N]))
    assert err <= bar()
    # without out: a (k, S, N) tensor of the same bits
    plain = ctx.paths_eval(torch.as_tensor(np.array(Xc), device=ctx.device), k).cpu().numpy()
    assert plain.shape == (k, S, N) and np.array_equal(bits(plain), bits(got[:, :, :N]))


def test_library_cosine_variant_agrees(ctx):
    """The debug switch's library cosine gives the same values to the cosines' rounding (and passes the same bar)."""
    i = 3
    n, d, m, S, N, kernel, k, _ = CASES[i]
    states, draws, Xc, ref, T, _ = case(i)
    ctx.debug_set("paths_libcos", 1)
    try:
        _install(ctx, states, draws, kernel)
        got = ctx.paths_eval(torch.as_tensor(np.array(Xc), device=ctx.device), k).cpu().numpy()
    finally:
        ctx.debug_set("paths_libcos", 0)
    assert float(pr.normalised(got, ref, T).max()) <= bar()


@pytest.mark.parametrize("kernel,n,d", [("matern52", 130, 6), ("rbf", 65, 9), ("matern52", 300, 30)])
def test_mean_path_is_the_posterior_mean(ctx, kernel, n, d):
    """w = 0 and z = None: U = 0, V = α, and every path is μ — to μ's own bar (1e-6 relative, floor 1e-7·σ_f)."""
    st = pr.make_state(n, d, kernel, seed=n + d)
    rng = np.random.default_rng(n)
    omega, phase, w, _ = paths.draw_path_inputs(kernel, n, d, 16, 33, rng)
    ctx.set_gp(0, st.X, st.lengthscale, st.variance, st.alpha, st.Linv, kernel=kernel)
    ctx.paths_set(0, omega, phase, np.zeros_like(w), None, noise=0.0)
    Xc = torch.as_tensor(rng.uniform(0.0, 1.0, (100, d)), device=ctx.device)
    f = ctx.paths_eval(Xc, 1).cpu().numpy()[0]
    mu = ctx.posterior(Xc, 1)[0].cpu().numpy()[0]
    tol = 1e-6 * np.abs(mu) + 1e-7 * np.sqrt(st.variance)
    assert f.shape == (16, 100) and np.all(np.abs(f - mu[None, :]) <= tol[None, :])
    from oracle import gp as ogp
    mu_o = ogp.KERNELS[kernel](Xc.cpu().numpy(), st.X, st.lengthscale, st.variance) @ st.alpha.reshape(-1)
    assert np.all(np.abs(f - mu_o[None, :]) <= (1e-6 * np.abs(mu_o) + 1e-7 * np.sqrt(st.variance))[None, :])


def test_bitwise_properties(ctx):
    """A path's value at a point depends on the point and the installed state alone; the plan and the GP states are
    not touched."""
    i = 7
    n, d, m, S, N, kernel, k, _ = CASES[i]
    states, draws, Xc, _, _, _ = case(i)
    for o, st in enumerate(states):
        ctx.set_gp(o, st.X, st.lengthscale, st.variance, st.alpha, st.Linv, kernel=kernel)
    Y = np.stack([st.y.reshape(-1) for st in states], 1)
    from optimobo_amd import pareto
    coords, _, boxes = pareto.box_decomposition(pareto.calc_pf(Y), Y.max(0) + 0.1)
    ctx.plan_ehvi_boxes(coords, boxes)
    Xd = torch.as_tensor(np.array(Xc), device=ctx.device)
    before = ctx.eval(Xd).cpu().numpy()
    mu0 = [t.cpu().numpy() for t in ctx.posterior(Xd, k)]
    for o, (omega, phase, w, z) in enumerate(draws):
        ctx.paths_set(o, omega, phase, w, z, noise=NOISE)
    full = ctx.paths_eval(Xd, k).cpu().numpy()
    assert np.array_equal(bits(ctx.paths_eval(Xd, k).cpu().numpy()), bits(full))          # across two calls
    for c in (0, 16, 999):
        one = ctx.paths_eval(Xd[c:c + 1], k).cpu().numpy()                                  # N = 1, column 0
        assert np.array_equal(bits(one[:, :, 0]), bits(full[:, :, c]))
        block = torch.cat([Xd[5:21], Xd[c:c + 1]])                                          # N = 17, column 16
        assert np.array_equal(bits(ctx.paths_eval(block, k).cpu().numpy()[:, :, 16]), bits(full[:, :, c]))
        front = torch.cat([Xd[c:c + 1], Xd[100:137]])                                       # N = 38, column 0
        assert np.array_equal(bits(ctx.paths_eval(front, k).cpu().numpy()[:, :, 0]), bits(full[:, :, c]))
    assert np.array_equal(bits(ctx.eval(Xd).cpu().numpy()), bits(before))                   # the installed plan
    for a, b in zip(mu0, ctx.posterior(Xd, k)):
        assert np.array_equal(bits(a), bits(b.cpu().numpy()))                               # and the GP states


def test_statistics_of_256_paths(ctx):
    """16 batches of 16 paths at 64 candidates: the mean against μ in units of its standard error (closed form)."""
    st, Xc, draws = pr.statistics_case()
    ctx.set_gp(0, st.X, st.lengthscale, st.variance, st.alpha, st.Linv, kernel="matern52")
    Xd = torch.as_tensor(np.array(Xc), device=ctx.device)
    total, pv = np.zeros(64), np.zeros(64)
    for omega, phase, w, z in draws:
        ctx.paths_set(0, omega, phase, w, z, noise=0.0)
        total += ctx.paths_eval(Xd, 1).cpu().numpy()[0].sum(0)
        mu, pathvar, _ = pr.path_moments(st, "matern52", omega, phase, 0.0, Xc)
        pv += pathvar / len(draws)
    t = np.abs(total / 256 - mu) / np.sqrt(pv / 256)
    print(f"device: max |mean - mu| / sqrt(pathvar/256) = {t.max():.2f}")
    assert t.max() <= 5.0


# ------------------------------------------------------------------------------------- return codes and coherence
def _raw(ctx):
    st = pr.make_state(20, 3, "matern52", seed=5)
    ctx.set_gp(0, st.X, st.lengthscale, st.variance, st.alpha, st.Linv)
    ctx.set_gp(1, st.X, st.lengthscale, st.variance, st.alpha, st.Linv)
    omega, phase, w, z = paths.draw_path_inputs("matern52", 20, 3, 4, 8, np.random.default_rng(0))
    return st, [np.ascontiguousarray(a) for a in (omega, phase, w, z)]


def test_return_codes_through_ctypes(ctx):
    st, (omega, phase, w, z) = _raw(ctx)
    lib, h, P = ctx.lib, ctx._h, _lib.host_ptr
    Xd = torch.as_tensor(st.X, device=ctx.device)
    out = torch.zeros((2, 4, 25), dtype=torch.float64, device=ctx.device)
    xp, op = ctypes.c_void_p(Xd.data_ptr()), ctypes.c_void_p(out.data_ptr())

    def pset(obj=0, S=4, m=8, om=P(omega), ph=P(phase), ww=P(w), zz=P(z), noise=0.0):
        return lib.omb_paths_set(h, obj, S, m, om, ph, ww, zz, noise)

    assert pset() == 0 and pset(zz=None) == 0
    for kw in (dict(S=0), dict(S=17), dict(m=0), dict(m=65537), dict(om=None), dict(ph=None), dict(ww=None),
               dict(noise=-1e-9), dict(noise=float("inf")), dict(noise=float("nan")), dict(obj=-1), dict(obj=8)):
        assert pset(**kw) == OMB_EINVAL, kw
        assert lib.omb_last_error(h)
    assert pset(obj=5) == OMB_ESTATE                            # no GP in slot 5
    assert pset(S=17, obj=5) == OMB_EINVAL                      # OMB_EINVAL comes first
    # a failed call leaves the objective without paths
    assert pset() == 0 and lib.omb_paths_eval(h, 1, xp, 20, 25, op) == 0
    assert pset(m=0) == OMB_EINVAL and lib.omb_paths_eval(h, 1, xp, 20, 25, op) == OMB_ESTATE
    assert pset() == 0
    assert lib.omb_paths_eval(h, 1, xp, 0, 0, None) == 0        # N = 0 writes nothing
    assert float(out[0, 0, 24]) == 0.0
    for args in ((0, xp, 20, 25, op), (9, xp, 20, 25, op), (1, xp, -1, 25, op), (1, xp, 20, 19, op),
                 (1, None, 20, 25, op), (1, xp, 20, 25, None)):
        assert lib.omb_paths_eval(h, *args) == OMB_EINVAL, args
    assert lib.omb_paths_eval(h, 2, xp, 20, 25, op) == OMB_ESTATE      # objective 1 has no paths
    assert pset(obj=1, S=3, ww=P(np.ascontiguousarray(w[:, :3])), zz=None) == 0
    assert lib.omb_paths_eval(h, 2, xp, 20, 25, op) == OMB_ESTATE      # 4 and 3 paths
    assert lib.omb_paths_eval(h, 3, xp, 20, 25, op) == OMB_ESTATE      # objective 2 is not set
    assert pset(obj=1, zz=None) == 0 and lib.omb_paths_eval(h, 2, xp, 20, 25, op) == 0
    # n_var > 64: the wide path is out of scope
    wide = pr.make_state(12, 70, "matern52", seed=6)
    ctx.set_gp(2, wide.X, wide.lengthscale, wide.variance, wide.alpha, wide.Linv)
    om70 = np.ascontiguousarray(np.random.default_rng(1).standard_normal((8, 70)))
    assert pset(obj=2, om=P(om70), zz=None) == OMB_EUNSUP
    assert pset(obj=2, S=0, om=P(om70)) == OMB_EINVAL


def test_errors_and_coherence_through_acqcontext(ctx):
    st, (omega, phase, w, z) = _raw(ctx)
    Xd = torch.as_tensor(st.X, device=ctx.device)

    def code(fn, *a, **kw):
        with pytest.raises(OMBError) as e:
            fn(*a, **kw)
        return e.value.code

    with pytest.raises(ValueError):
        ctx.paths_set(0, omega[:, :2], phase, w, z)                   # width against the installed GP
    with pytest.raises(ValueError):
        ctx.paths_set(0, omega, phase, w, z[:5])
    with pytest.raises(ValueError):
        ctx.paths_eval(Xd[:, :2], 1)
    assert code(ctx.paths_set, 0, omega, phase, w, z, noise=-1.0) == OMB_EINVAL
    assert code(ctx.paths_set, 0, omega, phase, np.zeros((8, 17)), None) == OMB_EINVAL
    assert code(ctx.paths_set, 6, omega, phase, w, None) == OMB_ESTATE
    assert code(ctx.paths_eval, Xd, 1) == OMB_ESTATE                  # the failed set above dropped the paths
    # a new state under the paths drops them: set_gp, gp_fit_state, gp_append
    ctx.paths_set(0, omega, phase, w, z)
    assert ctx.paths_eval(Xd, 1).shape == (1, 4, 20)
    for shape in ((1, 3, 20), (1, 4, 19), (2, 4, 20), (4, 20)):       # an out of another layout is refused, not written
        with pytest.raises(ValueError, match="out"):
            ctx.paths_eval(Xd, 1, out=torch.empty(shape, dtype=torch.float64, device=ctx.device))
    with pytest.raises(ValueError, match="out"):
        ctx.paths_eval(Xd, 1, out=torch.empty((1, 4, 40), dtype=torch.float64, device=ctx.device)[:, :, ::2])
    with pytest.raises(ValueError, match="out"):
        ctx.paths_eval(Xd, 1, out=torch.empty((1, 4, 20), dtype=torch.float32, device=ctx.device))
    ctx.set_gp(0, st.X, st.lengthscale, st.variance, st.alpha, st.Linv)
    assert code(ctx.paths_eval, Xd, 1) == OMB_ESTATE
    ctx.paths_set(0, omega, phase, w, z)
    ctx.gp_fit_state(0, st.X, st.y, st.lengthscale, st.variance)
    assert code(ctx.paths_eval, Xd, 1) == OMB_ESTATE
    ctx.paths_set(0, omega, phase, w, z)
    ctx.gp_append(0, np.full((1, 3), 0.37), np.array([0.2]), noise=0.0)
    assert code(ctx.paths_eval, Xd, 1) == OMB_ESTATE
    z21 = np.random.default_rng(3).standard_normal((21, 4))
    ctx.paths_set(0, omega, phase, w, z21)                            # over the grown state
    assert np.all(np.isfinite(ctx.paths_eval(Xd, 1).cpu().numpy()))
    # the other objective's paths never moved
    ctx.paths_set(1, omega, phase, w, z)
    a = ctx.paths_eval(Xd, 2).cpu().numpy()[1]
    ctx.set_gp(0, st.X, st.lengthscale, st.variance, st.alpha, st.Linv)
    ctx.paths_set(0, omega, phase, w, z)
    assert np.array_equal(bits(ctx.paths_eval(Xd, 2).cpu().numpy()[1]), bits(a))
