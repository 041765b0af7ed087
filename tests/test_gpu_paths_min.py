"""GPU: omb_paths_min — the minimum of every installed sample path over a candidate set, taken in the evaluation
kernel's epilogue.

The reference is omb_paths_eval itself: the value must be bitwise the minimum of its row and the index the lowest
arg-min (plus the offset).  Surrogates: tests/test_grad_reference.acq_gps (n = 17, d = 3; one case at d = 10, the
16-dimension padding; one RBF), m = 33 features (three feature tiles, the last one padded).  N walks the edges of
the 16-candidate wave tile, the 64-candidate workgroup block and more than one block (several partial pairs per path
for the second launch to reduce)."""
import ctypes

import numpy as np
import pytest
from scipy import linalg

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import test_grad_reference as ref  # noqa: E402

from optimobo_amd import _lib, paths  # noqa: E402

M_FEATURES = 33
NS = (1, 15, 16, 17, 63, 64, 65, 257, 4099)
# (kernel, d, S, n_obj)
CASES = [("matern52", 3, S, k) for S in (1, 5, 16) for k in (1, 2)] + [("matern52", 10, 5, 2), ("rbf", 3, 16, 1)]
SENT = -7.5


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device="cuda:0")


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else t
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def ctx():
    from optimobo_amd.device import AcqContext
    c = AcqContext(0)
    yield c
    c.close()


def install(ctx, kernel, d, S, k, seed=0):
    gps = ref.acq_gps(k, d=d, kernel=kernel)
    rng = np.random.default_rng(500 + seed)
    for o, g in enumerate(gps):
        Linv = linalg.solve_triangular(g.L, np.eye(len(g.L)), lower=True)
        ctx.set_gp(o, g.X, g.lengthscale, g.variance, g.alpha, Linv, g.kernel)
        omega, phase, w, z = paths.draw_path_inputs(kernel, len(g.X), d, S, M_FEATURES, rng, np.zeros(d), np.ones(d),
                                                    g.lengthscale)
        ctx.paths_set(o, omega, phase, w, z, noise=g.noise)
    return gps


def lowest_argmin(rows):
    """rows (k, S, N) on the host → (min (k, S), the lowest index attaining it (k, S))."""
    m = rows.min(-1)
    return m, np.argmax(rows == m[..., None], axis=-1)


@pytest.mark.parametrize("kernel,d,S,k", CASES)
def test_values_and_indices_are_the_rows_minimum(ctx, kernel, d, S, k):
    install(ctx, kernel, d, S, k)
    X = np.random.default_rng(7 * S + k + d).uniform(0.0, 1.0, (max(NS), d))
    for N in NS:
        Xd = dev(X[:N])
        rows = ctx.paths_eval(Xd, k)
        want_v, want_i = lowest_argmin(rows.cpu().numpy())
        for offset in (0, 1000003):
            val, idx = ctx.paths_min(Xd, k, offset=offset)
            assert val.shape == (k, S) and idx.shape == (k, S) and idx.dtype == torch.int64
            assert np.array_equal(bits(val), bits(rows.min(dim=-1).values)), (N, offset)
            assert np.array_equal(bits(val), bits(want_v)) and np.array_equal(idx.cpu().numpy(), want_i + offset), N


def test_duplicate_rows_return_the_lower_index(ctx):
    install(ctx, "matern52", 3, 5, 2)
    X = np.random.default_rng(3).uniform(0.0, 1.0, (300, 3))
    rows = ctx.paths_eval(dev(X), 2).cpu().numpy()
    _, at = lowest_argmin(rows)
    # every path's minimiser is copied to a later row in another workgroup's block and to an earlier one
    Xd = np.concatenate([X, X[at.reshape(-1)]])
    val, idx = ctx.paths_min(dev(Xd), 2)
    assert np.array_equal(idx.cpu().numpy(), at) and np.array_equal(bits(val), bits(rows.min(-1)))
    Xe = np.concatenate([X[at.reshape(-1)], X])
    val, idx = ctx.paths_min(dev(Xe), 2)
    flat = at.reshape(-1)                   # two paths may share a minimiser: its first copy wins for both
    first = np.array([np.flatnonzero(flat == v)[0] for v in flat]).reshape(2, 5)
    assert np.array_equal(idx.cpu().numpy(), first) and np.array_equal(bits(val), bits(rows.min(-1)))


def test_nan_rows_never_win_and_empty_results(ctx):
    install(ctx, "matern52", 3, 5, 2)
    X = np.random.default_rng(4).uniform(0.0, 1.0, (130, 3))
    clean = ctx.paths_min(dev(X), 2)
    for row in (0, 64, 129):
        Xn = X.copy()
        Xn[row, 1] = np.nan
        keep = np.delete(np.arange(130), row)
        want_v, want_i = lowest_argmin(ctx.paths_eval(dev(X[keep]), 2).cpu().numpy())
        val, idx = ctx.paths_min(dev(Xn), 2)
        assert np.array_equal(bits(val), bits(want_v)) and np.array_equal(idx.cpu().numpy(), keep[want_i]), row
    val, idx = ctx.paths_min(dev(np.full((70, 3), np.nan)), 2, offset=11)
    assert bool((val == float("inf")).all()) and bool((idx == -1).all())
    # N = 0: {+inf, −1} for every path, nothing past the 2·n_obj·S results
    res = torch.full((2 * 2 * 5 + 1,), SENT, dtype=torch.float64, device="cuda:0")
    assert ctx.lib.omb_paths_min(ctx._h, 2, None, 0, 11, ptr(res)) == _lib.OMB_OK
    ctx.synchronize()
    r = res.cpu().numpy()
    assert np.all(r[0:20:2] == np.inf) and np.all(r[1:20:2] == -1.0) and r[20] == SENT
    # a call with candidates leaves the same sentinel alone
    Xd = dev(X)
    assert ctx.lib.omb_paths_min(ctx._h, 2, ptr(Xd), 130, 0, ptr(res)) == _lib.OMB_OK
    ctx.synchronize()
    r = res.cpu().numpy()
    assert np.array_equal(bits(r[0:20:2]), bits(clean[0]).reshape(-1)) and r[20] == SENT
    assert np.array_equal(r[1:20:2].astype(np.int64), clean[1].cpu().numpy().reshape(-1))


def test_result_does_not_depend_on_what_else_is_in_the_batch(ctx):
    """A fixed point set's minimum is the same bits in front of, behind and in the middle of worse points — other
    columns, waves, workgroups and grid sizes."""
    install(ctx, "matern52", 3, 16, 2)
    rng = np.random.default_rng(5)
    X = rng.uniform(0.0, 1.0, (65, 3))
    alone_v, alone_i = ctx.paths_min(dev(X), 2)
    rows = ctx.paths_eval(dev(X), 2).cpu().numpy()
    pool = rng.uniform(0.0, 1.0, (20000, 3))
    prow = ctx.paths_eval(dev(pool), 2).cpu().numpy()
    worse = pool[np.all(prow > rows.min(-1)[..., None], axis=(0, 1))][:4100]    # every path above its minimum over X
    assert len(worse) >= 200
    for lead in (0, 1, 77, len(worse)):
        Xb = np.concatenate([worse[:lead], X, worse[lead:]])
        val, idx = ctx.paths_min(dev(Xb), 2)
        assert np.array_equal(bits(val), bits(alone_v)), lead
        assert np.array_equal(idx.cpu().numpy(), alone_i.cpu().numpy() + lead), lead


def test_refusals_in_paths_evals_order():
    from optimobo_amd.device import AcqContext
    E, S_, OK = _lib.OMB_EINVAL, _lib.OMB_ESTATE, _lib.OMB_OK
    c = AcqContext(0)
    try:
        lib, h = c.lib, c._h
        X = dev(np.random.default_rng(1).uniform(0, 1, (9, 3)))
        res = torch.full((2 * 2 * 16,), SENT, dtype=torch.float64, device="cuda:0")
        pm = lambda k, x, n, r: lib.omb_paths_min(h, k, x, n, 0, r)  # noqa: E731
        # the arguments (OMB_EINVAL) before the state (OMB_ESTATE): nothing is installed yet
        assert pm(0, ptr(X), 9, ptr(res)) == E and pm(9, ptr(X), 9, ptr(res)) == E
        assert pm(1, ptr(X), -1, ptr(res)) == E
        assert pm(1, ptr(X), 9, None) == E and pm(1, None, 0, None) == E          # res may not be null even at N = 0
        assert pm(1, None, 9, ptr(res)) == E
        assert pm(1, ptr(X), 9, ptr(res)) == S_ and pm(1, None, 0, ptr(res)) == S_
        gps = install(c, "matern52", 3, 5, 1)
        assert pm(1, ptr(X), 9, ptr(res)) == OK
        assert pm(2, ptr(X), 9, ptr(res)) == S_                                    # objective 1 has no GP
        install(c, "matern52", 3, 5, 2)
        assert pm(2, ptr(X), 9, ptr(res)) == OK
        g = gps[0]
        omega, phase, w, z = paths.draw_path_inputs("matern52", 17, 3, 3, M_FEATURES, np.random.default_rng(2),
                                                    np.zeros(3), np.ones(3), g.lengthscale)
        c.paths_set(1, omega, phase, w, z, noise=g.noise)
        assert pm(2, ptr(X), 9, ptr(res)) == S_ and b"paths" in lib.omb_last_error(h)   # 5 and 3 paths
        assert pm(1, ptr(X), 9, ptr(res)) == OK
        # omb_set_gp drops the paths
        Linv = linalg.solve_triangular(g.L, np.eye(len(g.L)), lower=True)
        c.set_gp(0, g.X, g.lengthscale, g.variance, g.alpha, Linv, g.kernel)
        assert pm(1, ptr(X), 9, ptr(res)) == S_ and b"no sample paths" in lib.omb_last_error(h)
        with pytest.raises(_lib.OMBError):
            c.paths_min(X, 1)
    finally:
        c.close()
