"""GPU: omb_hvi_paths_grad — omb_hvi_paths' value (bitwise) with its gradient through the paths and the per-path
outputs, against the np.longdouble restatement of tests/_paths_grad_reference.py.

Lists per k: one decomposition of at least 3,700 boxes cut to 3,700, 1, 1023, 1024 and 1025 boxes (the slice edges),
cycled over the S paths; at k = 1 refined threshold lists of those lengths.  Accuracy bar: 4 × the plain-fp64
restatement's own worst error over the same table, in units of the term sum Σ_s Σ_j Σ_b |box term|·|dy| / S."""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _nehvi_reference as R  # noqa: E402
import _paths_grad_reference as gr  # noqa: E402

from optimobo_amd import pareto  # noqa: E402
from optimobo_amd._lib import OMB_EINVAL, OMB_EUNSUP, OMB_OK  # noqa: E402

LD = np.longdouble
KS = (1, 2, 3, 5, 8)
SS = (1, 5, 16)
DS = (1, 6, 64)
SIZES = (3700, 1, 1023, 1024, 1025)
FRONT = {2: 3700, 3: 220, 5: 26, 8: 9}       # front sizes whose decomposition has at least 3,700 boxes
N = 70
TABLE = [(k, S, DS[(a + b) % 3]) for a, k in enumerate(KS) for b, S in enumerate(SS)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def refined_threshold(b, B, rng):
    """(−∞, b] cut into B boxes: the same improvement (b − y)⁺ over a list of B boxes."""
    cuts = np.sort(b - rng.uniform(0.01, 2.0, size=B - 1))
    return (np.concatenate(([-np.inf], cuts, [b]))[None, :], np.array([B + 1], np.int32),
            np.stack([np.arange(B), np.arange(1, B + 1)], axis=1).astype(np.uint16))


@functools.lru_cache(maxsize=None)
def big(k):
    rng = np.random.default_rng(50 + k)
    dec = pareto.box_decomposition(R.front(k, FRONT[k], rng), np.full(k, 1.1))
    assert len(dec[2]) >= SIZES[0], (k, len(dec[2]))
    return dec


@functools.lru_cache(maxsize=None)
def case(k, S, d):
    """Packed lists, path values y (k, S, N), path gradients dy (k, S, d, N), the longdouble reference and the fp64
    restatement, built once and shared read-only."""
    rng = np.random.default_rng(100 * k + S)
    if k == 1:
        b = rng.normal(size=S)
        decomps = [refined_threshold(b[s], SIZES[s % 5], rng) for s in range(S)]
        y = rng.normal(size=(1, S, N)) * 1.5
    else:
        c, nc, bx = big(k)
        decomps = [(c, nc, bx[:SIZES[s % 5]]) for s in range(S)]
        y = R.candidates(k, S, N, rng)
    packed = pareto.pack_box_lists(decomps)
    assert list(np.diff(packed[1])) == [SIZES[s % 5] for s in range(S)]
    dy = rng.normal(size=(k, S, d, N))
    for a in (y, dy):
        a.setflags(write=False)
    ref = gr.hvi_gradient(y, dy, *packed)
    own = gr.hvi_gradient(y, dy, *packed, dtype=np.float64)
    return packed, y, dy, ref, own


def _err(got, ref, T):
    e = np.abs(np.asarray(got, np.float64).astype(LD) - ref)
    assert np.all(e[T == 0] == 0)                       # no term: exactly 0 in every evaluation
    return float(np.max(np.where(T > 0, e / np.where(T > 0, T, 1), 0)))


@functools.lru_cache(maxsize=None)
def bar():
    worst = 0.0
    for k, S, d in TABLE:
        _, _, _, ref, own = case(k, S, d)
        worst = max(worst, _err(own["g"], ref["g"], ref["Tg"]), _err(own["tg"], ref["tg"], ref["Ttg"]))
    return 4.0 * worst


@pytest.fixture(scope="module")
def ctx():
    from optimobo_amd.device import AcqContext
    c = AcqContext(0)
    yield c
    c.close()


def pitched(y, dy, n, pad=3):
    """y[:, :, :n] and dy[:, :, :, :n] on the device at row pitch n + pad (the padding NaN)."""
    k, S, d = dy.shape[:3]
    yb = torch.full((k, S, n + pad), float("nan"), dtype=torch.float64, device="cuda:0")
    db = torch.full((k, S, d, n + pad), float("nan"), dtype=torch.float64, device="cuda:0")
    yb[:, :, :n] = torch.as_tensor(np.array(y[:, :, :n]), device="cuda:0")
    db[:, :, :, :n] = torch.as_tensor(np.array(dy[:, :, :, :n]), device="cuda:0")
    return yb[:, :, :n], db[:, :, :, :n]


def run(ctx, y, dy, packed, n=None, per_path=True):
    n = y.shape[2] if n is None else n
    yd, dd = pitched(y, dy, n)
    return [t.cpu().numpy() for t in ctx.hvi_paths_grad(yd, dd, *packed, per_path=per_path)], yd


@pytest.mark.parametrize("k,S,d", TABLE)
def test_value_bitwise_and_gradient_against_the_longdouble_restatement(ctx, k, S, d):
    packed, y, dy, ref, own = case(k, S, d)
    (v, g, t, tg), yd = run(ctx, y, dy, packed)
    assert np.array_equal(bits(v), bits(ctx.hvi_paths(yd, *packed).cpu().numpy()))         # omb_hvi_paths' value
    assert g.shape == (N, d) and t.shape == (S, N) and tg.shape == (S, N, d)
    assert np.array_equal(bits(t), bits(own["t"])) or k > 1      # k = 1: no fused operation anywhere
    e_g, e_tg = _err(g, ref["g"], ref["Tg"]), _err(tg, ref["tg"], ref["Ttg"])
    o_g, o_tg = _err(own["g"], ref["g"], ref["Tg"]), _err(own["tg"], ref["tg"], ref["Ttg"])
    print(f"k={k} S={S} d={d}: device g {e_g:.3e} tg {e_tg:.3e}, fp64 numpy g {o_g:.3e} tg {o_tg:.3e}, bar "
          f"{bar():.3e} (term-sum units); device / table-worst numpy = {4 * max(e_g, e_tg) / bar():.3f}")
    assert max(e_g, e_tg) <= bar()
    assert np.any(g != 0) and np.any(tg != 0)                    # a kernel that returns zeros cannot pass
    # without the per-path outputs: the same bits
    (v2, g2), _ = run(ctx, y, dy, packed, per_path=False)
    assert np.array_equal(bits(v2), bits(v)) and np.array_equal(bits(g2), bits(g))


@pytest.mark.parametrize("S", SS)
def test_one_objective_is_the_restatement_bit_for_bit(ctx, S):
    d = DS[(0 + SS.index(S)) % 3]
    packed, y, dy, _, own = case(1, S, d)
    (v, g, t, tg), _ = run(ctx, y, dy, packed)
    for name, got in (("v", v), ("g", g), ("t", t), ("tg", tg)):
        assert np.array_equal(np.asarray(got), np.asarray(own[name])), name


def test_a_value_on_a_grid_coordinate_takes_derivative_zero_for_that_factor(ctx):
    """Two boxes that meet at y_0 = 0.5: (−∞, 0.5] × (−∞, 1] and (0.5, 1] × (−∞, 0.3].  At y = (0.5, 0.1) neither
    strict inequality holds for objective 0, so ∂t/∂y_0 = 0 (a step to the right would give −0.2), and
    ∂t/∂y_1 = −(0·1[…] + 0.5) = −0.5; t = 0·0.9 + 0.5·0.2."""
    dec = (np.array([[-np.inf, 0.2, 0.5, 1.0], [-np.inf, 0.3, 0.6, 1.0]]), np.array([4, 4], np.int32),
           np.array([[0, 2, 0, 3], [2, 3, 0, 1]], np.uint16))
    packed = pareto.pack_box_lists([dec])
    y = np.array([[[0.5, 0.5 + 2.0 ** -20]], [[0.1, 0.1]]])                 # (k = 2, S = 1, N = 2)
    dy = np.zeros((2, 1, 2, 2))
    dy[0, 0, 0, :] = 1.0                                                    # x_0 moves y_0 alone, x_1 moves y_1
    dy[1, 0, 1, :] = 1.0
    (v, g, t, tg), _ = run(ctx, y, dy, packed)
    assert v[0] == 0.5 * (0.3 - 0.1) and np.array_equal(g[0], [0.0, -0.5])
    assert g[1, 0] == -(0.3 - 0.1) and g[1, 1] == -(1.0 - (0.5 + 2.0 ** -20))
    own = gr.hvi_gradient(y, dy, *packed, dtype=np.float64)
    assert np.array_equal(g, own["g"]) and np.array_equal(tg, own["tg"])


@pytest.mark.parametrize("k,S,d", [(1, 5, 6), (3, 5, 1), (8, 5, 6)])
def test_nan_and_past_the_reference_point(ctx, k, S, d):
    packed, y, dy, _, _ = case(k, S, d)
    coords = packed[0]
    (_, g0, _, tg0), _ = run(ctx, y, dy, packed)
    y2 = np.array(y)
    y2[k - 1, S - 1, 7] = np.nan                          # one coordinate of one path
    y2[:, :, 11] = coords[:, :, -1].max() + 0.5           # past every path's reference point / threshold
    (v, g, t, tg), _ = run(ctx, y2, dy, packed)
    assert np.isnan(v[7]) and np.all(np.isnan(g[7])) and np.isnan(t[S - 1, 7]) and np.all(np.isnan(tg[S - 1, 7]))
    assert np.all(np.isfinite(tg[0, 7]))
    assert v[11] == 0.0 and np.all(g[11] == 0.0) and np.all(tg[:, 11] == 0.0)
    keep = np.setdiff1d(np.arange(N), [7, 11])
    assert np.array_equal(bits(g[keep]), bits(g0[keep])) and np.array_equal(bits(tg[:, keep]), bits(tg0[:, keep]))


@pytest.mark.parametrize("k,S,d", [(2, 5, 64), (5, 16, 1)])
def test_results_do_not_depend_on_N_or_the_column(ctx, k, S, d):
    packed, y, dy, _, _ = case(k, S, d)
    (v, g, t, tg), _ = run(ctx, y, dy, packed)
    for n in (1, 255, 256, 257):
        reps = -(-n // N)
        yy, dd = np.tile(y, (1, 1, reps))[:, :, :n], np.tile(dy, (1, 1, 1, reps))[:, :, :, :n]
        (vn, gn, tn, tgn), _ = run(ctx, yy, dd, packed)
        idx = np.arange(n) % N
        assert np.array_equal(bits(vn), bits(v[idx])) and np.array_equal(bits(gn), bits(g[idx])), n
        assert np.array_equal(bits(tn), bits(t[:, idx])) and np.array_equal(bits(tgn), bits(tg[:, idx])), n


def test_a_batch_past_one_pass_of_the_workspace_gives_the_same_bits(ctx):
    """N above the 2^16 candidates of one pass: the second pass's candidates get the bits of the first's."""
    packed, y, dy, _, _ = case(2, 1, 6)
    (v, g, t, tg), _ = run(ctx, y, dy, packed)
    n = (1 << 16) + 5
    reps = -(-n // N)
    yy, dd = np.tile(y, (1, 1, reps))[:, :, :n], np.tile(dy, (1, 1, 1, reps))[:, :, :, :n]
    (vn, gn, tn, tgn), _ = run(ctx, yy, dd, packed)
    idx = np.arange(n) % N
    assert np.array_equal(bits(vn), bits(v[idx])) and np.array_equal(bits(gn), bits(g[idx]))
    assert np.array_equal(bits(tn), bits(t[:, idx])) and np.array_equal(bits(tgn), bits(tg[:, idx]))


@pytest.mark.parametrize("k,S,d", [(3, 5, 1), (1, 16, 64)])
def test_per_path_entries_are_the_single_path_call(ctx, k, S, d):
    packed, y, dy, _, _ = case(k, S, d)
    coords, off, boxes = packed
    (_, _, t, tg), _ = run(ctx, y, dy, packed)
    for s in range(S):
        one = (coords[s:s + 1], np.array([0, off[s + 1] - off[s]], np.int32), boxes[off[s]:off[s + 1]])
        (v1, g1, t1, tg1), _ = run(ctx, y[:, s:s + 1], dy[:, s:s + 1], one)
        assert np.array_equal(bits(t1[0]), bits(t[s])) and np.array_equal(bits(tg1[0]), bits(tg[s])), s
        assert np.array_equal(bits(v1), bits(t[s])) and np.array_equal(bits(g1), bits(tg[s])), s


# ----------------------------------------------------------------------------------------------- return codes
def test_refusals_in_order_through_ctypes(ctx):
    lib, h = ctx.lib, ctx._h
    (coords, off, boxes), y, dy, _, _ = case(2, 5, 64)
    S, k, C = coords.shape
    d, n = 64, 33
    yd, dd = pitched(y, dy, n)
    cd = torch.as_tensor(coords, device="cuda:0")
    bd = torch.as_tensor(boxes.view(np.int16), device="cuda:0")
    out = torch.zeros(n + 3, dtype=torch.float64, device="cuda:0")
    grad = torch.zeros((d, n + 3), dtype=torch.float64, device="cuda:0")
    tt = torch.zeros((S, n + 3), dtype=torch.float64, device="cuda:0")
    tg = torch.zeros((S, d, n + 3), dtype=torch.float64, device="cuda:0")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())                                     # noqa: E731
    keep = []

    def call(k=k, S=S, d=d, y=ptr(yd), dy=ptr(dd), ld=n + 3, N=n, c=ptr(cd), C=C, o=off, b=ptr(bd), out=ptr(out),
             grad=ptr(grad), t=ptr(tt), tg=ptr(tg)):
        arr = None if o is None else np.ascontiguousarray(o, np.int32)
        keep.append(arr)
        return lib.omb_hvi_paths_grad(h, k, S, d, y, dy, ld, N, c, C,
                                      None if arr is None else ctypes.c_void_p(arr.ctypes.data), b, out, grad, t, tg)

    assert call() == OMB_OK and call(t=None, tg=None) == OMB_OK
    assert call(N=0, y=None, dy=None, out=None, grad=None, t=None, tg=None) == OMB_OK
    bad_off = np.array(off).copy()
    bad_off[2] = bad_off[1]
    odd = ctypes.c_void_p(grad.data_ptr() + 4)
    for kw in (dict(k=0), dict(k=9), dict(S=0), dict(S=17), dict(N=-1), dict(c=None), dict(b=None), dict(o=None),
               dict(o=bad_off), dict(y=None), dict(out=None), dict(ld=n - 1),
               dict(d=0), dict(d=65), dict(dy=None), dict(grad=None), dict(t=None), dict(tg=None), dict(grad=odd)):
        assert call(**kw) == OMB_EINVAL, kw
        assert lib.omb_last_error(h)
    assert call(C=1) == OMB_EUNSUP
    # omb_hvi_paths' OMB_EINVAL, then the added OMB_EINVAL, then OMB_EUNSUP
    assert call(C=1, d=0) == OMB_EINVAL and call(C=1, t=None) == OMB_EINVAL and call(C=1, ld=n - 1) == OMB_EINVAL
    torch.cuda.synchronize()
