"""GPU: omb_hvi_boxes — the hypervolume improvement Σ_b Π_j (hi_bj − max(y_j, lo_bj))⁺ of a batch of points over a
box decomposition — against the numpy box sum of _hvi_fixture.py.

Tolerance: rtol (B + 3k)·2^-52, the bound of the sum's own rounding (every term is non-negative, so any summation
order stays inside it); exact zeros must be exactly 0."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from _hvi_fixture import BIG_CASE, CASES, fixture, hvi_numpy, rtol  # noqa: E402

from optimobo_amd._lib import OMB_EINVAL, OMB_EUNSUP, OMB_OK, OMBError  # noqa: E402

SENTINEL = -12345.678


@pytest.fixture(scope="module")
def ctx():
    from optimobo_amd.device import AcqContext
    c = AcqContext(0)
    yield c
    c.close()


def dev(x):
    return torch.as_tensor(np.array(x, dtype=np.float64, order="C"), device="cuda:0")


def dev_boxes(boxes):
    return torch.as_tensor(np.array(boxes, dtype=np.uint16, order="C").view(np.int16), device="cuda:0")


def tiled(Y, N, pad=3):
    """(y (k, N) view with row pitch N + pad, out (N + pad,) filled with the sentinel): column i is Y[i % 64]."""
    k = Y.shape[1]
    buf = torch.full((k, N + pad), float("nan"), dtype=torch.float64, device="cuda:0")
    buf[:, :N] = dev(Y.T[:, np.arange(N) % len(Y)])
    out = torch.full((N + pad,), SENTINEL, dtype=torch.float64, device="cuda:0")
    return buf[:, :N], out


def run(ctx, y, coords, boxes, out):
    N = y.shape[1]
    ctx.hvi_boxes(y, coords, boxes, out=out)
    o = out.cpu().numpy()
    assert np.all(o[N:] == SENTINEL)                         # nothing written past N
    return o[:N]


def check(out, ref, k, B):
    assert (ref > 0).mean() >= 0.5                           # a kernel that returns zeros cannot pass
    assert np.all(out[ref == 0.0] == 0.0)
    err = np.abs(out - ref) / np.where(ref > 0, ref, 1.0)
    print(f"    worst relative error {err.max():.3g} (bound {rtol(k, B):.3g})")
    assert np.all(err <= rtol(k, B))


@pytest.mark.parametrize("case", CASES)
def test_hvi_boxes_vs_numpy(ctx, case):
    f = fixture(*case)
    k, B = case[0], len(f["boxes"])
    coords, boxes = dev(f["coords"]), dev_boxes(f["boxes"])
    for N in (1, 63, 64, 65, 1000, 70001):
        y, out = tiled(f["Y"], N)
        assert y.stride(0) == N + 3
        got = run(ctx, y, coords, boxes, out)
        ref = f["ref"][np.arange(N) % 64]
        print(f"case {case} B={B} N={N}")
        if N >= 63:
            check(got, ref, k, B)
        else:
            assert got[0] == 0.0                             # row 0 is a front point


def test_hvi_boxes_streams_a_list_larger_than_lds(ctx):
    """(k 6, P 30): ≈ 8·10^4 boxes, 24 bytes each — far beyond the 64 KiB the grid alone may take."""
    f = fixture(*BIG_CASE)
    B = len(f["boxes"])
    assert B * 4 * 6 > 16 * 65536
    y, out = tiled(f["Y"], 257)
    got = run(ctx, y, dev(f["coords"]), dev_boxes(f["boxes"]), out)
    print(f"case {BIG_CASE} B={B} N=257")
    check(got, f["ref"][np.arange(257) % 64], 6, B)


@pytest.mark.parametrize("k,C", [(2, 4096), (8, 1024), (3, 2730)])
def test_hvi_boxes_grid_at_the_lds_cap(ctx, k, C):
    """k·C = 8192 doubles (8190 at k = 3): the whole 64 KiB of dynamic LDS, grids the EHVI kernels refuse
    (3·k·C + 2·k + 4 ≤ 8192 there).  A synthetic grid and a short list whose indices reach both ends of it; the sum
    needs no disjoint boxes, so the reference is the numpy box sum as everywhere."""
    rng = np.random.default_rng(k * C)
    coords = np.concatenate([np.full((k, 1), -np.inf), np.sort(rng.uniform(0.0, 1.0, (k, C - 2)), axis=1),
                             np.full((k, 1), 1.2)], axis=1)
    assert coords.shape == (k, C) and k * C > 8192 - k
    B = 7
    boxes = np.empty((B, 2 * k), np.uint16)
    boxes[:, 0::2] = rng.integers(0, C // 3, (B, k))
    boxes[:, 1::2] = np.where(np.arange(B)[:, None] < 4, C - 1, rng.integers(2 * C // 3, C, (B, k)))
    boxes[0, 0::2] = 0                                       # the −∞ column
    Y = rng.uniform(-0.2, 1.25, (300, k))
    ref = hvi_numpy(Y, coords, boxes)
    y, out = tiled(Y, 300)
    got = run(ctx, y, dev(coords), dev_boxes(boxes), out)
    print(f"k={k} C={C} B={B} N=300")
    check(got, ref, k, B)
    with pytest.raises(OMBError) as e:                       # the candidate-blocked EHVI kernel cannot take this grid
        ctx.ehvi_boxes(y.contiguous(), torch.ones_like(y.contiguous()), coords, boxes, kd=True)
    assert e.value.code == OMB_EUNSUP


@pytest.mark.parametrize("case", [(3, 12, 2), (8, 6, 5), BIG_CASE])
def test_hvi_boxes_is_bitwise_reproducible(ctx, case):
    """The same point at columns 0, 64 and N − 1 of batches of different N — on both sides of the size at which the
    box list's slices get workgroup rows of their own (N = 130816 / 130817 at B > 1024), and of the workspace cap
    that ends it for the long list — gives the same bits; so do two calls."""
    f = fixture(*case)
    coords, boxes = dev(f["coords"]), dev_boxes(f["boxes"])
    sizes = (65, 129, 1000) if case == BIG_CASE else (65, 1000, 130816, 130817)
    if case == BIG_CASE:                                     # slices·N ≤ 2^23 doubles of workspace, slices of 1024
        n_ws = (1 << 23) // -(-len(f["boxes"]) // 1024)
        assert 1000 < n_ws < 130816
        sizes = sizes + (n_ws, n_ws + 1)
    seen = None
    for N in sizes:
        Y = f["Y"][np.arange(N) % 64].copy()
        Y[N - 1] = Y[0] = f["Y"][5]                          # column 64 holds Y[64 % 64] = the same point
        Y[64] = f["Y"][5]
        buf = dev(Y.T)
        out = torch.full((N,), SENTINEL, dtype=torch.float64, device="cuda:0")
        a = ctx.hvi_boxes(buf, coords, boxes, out=out).cpu().numpy().copy()
        b = ctx.hvi_boxes(buf, coords, boxes).cpu().numpy()
        assert a.tobytes() == b.tobytes()
        assert a[0] == a[64] == a[N - 1] and a[0] > 0
        same = a[1:N - 1][np.arange(1, N - 1) % 64 == 7]     # every copy of another point, wherever it stands
        assert np.all(same == same[0])
        seen = a[:64].copy() if seen is None else seen
        assert a[:64].tobytes() == seen.tobytes(), f"values depend on N (N={N})"


def test_hvi_boxes_non_finite_inputs(ctx):
    f = fixture(4, 20, 3)
    coords, boxes = dev(f["coords"]), dev_boxes(f["boxes"])
    base = ctx.hvi_boxes(dev(f["Y"].T), coords, boxes).cpu().numpy()
    Y = f["Y"].copy()
    Y[10, 2] = np.nan
    Y[11, 0] = np.inf
    Y[12] = np.nan
    got = ctx.hvi_boxes(dev(Y.T), coords, boxes).cpu().numpy()
    assert np.isnan(got[10]) and np.isnan(got[12]) and got[11] == 0.0
    keep = np.ones(64, bool)
    keep[[10, 11, 12]] = False
    assert got[keep].tobytes() == base[keep].tobytes()       # NaN for that point only
    Y = f["Y"].copy()
    Y[20, 1] = -np.inf
    Y[21] = -np.inf
    got = ctx.hvi_boxes(dev(Y.T), coords, boxes).cpu().numpy()
    keep = np.ones(64, bool)
    keep[[20, 21]] = False
    assert got[keep].tobytes() == base[keep].tobytes()       # −∞ itself is unspecified (inf or NaN)
    assert not np.isfinite(got[21])
    again = ctx.hvi_boxes(dev(f["Y"].T), coords, boxes).cpu().numpy()
    assert again.tobytes() == base.tobytes()                 # the context is as usable as before


# ------------------------------------------------------------------------------------------------ refusals
def _raw(ctx, k, y, ld, N, coords, C, boxes, B, out):
    ctx._stream()
    return ctx.lib.omb_hvi_boxes(ctx._h, k, ctypes.c_void_p(y), ld, N, ctypes.c_void_p(coords), C,
                                 ctypes.c_void_p(boxes), B, ctypes.c_void_p(out))


def test_hvi_boxes_refusals_ctypes(ctx):
    f = fixture(2, 9, 1)
    C, B = f["coords"].shape[1], len(f["boxes"])
    coords, boxes, y = dev(f["coords"]), dev_boxes(f["boxes"]), dev(f["Y"].T)
    out = torch.full((64,), SENTINEL, dtype=torch.float64, device="cuda:0")
    py, pc, pb, po = y.data_ptr(), coords.data_ptr(), boxes.data_ptr(), out.data_ptr()
    good = dict(k=2, y=py, ld=64, N=64, coords=pc, C=C, boxes=pb, B=B, out=po)
    cases = [(dict(k=1), OMB_EINVAL), (dict(k=9), OMB_EINVAL), (dict(N=-1), OMB_EINVAL), (dict(B=0), OMB_EINVAL),
             (dict(y=None), OMB_EINVAL), (dict(coords=None), OMB_EINVAL), (dict(boxes=None), OMB_EINVAL),
             (dict(out=None), OMB_EINVAL), (dict(y=py + 4), OMB_EINVAL), (dict(coords=pc + 4), OMB_EINVAL),
             (dict(out=po + 4), OMB_EINVAL), (dict(boxes=pb + 2), OMB_EINVAL), (dict(ld=63), OMB_EINVAL),
             (dict(C=1), OMB_EUNSUP), (dict(C=4097), OMB_EUNSUP), (dict(B=(1 << 24) + 1), OMB_EUNSUP),
             # the order: an invalid argument is reported before an unsupported size
             (dict(C=1, ld=63), OMB_EINVAL), (dict(B=(1 << 24) + 1, k=9), OMB_EINVAL)]
    for change, want in cases:
        rc = _raw(ctx, **{**good, **change})
        assert rc == want, (change, rc)
        msg = ctx.lib.omb_last_error(ctx._h).decode()
        assert msg, change
        if want == OMB_EUNSUP:
            assert "8192" in msg or "16777216" in msg, msg   # the cap is named
    ctx.synchronize()
    assert np.all(out.cpu().numpy() == SENTINEL)             # a refused call writes nothing
    assert _raw(ctx, **{**good, "N": 0}) == OMB_OK           # N = 0: OMB_OK, nothing written
    assert _raw(ctx, **{**good, "N": 0, "y": None, "out": None, "ld": 0}) == OMB_OK
    ctx.synchronize()
    assert np.all(out.cpu().numpy() == SENTINEL)
    assert _raw(ctx, **good) == OMB_OK
    np.testing.assert_allclose(out.cpu().numpy(), f["ref"], rtol=rtol(2, B), atol=0)


def test_hvi_boxes_refusals_wrapper(ctx):
    f = fixture(2, 9, 1)
    y = dev(f["Y"].T)

    def code(fn):
        with pytest.raises(OMBError) as e:
            fn()
        return e.value.code

    one = torch.zeros((1, 8), dtype=torch.float64, device="cuda:0")
    nine = torch.zeros((9, 8), dtype=torch.float64, device="cuda:0")
    assert code(lambda: ctx.hvi_boxes(one, np.zeros((1, 4)), np.zeros((3, 2), np.uint16))) == OMB_EINVAL
    assert code(lambda: ctx.hvi_boxes(nine, np.zeros((9, 4)), np.zeros((3, 18), np.uint16))) == OMB_EINVAL
    assert code(lambda: ctx.hvi_boxes(y, f["coords"], np.zeros((0, 4), np.uint16))) == OMB_EINVAL
    assert code(lambda: ctx.hvi_boxes(y, np.zeros((2, 1)), f["boxes"])) == OMB_EUNSUP
    assert code(lambda: ctx.hvi_boxes(y, np.zeros((2, 4097)), f["boxes"])) == OMB_EUNSUP
    many = torch.zeros(((1 << 24) + 1, 4), dtype=torch.int16, device="cuda:0")
    assert code(lambda: ctx.hvi_boxes(y, f["coords"], many)) == OMB_EUNSUP
    del many
    with pytest.raises(ValueError):
        ctx.hvi_boxes(y, np.zeros((3, 4)), f["boxes"])       # grid rows != k: refused before the call
    with pytest.raises(ValueError):
        ctx.hvi_boxes(y.T, f["coords"], f["boxes"])          # not objective-major with unit column stride
    bd = dev_boxes(f["boxes"])
    for bad in (bd.to(torch.int32), bd[:, :2], bd.reshape(-1), bd.cpu(), bd.to(torch.float16), bd[::2]):
        with pytest.raises(ValueError, match="box list"):    # a device list is not reinterpreted
            ctx.hvi_boxes(y, f["coords"], bad)
    with pytest.raises(ValueError):
        ctx.hvi_boxes(y.cpu(), f["coords"], bd)
    with pytest.raises(ValueError):
        ctx.hvi_boxes(y.to(torch.float32), f["coords"], bd)
    with pytest.raises(ValueError, match="out"):
        ctx.hvi_boxes(y, f["coords"], bd, out=torch.empty(63, dtype=torch.float64, device="cuda:0"))
    out = torch.full((5,), SENTINEL, dtype=torch.float64, device="cuda:0")
    empty = ctx.hvi_boxes(y[:, :0], f["coords"], f["boxes"])
    assert empty.shape == (0,)
    ctx.hvi_boxes(y[:, :0], f["coords"], f["boxes"], out=out)
    assert np.all(out.cpu().numpy() == SENTINEL)


def test_engine_hvi_and_facade(ctx):
    from optimobo_amd import util_functions
    from optimobo_amd.acquisition import AcquisitionEngine
    f = fixture(3, 12, 2)
    eng = AcquisitionEngine(0)
    got = eng.hvi(f["Y"], f["r"], f["F"])
    assert got.shape == (64,) and got.is_cuda
    B = len(f["boxes"])
    check(got.cpu().numpy(), f["ref"], 3, B)
    np.testing.assert_array_equal(util_functions.hypervolume_improvement(f["Y"], f["F"], f["r"]), got.cpu().numpy())
    one = util_functions.hypervolume_improvement(f["Y"][3], f["F"], f["r"])
    assert isinstance(one, float) and one == got[3].item()
    with pytest.raises(ValueError):
        eng.hvi(fixture(4, 20, 3)["Y"], np.full(4, 1.2), fixture(4, 20, 3)["F"], max_boxes=100)
