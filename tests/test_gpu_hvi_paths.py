"""GPU: omb_hvi_paths — the mean over S sampled fronts of the hypervolume improvement of every candidate's path values
 — bitwise against omb_hvi_boxes list by list, and against the np.longdouble restatement of
tests/_nehvi_reference.py.

Lists per case (k, S): unequal lengths, an empty front, grids shorter than C, one list past 1024 boxes and one of
exactly 1024 (the slice edge), at k = 1 two refined threshold lists that do the same.  Every N here is below the size at
which the kernel stops giving each path a workgroup row (130817 candidates); the launch-shape test crosses it.

Accuracy bar: 4× the plain-fp64 restatement's own worst error on the same inputs, in units of the term sum
Σ_s Σ_b |term| / S (every term is ≥ 0, so that is the value itself) — the bar of DESIGN §20-21."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _nehvi_reference as R  # noqa: E402

from optimobo_amd import pareto  # noqa: E402
from optimobo_amd._lib import OMB_EINVAL, OMB_EUNSUP, OMB_OK, OMBError  # noqa: E402

SENTINEL = -12345.678
NS = (1, 13, 255, 256, 257, 1000)
SPLIT_EDGE = 511 * 256          # workgroups of 256 candidates: up to 511 of them, every path gets a workgroup row
_CACHE = {}


@pytest.fixture(scope="module")
def ctx():
    from optimobo_amd.device import AcqContext
    c = AcqContext(0)
    yield c
    c.close()


def refined_threshold(b, B, rng):
    """(−∞, b] cut into B boxes: the same improvement (b − y)⁺, summed over a list that crosses the slice edge."""
    cuts = np.sort(b - rng.uniform(0.01, 2.0, size=B - 1))
    return (np.concatenate(([-np.inf], cuts, [b]))[None, :], np.array([B + 1], np.int32),
            np.stack([np.arange(B), np.arange(1, B + 1)], axis=1).astype(np.uint16))


def case(k, S):
    """(decompositions, packed lists, path values (k, S, 1000)) of one (k, S), built once."""
    if (k, S) in _CACHE:
        return _CACHE[(k, S)]
    rng = np.random.default_rng(1000 * k + S)
    if k == 1:
        b = rng.normal(size=S)
        decomps = pareto.threshold_lists(b)
        decomps[0] = refined_threshold(b[0], 1100, rng)
        if S >= 3:
            decomps[1] = refined_threshold(b[1], 1024, rng)
        y = rng.normal(size=(1, S, 1000)) * 1.5
    else:
        big = {2: 1100, 3: 100, 4: 32}[k]
        sizes = ([big, 0, big, 7, 3] + list(rng.integers(1, 12, size=16)))[:S]
        r = np.full(k, 1.1)
        decomps = [pareto.box_decomposition(R.front(k, P, rng), r) for P in sizes]
        assert len(decomps[0][2]) > 1024
        if S >= 3:                                       # the slice edge itself: the first 1024 boxes of a longer list
            decomps[2] = (decomps[2][0], decomps[2][1], decomps[2][2][:1024])
        y = R.candidates(k, S, 1000, rng)
    packed = pareto.pack_box_lists(decomps)
    lens = np.diff(packed[1])
    assert lens[0] > 1024 and (S < 3 or (1024 in lens and len(set(lens)) > 2))
    assert S < 3 or len({d[0].shape[1] for d in decomps}) > 1            # a grid shorter than C
    assert k == 1 or S < 3 or lens[1] == 1                               # the empty front's single box
    _CACHE[(k, S)] = (decomps, packed, y)
    return _CACHE[(k, S)]


def pitched(y, N, pad=3):
    """y[:, :, :N] on the device at row pitch N + pad (the padding NaN), and an output of N + pad sentinels."""
    k, S = y.shape[:2]
    buf = torch.full((k, S, N + pad), float("nan"), dtype=torch.float64, device="cuda:0")
    buf[:, :, :N] = torch.as_tensor(np.ascontiguousarray(y[:, :, :N]), device="cuda:0")
    out = torch.full((N + pad,), SENTINEL, dtype=torch.float64, device="cuda:0")
    return buf[:, :, :N], out


def run(ctx, yd, packed, out):
    N = yd.shape[2]
    assert ctx.hvi_paths(yd, *packed, out=out) is out
    o = out.cpu().numpy()
    assert np.all(o[N:] == SENTINEL)                     # nothing written past N
    return o[:N]


def run_host(ctx, y, N, packed):
    yd, out = pitched(y, N)
    return run(ctx, yd, packed, out)


@pytest.mark.parametrize("S", [1, 3, 16])
@pytest.mark.parametrize("k", [2, 3, 4])
def test_bitwise_omb_hvi_boxes_per_path_and_their_mean_in_path_order(ctx, k, S):
    decomps, packed, y = case(k, S)
    coords, off, boxes = packed
    for N in NS:
        yd, out = pitched(y, N)
        assert yd.stride(1) == N + 3
        got = run(ctx, yd, packed, out)
        ts = np.stack([ctx.hvi_boxes(yd[:, s, :], coords[s], boxes[off[s]:off[s + 1]]).cpu().numpy() for s in range(S)])
        assert np.array_equal(got, R.mean_in_order(ts)), (k, S, N)
        # the padded grid changes nothing: the list's own grid gives the same bits
        t0 = ctx.hvi_boxes(yd[:, S - 1, :], decomps[S - 1][0], decomps[S - 1][2]).cpu().numpy()
        assert np.array_equal(t0, ts[S - 1])
        assert N < 255 or (got > 0).mean() >= 0.2        # a kernel that returns zeros cannot pass


@pytest.mark.parametrize("S", [1, 3, 16])
def test_one_objective_is_the_restatement_bit_for_bit(ctx, S):
    """k = 1 has no fused operation: the fp64 restatement performs the kernel's additions exactly."""
    _, packed, y = case(1, S)
    for N in NS:
        yd, out = pitched(y, N)
        got = run(ctx, yd, packed, out)
        assert np.array_equal(got, R.alpha(y[:, :, :N], *packed)), (S, N)
    assert (got > 0).mean() >= 0.25


@pytest.mark.parametrize("S", [1, 3, 16])
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_accuracy_against_the_longdouble_restatement(ctx, k, S):
    _, packed, y = case(k, S)
    N = 257
    yd, out = pitched(y, N)
    got = run(ctx, yd, packed, out)
    ref = R.alpha(y[:, :, :N], *packed, dtype=np.longdouble)
    own = R.alpha(y[:, :, :N], *packed)
    live = ref > 0
    assert live.mean() >= 0.2 and np.all(got[~live] == 0.0) and np.all(own[~live] == 0.0)
    e_dev = float(np.max(np.abs(got[live] - ref[live]) / ref[live]))
    e_own = float(np.max(np.abs(own[live] - ref[live]) / ref[live]))
    print(f"k = {k}, S = {S}: device {e_dev:.3g}, fp64 restatement {e_own:.3g} of the term sum (bar 4x)")
    assert e_dev <= 4.0 * e_own


@pytest.mark.parametrize("k,S", [(1, 3), (2, 3), (3, 16)])
def test_edge_values(ctx, k, S):
    _, packed, y = case(k, S)
    N = 300
    yd, out = pitched(y, N)
    base = run(ctx, yd, packed, out).copy()
    y2 = y[:, :, :N].copy()
    y2[k - 1, S - 1, 7] = np.nan                        # one coordinate of one path
    y2[0, 0, 256] = np.nan
    top = packed[0][:, :, -1].max() + 0.5                # at or past every path's reference point / threshold
    y2[:, :, 11] = top
    y2[:, :, 299] = np.inf
    yd, out = pitched(y2, N)
    got = run(ctx, yd, packed, out)
    assert np.isnan(got[7]) and np.isnan(got[256])
    assert got[11] == 0.0 and got[299] == 0.0 and not np.signbit(got[11])
    keep = np.setdiff1d(np.arange(N), [7, 11, 256, 299])
    assert np.array_equal(got[keep], base[keep])         # that candidate only


@pytest.mark.parametrize("k,S", [(1, 16), (2, 3), (4, 3)])
def test_value_does_not_depend_on_the_launch_shape(ctx, k, S):
    """The same candidates at other columns of batches of N ∈ {1, 17, 1000}, and on both sides of the size at which the
    paths stop getting a workgroup row each (the unsplit kernel adds the paths itself): the same bits."""
    _, packed, y = case(k, S)
    probe = y[:, :, :3]
    want = run_host(ctx, probe, 3, packed)
    assert np.all(np.isfinite(want)) and np.any(want > 0)
    for N, cols in ((1, [0]), (17, [16, 3]), (1000, [999, 256, 0]), (SPLIT_EDGE, [SPLIT_EDGE - 1, 70000]),
                    (SPLIT_EDGE + 1, [SPLIT_EDGE, 255, 70001])):
        yy = np.tile(y[:, :, 500:501], (1, 1, N)) if N > 1000 else y[:, :, :N].copy()
        for j, c in enumerate(cols):
            yy[:, :, c] = probe[:, :, j]
        got = run_host(ctx, yy, N, packed)
        for j, c in enumerate(cols):
            assert got[c] == want[j], (N, c)
        if N > 1000:                                     # the filler column too, wherever it stands
            rest = np.delete(got, cols)
            assert np.all(rest == rest[0])
    again = run_host(ctx, probe, 3, packed)
    assert np.array_equal(again, want)


# ----------------------------------------------------------------------------------------------- return codes
def test_return_codes_through_ctypes(ctx):
    lib, h = ctx.lib, ctx._h
    _, (coords, off, boxes), y = case(2, 3)
    S, k, C = coords.shape
    N = 33
    yd, out = pitched(y, N)
    cd = torch.as_tensor(coords, device="cuda:0")
    bd = torch.as_tensor(boxes.view(np.int16), device="cuda:0")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())                                     # noqa: E731
    offp = lambda o: ctypes.c_void_p(np.ascontiguousarray(o, np.int32).ctypes.data)   # noqa: E731
    keep = []

    def call(k=k, S=S, y=ptr(yd), ld=N + 3, N=N, c=ptr(cd), C=C, o=off, b=ptr(bd), out=ptr(out)):
        arr = None if o is None else np.ascontiguousarray(o, np.int32)
        keep.append(arr)
        return lib.omb_hvi_paths(h, k, S, y, ld, N, c, C, None if arr is None else ctypes.c_void_p(arr.ctypes.data),
                                 b, out)
    ctx._stream()
    assert call() == OMB_OK
    ok = out.cpu().numpy().copy()
    assert np.all(ok[:N] != SENTINEL)
    off_by = lambda t, n: ctypes.c_void_p(t.data_ptr() + n)                            # noqa: E731
    dec = off.copy()
    dec[2] = dec[1] - 1
    empty = off.copy()
    empty[2] = empty[1]
    from1 = off + 1
    big = off.copy()
    big[-1] = (1 << 24) + 1
    # each refusal with everything after it in the header's order wrong as well: the earlier one answers
    for want, kw in ((OMB_EINVAL, dict(k=0, S=0)), (OMB_EINVAL, dict(k=9, S=17)), (OMB_EINVAL, dict(S=0, N=-1)),
                     (OMB_EINVAL, dict(S=17, N=-1)), (OMB_EINVAL, dict(N=-1, c=None)), (OMB_EINVAL, dict(c=None, o=dec)),
                     (OMB_EINVAL, dict(b=None, o=dec)), (OMB_EINVAL, dict(o=None, y=None)),
                     (OMB_EINVAL, dict(o=dec, y=None)), (OMB_EINVAL, dict(o=empty, y=None)),
                     (OMB_EINVAL, dict(o=from1, y=None)), (OMB_EINVAL, dict(y=None, c=off_by(cd, 4))),
                     (OMB_EINVAL, dict(out=None, c=off_by(cd, 4))), (OMB_EINVAL, dict(y=off_by(yd, 4), ld=N - 1)),
                     (OMB_EINVAL, dict(c=off_by(cd, 4), ld=N - 1)), (OMB_EINVAL, dict(out=off_by(out, 4), ld=N - 1)),
                     (OMB_EINVAL, dict(b=off_by(bd, 2), ld=N - 1)), (OMB_EINVAL, dict(ld=N - 1, C=1)),
                     (OMB_EUNSUP, dict(C=1)), (OMB_EUNSUP, dict(C=0)), (OMB_EUNSUP, dict(C=4097)),
                     (OMB_EUNSUP, dict(k=8, C=1025)), (OMB_EUNSUP, dict(o=big))):
        assert call(**kw) == want, kw
        assert ctx.lib.omb_last_error(h)
    assert call(b=off_by(bd, 4), o=[0, 1, 2, 3]) == OMB_OK           # 4-byte alignment is the box list's
    ctx.synchronize()
    out.fill_(SENTINEL)
    assert call(N=0, y=None, out=None, ld=0) == OMB_OK and call(N=0) == OMB_OK      # N = 0: nothing written
    ctx.synchronize()
    assert np.all(out.cpu().numpy() == SENTINEL)
    assert call() == OMB_OK
    assert np.array_equal(out.cpu().numpy(), ok)                     # the refusals left the context as it was
    # the plan entry: the same checks on host arrays, then every list's indices
    cz = np.ascontiguousarray(coords)
    bz = np.ascontiguousarray(boxes)

    def plan(k=k, S=S, c=cz, C=C, o=off, b=bz):
        arr = None if o is None else np.ascontiguousarray(o, np.int32)
        keep.append(arr)
        hp = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)          # noqa: E731
        return lib.omb_plan_hvi_paths(h, k, S, hp(c), C, hp(arr), hp(b))
    for want, kw in ((OMB_EINVAL, dict(k=0)), (OMB_EINVAL, dict(S=17)), (OMB_EINVAL, dict(c=None)),
                     (OMB_EINVAL, dict(b=None)), (OMB_EINVAL, dict(o=None)), (OMB_EINVAL, dict(o=dec)),
                     (OMB_EUNSUP, dict(C=1)), (OMB_EUNSUP, dict(o=big, C=1))):
        assert plan(**kw) == want, kw
    bad = bz.copy()
    bad[off[2], 1] = C                                               # list 2's first box: an index past the grid
    assert plan(b=bad) == OMB_EINVAL and b"list 2" in lib.omb_last_error(h)
    bad = bz.copy()
    bad[off[1] - 1, 2:4] = bad[off[1] - 1, 3:1:-1]                   # list 0's last box: lo > hi
    assert plan(b=bad) == OMB_EINVAL and b"list 0" in lib.omb_last_error(h)
    x = torch.zeros((1, 2), dtype=torch.float64, device="cuda:0")
    v = torch.zeros(1, dtype=torch.float64, device="cuda:0")
    assert lib.omb_eval(h, ptr(x), 1, ptr(v)) == -4                  # a refused plan call leaves no plan (OMB_ESTATE)
    assert plan() == OMB_OK


def test_return_codes_through_the_context(ctx):
    _, (coords, off, boxes), y = case(2, 3)
    yd, _ = pitched(y, 20)
    assert ctx.hvi_paths(yd, coords, off, boxes).shape == (20,)
    empty = torch.empty((2, 3, 0), dtype=torch.float64, device="cuda:0")
    assert ctx.hvi_paths(empty, coords, off, boxes).shape == (0,)
    for bad_y in (yd.cpu(), yd.float(), yd[:, :2], yd[:1], yd.permute(1, 0, 2), yd[:, :, ::2]):
        with pytest.raises(ValueError, match="hvi_paths: y"):
            ctx.hvi_paths(bad_y, coords, off, boxes)
    with pytest.raises(ValueError, match="hvi_paths: out"):
        ctx.hvi_paths(yd, coords, off, boxes, out=torch.empty(19, dtype=torch.float64, device="cuda:0"))
    for args in ((coords[0], off, boxes), (coords, off[:-1], boxes), (coords, off, boxes[:-1]), (coords, off, boxes[:, :2])):
        with pytest.raises(ValueError, match="grids"):
            ctx.hvi_paths(yd, *args)
        with pytest.raises(ValueError, match="grids"):
            ctx.plan_hvi_paths(*args)
    dec = off.copy()
    dec[1], dec[2] = off[2], off[1]
    for fn in (lambda *a: ctx.hvi_paths(yd, *a), ctx.plan_hvi_paths):
        with pytest.raises(OMBError) as e:
            fn(coords, dec, boxes)
        assert e.value.code == OMB_EINVAL
        with pytest.raises(OMBError) as e:
            fn(coords[:, :, :1], off, boxes)
        assert e.value.code == OMB_EUNSUP
    assert ctx.plan_kind is None and not ctx.plan_has_gradient()
    ctx.plan_hvi_paths(coords, off, boxes)
    assert ctx.plan_kind == ("omb_plan_hvi_paths", None) and not ctx.plan_has_gradient()
    S17 = pareto.pack_box_lists(pareto.threshold_lists(np.arange(17.0)))
    with pytest.raises(OMBError) as e:
        ctx.plan_hvi_paths(*S17)
    assert e.value.code == OMB_EINVAL and ctx.plan_kind is None
