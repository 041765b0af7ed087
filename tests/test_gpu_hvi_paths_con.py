"""GPU: omb_hvi_paths_con — omb_hvi_paths under constraints through sample paths — against the numpy
restatement of tests/_nehvi_con_reference.py.

Cases (k, c) ∈ {(1,1), (2,1), (2,2), (3,2), (1,7)} × S ∈ {1, 3, 16} × N ∈ {1, 13, 255, 256, 257, 1000}, rows at pitch
N + 3 behind NaN padding, outputs behind sentinels; synthetic path values: at k ≥ 2 fronts of unequal sizes, an empty
one and (k = 2) a list past 1024 boxes.  The constraint values are N(shift, 1) with the shift that leaves half of the
(candidate, path) pairs feasible; on the numpy side every case asserts that 20–80 % of its pairs are feasible and
(S ≥ 2; one path cannot disagree with itself) that some candidate is feasible in some paths and not in others — over
the case's 1000 candidates, of which the smaller N are prefixes.

eta = 0 is exact: out and every u_s are bitwise the restatement over the device's own t_s (omb_hvi_boxes list by list;
k = 1: numpy's, which has no fused operation to differ in).  eta > 0 is measured in units of the term sum
Σ_s |u_s| / S (every term is ≥ 0: the value itself) against the np.longdouble twin; bar: 4× the plain-fp64
restatement's own worst error on the same inputs (DESIGN §24's rule)."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _nehvi_con_reference as RC  # noqa: E402
import _nehvi_reference as R  # noqa: E402

from optimobo_amd import pareto  # noqa: E402
from optimobo_amd._lib import CON_VIOLATION, OMB_EINVAL, OMB_EUNSUP, OMB_OK, OMBError  # noqa: E402

SENTINEL = -12345.678
NS = (1, 13, 255, 256, 257, 1000)
KC = [(1, 1), (2, 1), (2, 2), (3, 2), (1, 7)]
SPLIT_EDGE = 511 * 256          # up to 511 workgroups of 256 candidates every path gets a workgroup row


@pytest.fixture(scope="module")
def ctx():
    from optimobo_amd.device import AcqContext
    c = AcqContext(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def pitched(y, N, pad=3):
    rows, S = y.shape[:2]
    buf = torch.full((rows, S, N + pad), float("nan"), dtype=torch.float64, device="cuda:0")
    buf[:, :, :N] = torch.as_tensor(np.ascontiguousarray(y[:, :, :N]), device="cuda:0")
    out = torch.full((N + pad,), SENTINEL, dtype=torch.float64, device="cuda:0")
    return buf[:, :, :N], out


def run(ctx, y, N, c, packed, **kw):
    """(out (N,), u (S, N), the device tensor of y) of y[:, :, :N] at pitch N + 3."""
    yd, out = pitched(y, N)
    got, u = ctx.hvi_paths_con(yd, c, *packed, out=out, per_path=True, **kw)
    assert got is out and u.shape == (y.shape[1], N)
    o = out.cpu().numpy()
    assert np.all(o[N:] == SENTINEL)                     # nothing written past N
    return o[:N], u.cpu().numpy(), yd


def device_ts(ctx, yd, k, packed):
    """t_s of the device: omb_hvi_boxes list by list (k = 1 has no such entry: the restatement's, exact there)."""
    coords, off, boxes = packed
    if k == 1:
        return R.path_values(yd[:1].cpu().numpy(), *packed)
    return np.stack([ctx.hvi_boxes(yd[:k, s, :], coords[s], boxes[off[s]:off[s + 1]]).cpu().numpy()
                     for s in range(coords.shape[0])])


@pytest.mark.parametrize("S", [1, 3, 16])
@pytest.mark.parametrize("k,c", KC)
def test_no_constraints_is_omb_hvi_paths_bit_for_bit(ctx, k, c, S):
    packed, y = RC.case(k, c, S)
    for N in NS:
        yd, out = pitched(y[:k], N)
        got = ctx.hvi_paths_con(yd, 0, *packed, out=out).cpu().numpy()[:N]
        want = ctx.hvi_paths(yd, *packed).cpu().numpy()
        assert np.array_equal(bits(got), bits(want)), (k, S, N)
    assert (got > 0).mean() >= 0.2


@pytest.mark.parametrize("S", [1, 3, 16])
@pytest.mark.parametrize("k,c", KC)
def test_indicator_weight_is_the_restatement_bit_for_bit(ctx, k, c, S):
    packed, y = RC.case(k, c, S)
    feas = RC.check_mix(y[k:])
    for N in NS:
        for violation in (False, True):
            got, u, yd = run(ctx, y, N, c, packed, violation=violation)
            ts = device_ts(ctx, yd, k, packed)
            want, wu = RC.alpha(y[:, :, :N], c, *packed, violation=violation, ts=ts)
            assert np.array_equal(bits(u), bits(wu)), (k, c, S, N, violation)
            assert np.array_equal(bits(got), bits(want)), (k, c, S, N, violation)
            f = feas[:, :N]
            assert np.all(u[f] >= 0) and (np.all(u[~f] < 0) if violation else np.all(u[~f] == 0.0))
            if N == 1000:                                # a kernel that returns zeros cannot pass
                assert (u > 0).mean() >= 0.1 and ((u < 0).mean() >= 0.2 if violation else (got > 0).mean() >= 0.1)


@pytest.mark.parametrize("eta", [1e-3, 0.5])
@pytest.mark.parametrize("S", [1, 3, 16])
@pytest.mark.parametrize("k,c", KC)
def test_sigmoid_weight_against_the_longdouble_twin(ctx, k, c, S, eta):
    packed, y = RC.case(k, c, S)
    RC.check_mix(y[k:])
    N = 257
    got, u, _ = run(ctx, y, N, c, packed, eta=eta)
    ref, ru = RC.alpha(y[:, :, :N], c, *packed, eta=eta, dtype=np.longdouble)
    own, ou = RC.alpha(y[:, :, :N], c, *packed, eta=eta)
    # the twin's exponent range is wider than fp64's: a weight it holds below fp64's smallest normal number has no
    # relative accuracy in fp64 at all (e^{−1000} is 0 there), so such values are held to that bound, not to a ratio
    tiny = np.finfo(np.float64).tiny
    live = ref >= tiny
    assert live.mean() >= 0.2 and np.all(got[~live] <= tiny) and np.all(own[~live] <= tiny)
    e_dev = float(np.max(np.abs(got[live] - ref[live]) / ref[live]))
    e_own = float(np.max(np.abs(own[live] - ref[live]) / ref[live]))
    lu = ru >= tiny
    eu_dev = float(np.max(np.abs(u[lu] - ru[lu]) / ru[lu]))
    eu_own = float(np.max(np.abs(ou[lu] - ru[lu]) / ru[lu]))
    print(f"k = {k}, c = {c}, S = {S}, eta = {eta}: device {e_dev:.3g}, fp64 restatement {e_own:.3g} of the term sum; "
          f"per path {eu_dev:.3g} against {eu_own:.3g} (bar 4x)")
    assert np.all(u[~lu] <= tiny) and np.all(u >= 0)
    assert e_dev <= 4.0 * e_own
    assert eu_dev <= 4.0 * eu_own


@pytest.mark.parametrize("k,c,S", [(1, 7, 3), (2, 1, 16), (3, 2, 3)])
def test_value_does_not_depend_on_the_launch_shape(ctx, k, c, S):
    """The same candidates at other columns of batches of N ∈ {1, 17, 1000}, and on both sides of the size at which the
    paths stop getting a workgroup row each: the same bits, with the indicator, the flag and the sigmoid."""
    packed, y = RC.case(k, c, S)
    feas = RC.check_mix(y[k:])
    mixed = np.flatnonzero((feas.sum(0) > 0) & (feas.sum(0) < S))[:3]
    probe = y[:, :, mixed]
    for kw in (dict(), dict(violation=True), dict(eta=0.5)):
        want, wu, _ = run(ctx, probe, 3, c, packed, **kw)
        assert np.all(np.isfinite(want)) and np.any(wu != 0)
        for N, cols in ((1, [0]), (17, [16, 3]), (1000, [999, 256, 0]), (SPLIT_EDGE, [SPLIT_EDGE - 1, 70000]),
                        (SPLIT_EDGE + 1, [SPLIT_EDGE, 255, 70001])):
            yy = np.tile(y[:, :, 500:501], (1, 1, N)) if N > 1000 else y[:, :, :N].copy()
            for j, col in enumerate(cols):
                yy[:, :, col] = probe[:, :, j]
            got, u, _ = run(ctx, yy, N, c, packed, **kw)
            for j, col in enumerate(cols):
                assert bits(got)[col] == bits(want)[j], (N, col, kw)
                assert np.array_equal(bits(u[:, col]), bits(wu[:, j])), (N, col, kw)
            if N > 1000:                                 # the filler column too, wherever it stands
                rest = np.delete(got, cols)
                assert np.all(rest == rest[0])


@pytest.mark.parametrize("k,c,S", [(2, 1, 3), (1, 7, 16), (3, 2, 3)])
def test_wavefronts_of_infeasible_candidates_skip_without_changing_a_bit(ctx, k, c, S):
    """Blocks of 64 consecutive candidates infeasible in every path (aligned to the wavefront, and not) next to
    feasible ones: the restatement's bits; the same candidates permuted — so that no wavefront is infeasible
    throughout — give the same bits."""
    packed, y = RC.case(k, c, S)
    N = 640
    y = y[:, :, :N].copy()
    for b0 in (64, 256, 300, 576):                       # 300..363 straddles two wavefronts
        y[k:, :, b0:b0 + 64] = np.abs(y[k:, :, b0:b0 + 64]) + 2.0
    y[k, 1 % S, 0:64] = 3.0                              # one path alone: a wavefront that skips list 1 only
    feas = np.all(y[k:] <= 0, axis=0)
    assert not feas[:, 64:128].any() and feas[:, :64].any() and feas[:, 128:256].any() and 0.1 <= feas.mean() <= 0.8
    perm = np.random.default_rng(5).permutation(N)
    assert all(feas[:, perm][:, w:w + 64].any() for w in range(0, N, 64))
    for kw in (dict(), dict(violation=True), dict(eta=1e-3)):
        got, u, yd = run(ctx, y, N, c, packed, **kw)
        if not kw.get("eta"):
            want, wu = RC.alpha(y, c, *packed, ts=device_ts(ctx, yd, k, packed), **kw)
            assert np.array_equal(bits(u), bits(wu)) and np.array_equal(bits(got), bits(want))
        else:                                            # e^{−2000} = 0: the sigmoid's weight is exactly 0 there
            assert np.all(u[:, 64:128] == 0.0) and np.all(got[64:128] == 0.0) and np.any(got[128:256] > 0)
        pg, pu, _ = run(ctx, y[:, :, perm], N, c, packed, **kw)
        assert np.array_equal(bits(pg), bits(got[perm])) and np.array_equal(bits(pu), bits(u[:, perm]))


@pytest.mark.parametrize("k,c,S", [(1, 1, 3), (2, 2, 3), (3, 2, 16)])
def test_nan_rules(ctx, k, c, S):
    packed, y = RC.case(k, c, S)
    N = 300
    for kw in (dict(), dict(violation=True), dict(eta=0.5)):
        base, bu, _ = run(ctx, y, N, c, packed, **kw)
        y2 = y[:, :, :N].copy()
        y2[k + c - 1, S - 1, 7] = np.nan                 # a constraint value of the last path
        y2[0, 0, 256] = np.nan                           # an objective value of path 0
        y2[k, 0, 70] = np.nan                            # a constraint value (c > 1: where another one is violated)
        if c > 1:
            y2[k + c - 1, 0, 70] = 5.0
        y2[k:, :, 71] = 5.0                              # infeasible everywhere, and a NaN objective in one path
        y2[k - 1, S - 1, 71] = np.nan
        got, u, _ = run(ctx, y2, N, c, packed, **kw)
        assert np.isnan(got[[7, 256, 70, 71]]).all()
        assert np.isnan(u[S - 1, 7]) and np.isnan(u[0, 256]) and np.isnan(u[0, 70]) and np.isnan(u[S - 1, 71])
        assert np.isnan(u).sum() == 4                    # that path only
        keep = np.setdiff1d(np.arange(N), [7, 256, 70, 71])
        assert np.array_equal(bits(got[keep]), bits(base[keep]))       # that candidate only
        assert np.array_equal(bits(u[:, keep]), bits(bu[:, keep]))


# ----------------------------------------------------------------------------------------------- return codes
def test_return_codes_through_ctypes(ctx):
    lib, h = ctx.lib, ctx._h
    (coords, off, boxes), y = RC.case(2, 2, 3)
    S, k, C = coords.shape
    N = 33
    yd, out = pitched(y, N)
    ud = torch.full((S, N + 3), SENTINEL, dtype=torch.float64, device="cuda:0")
    cd = torch.as_tensor(coords, device="cuda:0")
    bd = torch.as_tensor(boxes.view(np.int16), device="cuda:0")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())                                     # noqa: E731
    off_by = lambda t, n: ctypes.c_void_p(t.data_ptr() + n)                            # noqa: E731
    keep = []

    def call(k=k, S=S, n_con=2, y=ptr(yd), ld=N + 3, N=N, c=ptr(cd), C=C, o=off, b=ptr(bd), eta=0.0, flags=0,
             out=ptr(out), u=ptr(ud)):
        arr = None if o is None else np.ascontiguousarray(o, np.int32)
        keep.append(arr)
        return lib.omb_hvi_paths_con(h, k, S, n_con, y, ld, N, c, C,
                                     None if arr is None else ctypes.c_void_p(arr.ctypes.data), b, eta, flags, out, u)
    ctx._stream()
    assert call() == OMB_OK
    ctx.synchronize()
    ok, oku = out.cpu().numpy().copy(), ud.cpu().numpy().copy()
    assert np.all(ok[:N] != SENTINEL) and np.all(oku[:, :N] != SENTINEL) and np.all(oku[:, N:] == SENTINEL)
    dec = off.copy()
    dec[2] = dec[1] - 1
    big = off.copy()
    big[-1] = (1 << 24) + 1
    nan, inf = float("nan"), float("inf")
    # each refusal with everything after it in the header's order wrong as well: the earlier one answers
    for want, kw in ((OMB_EINVAL, dict(k=0, n_con=-1)), (OMB_EINVAL, dict(S=17, n_con=-1)), (OMB_EINVAL, dict(N=-1, eta=nan)),
                     (OMB_EINVAL, dict(c=None, eta=nan)), (OMB_EINVAL, dict(o=dec, eta=nan)),
                     (OMB_EINVAL, dict(y=None, flags=2)), (OMB_EINVAL, dict(out=off_by(out, 4), flags=2)),
                     (OMB_EINVAL, dict(ld=N - 1, flags=2)),
                     (OMB_EUNSUP, dict(C=1, n_con=-1)), (OMB_EUNSUP, dict(o=big, eta=-1.0)),     # omb_hvi_paths' own first
                     (OMB_EINVAL, dict(n_con=-1, eta=nan)), (OMB_EINVAL, dict(n_con=7, eta=-1e-300)),
                     (OMB_EINVAL, dict(n_con=7, eta=nan)), (OMB_EINVAL, dict(n_con=7, eta=inf)),
                     (OMB_EINVAL, dict(n_con=7, flags=2)), (OMB_EINVAL, dict(n_con=7, flags=0x80000000)),
                     (OMB_EINVAL, dict(n_con=7, flags=CON_VIOLATION, eta=0.5)),
                     (OMB_EINVAL, dict(n_con=7, out=None, u=None)), (OMB_EINVAL, dict(n_con=7, u=off_by(ud, 4))),
                     (OMB_EUNSUP, dict(n_con=7)), (OMB_EUNSUP, dict(n_con=2 ** 31 - 1))):
        assert call(**kw) == want, kw
        assert ctx.lib.omb_last_error(h)
    ctx.synchronize()
    assert np.array_equal(out.cpu().numpy(), ok) and np.array_equal(ud.cpu().numpy(), oku)      # a refusal writes nothing
    # either output alone
    out.fill_(SENTINEL)
    ud.fill_(SENTINEL)
    assert call(out=None) == OMB_OK and call(u=None, flags=CON_VIOLATION) == OMB_OK and call(eta=0.5, u=None) == OMB_OK
    ctx.synchronize()
    assert np.array_equal(ud.cpu().numpy(), oku) and np.all(out.cpu().numpy()[:N] != SENTINEL)
    assert call(u=None) == OMB_OK
    ctx.synchronize()
    assert np.array_equal(out.cpu().numpy(), ok)
    # N = 0: nothing written, with or without pointers
    out.fill_(SENTINEL)
    assert call(N=0, y=None, out=None, u=None, ld=0) == OMB_OK and call(N=0) == OMB_OK
    ctx.synchronize()
    assert np.all(out.cpu().numpy() == SENTINEL)
    # the plan entry: the same checks on host arrays, then every list's indices
    cz, bz = np.ascontiguousarray(coords), np.ascontiguousarray(boxes)

    def plan(k=k, S=S, n_con=2, eta=0.0, c=cz, C=C, o=off, b=bz):
        arr = None if o is None else np.ascontiguousarray(o, np.int32)
        keep.append(arr)
        hp = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)          # noqa: E731
        return lib.omb_plan_hvi_paths_con(h, k, S, n_con, eta, hp(c), C, hp(arr), hp(b))
    for want, kw in ((OMB_EINVAL, dict(k=0)), (OMB_EINVAL, dict(S=17)), (OMB_EINVAL, dict(c=None)),
                     (OMB_EINVAL, dict(o=dec)), (OMB_EUNSUP, dict(C=1, n_con=-1)), (OMB_EINVAL, dict(n_con=-1)),
                     (OMB_EINVAL, dict(eta=-1.0)), (OMB_EINVAL, dict(eta=nan)), (OMB_EUNSUP, dict(n_con=7))):
        assert plan(**kw) == want, kw
    bad = bz.copy()
    bad[off[2], 1] = C                                               # list 2's first box: an index past the grid
    assert plan(b=bad) == OMB_EINVAL and b"list 2" in lib.omb_last_error(h)
    x = torch.zeros((1, 2), dtype=torch.float64, device="cuda:0")
    v = torch.zeros(1, dtype=torch.float64, device="cuda:0")
    assert lib.omb_eval(h, ptr(x), 1, ptr(v)) == -4                  # a refused plan call leaves no plan (OMB_ESTATE)
    assert plan() == OMB_OK and plan(n_con=0, eta=0.5) == OMB_OK and plan(k=1, n_con=7, c=cz[:, :1], b=bz[:, :2]) == OMB_OK


def test_return_codes_through_the_context(ctx):
    (coords, off, boxes), y = RC.case(2, 2, 3)
    yd, _ = pitched(y, 20)
    assert ctx.hvi_paths_con(yd, 2, coords, off, boxes).shape == (20,)
    v, u = ctx.hvi_paths_con(yd, 2, coords, off, boxes, per_path=True, violation=True)
    assert v.shape == (20,) and u.shape == (3, 20)
    empty = torch.empty((4, 3, 0), dtype=torch.float64, device="cuda:0")
    assert ctx.hvi_paths_con(empty, 2, coords, off, boxes).shape == (0,)
    for bad_y, c in ((yd.cpu(), 2), (yd.float(), 2), (yd[:, :2], 2), (yd, 1), (yd, 3), (yd, -1), (yd[:, :, ::2], 2)):
        with pytest.raises(ValueError, match="hvi_paths_con: y"):
            ctx.hvi_paths_con(bad_y, c, coords, off, boxes)
    with pytest.raises(ValueError, match="hvi_paths_con: out"):
        ctx.hvi_paths_con(yd, 2, coords, off, boxes, out=torch.empty(19, dtype=torch.float64, device="cuda:0"))
    with pytest.raises(ValueError, match="grids"):
        ctx.hvi_paths_con(yd, 2, coords[0], off, boxes)
    for kw, code in ((dict(eta=-1.0), OMB_EINVAL), (dict(eta=0.5, violation=True), OMB_EINVAL)):
        with pytest.raises(OMBError) as e:
            ctx.hvi_paths_con(yd, 2, coords, off, boxes, **kw)
        assert e.value.code == code
    b7, packed7 = R.thresholds_for(3, np.random.default_rng(0))
    y9 = torch.zeros((9, 3, 4), dtype=torch.float64, device="cuda:0")
    with pytest.raises(OMBError) as e:
        ctx.hvi_paths_con(y9, 8, *packed7)
    assert e.value.code == OMB_EUNSUP
    ctx.plan_hvi_paths_con(2, coords, off, boxes)
    assert ctx.plan_kind == ("omb_plan_hvi_paths_con", None) and not ctx.plan_has_gradient()
    with pytest.raises(OMBError) as e:
        ctx.plan_hvi_paths_con(7, coords, off, boxes)
    assert e.value.code == OMB_EUNSUP and ctx.plan_kind is None
    assert pareto.pack_box_lists(pareto.threshold_lists(b7))[0].shape == (3, 1, 2)
