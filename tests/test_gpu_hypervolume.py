"""GPU: omb_hypervolume / omb_hypervolume_contrib against the grid-sweep formula in ``np.longdouble``
(tests/_hypervolume_reference.py; checked against ``pareto.hypervolume`` on the CPU by tests/test_hypervolume_host.py).

Bars.  n kept rows, k objectives, reference value HV:
  hypervolume     |device − reference| ≤ (n + k + 48)·2^-53·HV — n for a cell's staircase sum of positive terms, k for
                  the products, 48 for the depth of the tree of additions over at most 2^40 cells, with slack;
  contributions   |c_i − (HV − HV₋ᵢ)| ≤ 2·(n + k + 48)·2^-53·HV (two such sums); a duplicate's, a dominated row's and a
                  dropped row's is exactly 0.0, which is within it.
Every size where the code takes another path: n around the wavefront (63, 64, 65) and at the workgroup (1023, 1024),
cells around one cell workgroup (k = 4 at n = 70: 4900 cells in 3 workgroups; k = 8 at n = 5: 15,625 in 8), both rank
words (k ≥ 7 uses the second), N past one compaction pass (4096 rows).  One reference per input, shared."""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _hypervolume_reference as R  # noqa: E402

from optimobo_amd import _lib, pareto  # noqa: E402
from optimobo_amd._lib import OMB_EINVAL, OMB_EUNSUP, OMBError  # noqa: E402

U = 2.0 ** -53
SHAPES = [(k, n) for k in (1, 2, 3) for n in (0, 1, 2, 63, 64, 65, 1023, 1024)] + \
         [(4, 1), (4, 20), (4, 70), (5, 12), (6, 8), (8, 5)]
KINDS = ("sphere", "lattice")


@pytest.fixture(scope="module")
def ctx():
    from optimobo_amd.device import AcqContext
    c = AcqContext(0)
    yield c
    c.close()


def bar(n, k, hv):
    return (n + k + 48) * U * float(hv)


@functools.lru_cache(maxsize=None)
def case(kind, k, n):
    """(P (N, k), r, n, reference hypervolume in longdouble): n kept rows among duplicates, dominated and dropped rows."""
    P, r = R.dressed(np.random.default_rng(1000 * k + n + (7 if kind == "lattice" else 0)), kind, n, k)
    P.setflags(write=False)
    return P, r, R.hv_grid(P, r)


def put(sets, pad=3, slots=None, S=None):
    """The sets (each (N, k)) as one pitched (k, S, N) view of a buffer whose other entries hold 0.0 — a row that
    would be kept and dominate everything, were it read; ``slots``: the set slot of each, the others' rows NaN."""
    (N, k), slots = sets[0].shape, list(range(len(sets))) if slots is None else slots
    S = len(sets) if S is None else S
    buf = torch.zeros((k, S, N + pad), dtype=torch.float64, device="cuda:0")
    buf[:, :, :N] = np.nan
    for s, Y in zip(slots, sets):
        buf[:, s, :N] = torch.as_tensor(np.array(Y.T, order="C"), device="cuda:0")
    return buf[:, :, :N]


def hv_of(ctx, P, r, **kw):
    return ctx.hypervolume(put([P], **kw), r, 1).cpu().numpy()


def assert_bits(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.tobytes() == b.tobytes(), (what, a, b)


# ----------------------------------------------------------------------------------------------- accuracy
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k,n", SHAPES)
def test_hypervolume_matches_the_extended_precision_reference(ctx, kind, k, n):
    P, r, want = case(kind, k, n)
    got = hv_of(ctx, P, r)
    assert got.shape == (1,) and got.dtype == np.float64
    err = abs(R.LD(got[0]) - want)
    print(f"{kind} k={k} n={n}: hv={got[0]!r} err={float(err / want) / U if want else 0.0:.2f} ulp "
          f"(bar {n + k + 48})")
    if n == 0:
        assert got[0] == 0.0 and np.signbit(got[0]) == 0
    else:
        assert want > 0 and err <= bar(n, k, want)


def test_seven_objectives_use_both_rank_words(ctx):
    rng = np.random.default_rng(77)
    for k, n in ((7, 6), (8, 5)):
        P, r = R.dressed(rng, "sphere", n, k)
        P = np.vstack((P, R.lattice(rng, 3, k) / 4.0))       # ties with nothing, ranks in every objective
        n = int(R.kept_rows(P, r).sum())
        want = R.hv_grid(P, r)
        assert abs(R.LD(hv_of(ctx, P, r)[0]) - want) <= bar(n, k, want)
        assert abs(want - pareto.hypervolume(P[R.kept_rows(P, r)], r)) <= 1e-12 * want


def test_rows_past_one_compaction_pass(ctx):
    """N = 9001 rows (three passes of 4096), the kept ones spread over all of them."""
    P, r, want = case("sphere", 4, 70)
    rng = np.random.default_rng(5)
    big = np.full((9001, 4), 2.0)                              # dropped: beyond the reference point
    big[:, 1] = np.where(rng.uniform(size=9001) < 0.3, np.nan, 2.0)
    at = np.sort(rng.choice(9001, size=len(P), replace=False))
    at[-1] = 9000
    big[at] = P
    got = hv_of(ctx, big, r)
    assert_bits(got, hv_of(ctx, P, r), "dropped rows around the kept ones")
    assert abs(R.LD(got[0]) - want) <= bar(70, 4, want)


# ----------------------------------------------------------------------------------------------- sets and masks
@pytest.mark.parametrize("S", [1, 3, 16])
@pytest.mark.parametrize("k", [2, 3, 5])
def test_sets_with_their_own_masks(ctx, k, S):
    rng = np.random.default_rng(10 * k + S)
    N = 37 if k < 5 else 14
    sets = [np.vstack((R.sphere(rng, N - 5, k), R.dressed(rng, "sphere", 0, k)[0])) for _ in range(S)]
    r = np.full(k, 1.1)
    masks = rng.uniform(size=(S, N)) < 0.6
    masks[S // 2] = False                                      # one set with every row masked out
    if S > 2:
        sets[2][:, 0] = 1.2                                    # one set with every row dropped
    Y = put(sets, pad=3)
    m = torch.full((S, N + 5), 1, dtype=torch.uint8, device="cuda:0")     # ones past N: rows that must not be read
    m[:, :N] = torch.as_tensor(masks, device="cuda:0")
    got = ctx.hypervolume(Y, r, S, mask=m[:, :N]).cpu().numpy()
    gotb = ctx.hypervolume(Y, r, S, mask=torch.as_tensor(masks, device="cuda:0")).cpu().numpy()
    assert_bits(got, gotb, "a uint8 pitched mask and a bool one")
    for s in range(S):
        sub = sets[s][masks[s]]
        want, n = R.hv_grid(sub, r), int(R.kept_rows(sub, r).sum())
        assert abs(R.LD(got[s]) - want) <= bar(n, k, want), (s, got[s], want)
        if n == 0:
            assert got[s] == 0.0
        assert_bits(got[s:s + 1], hv_of(ctx, sub, r), f"set {s} alone, filtered on the host")
    assert got[S // 2] == 0.0 and (S <= 2 or got[2] == 0.0)


# ----------------------------------------------------------------------------------------------- bitwise equality
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k,n", [(1, 65), (2, 65), (3, 1024), (4, 70), (5, 12), (8, 5)])
def test_bits_do_not_depend_on_order_pitch_slot_or_padding(ctx, kind, k, n):
    P, r, _ = case(kind, k, n)
    base = hv_of(ctx, P, r)
    rng = np.random.default_rng(k + n)
    assert_bits(hv_of(ctx, P[rng.permutation(len(P))], r), base, "a row permutation")
    assert_bits(hv_of(ctx, P[::-1], r), base, "the rows reversed")
    assert_bits(hv_of(ctx, P, r, pad=0), base, "pitch N")
    assert_bits(hv_of(ctx, P, r, pad=1029), base, "pitch N + 1029")
    other, ro, _ = case(kind, k, 2 if n != 2 else 1)
    filler = np.vstack((other, np.full((len(P) - len(other), k), np.nan)))   # another set beside it: fewer cells
    for S, slot in ((3, 2), (16, 15), (16, 7)):
        got = ctx.hypervolume(put([P, filler], slots=[slot, 0], S=S), r, S).cpu().numpy()
        assert_bits(got[slot:slot + 1], base, f"slot {slot} of {S}")
        assert_bits(got[0:1], hv_of(ctx, other, ro), "the small set beside a large one")
    dropped = np.vstack((np.full((700, k), np.inf), P, np.full((3, k), r), np.full((611, k), np.nan)))
    assert_bits(hv_of(ctx, dropped, r), base, "N padded with dropped rows")
    kept = P[R.kept_rows(P, r)]
    assert_bits(hv_of(ctx, kept, r), base, "the kept rows alone")
    hv2, _ = ctx.hypervolume_contributions(put([P])[:, 0, :], r)
    assert_bits(hv2.cpu().numpy(), base, "the contributions entry's hypervolume")


def test_mask_from_nondominated_changes_no_bit(ctx):
    for kind, k, n in (("sphere", 3, 65), ("lattice", 3, 65), ("lattice", 4, 70), ("lattice", 5, 12)):
        P, r, want = case(kind, k, n)
        P = P[R.kept_rows(P, r)]              # the filter takes ±inf for ordinary values: finite rows only
        Y = put([P])
        mask, counts = ctx.nondominated(Y, 1)
        front = P[mask[0].cpu().numpy()]
        if kind == "lattice":
            assert len(front) < n                               # the mask does drop rows here
        a = ctx.hypervolume(Y, r, 1, mask=mask).cpu().numpy()
        assert_bits(a, hv_of(ctx, front, r), "nondominated's mask against the filtered set without one")
        # the dominated rows add no volume: the same number to rounding, not the same bits (another grid)
        assert abs(R.LD(a[0]) - want) <= bar(n, k, want)


# ----------------------------------------------------------------------------------------------- contributions
def _check_contributions(ctx, P, r, k, rows=None):
    n = int(R.kept_rows(P, r).sum())
    hv, c = ctx.hypervolume_contributions(put([P])[:, 0, :], r)
    hv, c = hv.cpu().numpy(), c.cpu().numpy()
    assert c.shape == (len(P),) and c.dtype == np.float64
    want_hv, want = R.contributions(P, r, rows=rows)
    rows = range(len(P)) if rows is None else rows
    tol = 2 * bar(n, k, want_hv)
    assert abs(R.LD(hv[0]) - want_hv) <= bar(n, k, want_hv)
    worst = max([float(abs(R.LD(c[i]) - w)) for i, w in zip(rows, want)] + [0.0])
    print(f"k={k} n={n}: worst contribution error {worst / (U * float(want_hv)) if n else 0:.2f} ulp of HV "
          f"(bar {2 * (n + k + 48)})")
    for i, w in zip(rows, want):
        assert abs(R.LD(c[i]) - w) <= tol, (i, c[i], w)
    kept = R.kept_rows(P, r)
    assert np.all(c[~kept] == 0.0) and not np.signbit(c[~kept]).any(), "dropped rows get exactly 0.0"
    return c, kept


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k,n", [(k, n) for k in (1, 2, 3) for n in (0, 1, 2, 63, 64, 65)] +
                         [(4, 1), (4, 20), (4, 70), (5, 12), (6, 8), (8, 5)])
def test_contributions_are_hypervolume_differences(ctx, kind, k, n):
    P, r, _ = case(kind, k, n)
    c, kept = _check_contributions(ctx, P, r, k)
    if n >= 8:
        # dressed(): two exact duplicates of kept rows and two rows that kept rows dominate — at least four zeros,
        # and they are exact: every variant is summed over the whole set's grid in the same tree
        vals, counts = np.unique(P[kept], axis=0, return_counts=True)
        dup = np.array([counts[np.all(vals == row, axis=1)][0] > 1 for row in P[kept]])
        assert dup.sum() >= 4
        assert np.all(c[kept][dup] == 0.0)
        le = np.all(P[kept][:, None, :] <= P[kept][None, :, :], axis=2) & \
            np.any(P[kept][:, None, :] < P[kept][None, :, :], axis=2)
        dominated = le.any(axis=0)
        assert dominated.sum() >= (2 if kind == "sphere" else 1)
        assert np.all(c[kept][dominated] == 0.0)
        assert np.all(c >= 0.0)


@pytest.mark.parametrize("n", [1023, 1024])
def test_contributions_at_the_point_limit(ctx, n):
    """k = 3 at 1023 / 1024 kept rows: 1024 / 1025 variants; the reference recomputes a sample of rows."""
    P, r, _ = case("sphere", 3, n)
    kept = np.flatnonzero(R.kept_rows(P, r))
    rows = sorted(set(kept[[0, 1, n // 2, n - 1]]) | set(np.flatnonzero(~R.kept_rows(P, r))[:2]))
    _check_contributions(ctx, P, r, 3, rows=rows)


def test_least_contributor_is_the_row_to_drop(ctx):
    """What archive truncation asks: the kept row with the least contribution, against the host's recomputation."""
    P = R.sphere(np.random.default_rng(12), 40, 3)
    r = np.full(3, 1.1)
    _, c = ctx.hypervolume_contributions(torch.as_tensor(np.ascontiguousarray(P.T), device="cuda:0"), r)
    full = pareto.hypervolume(P, r)
    host = np.array([full - pareto.hypervolume(np.delete(P, i, axis=0), r) for i in range(len(P))])
    assert int(torch.argmin(c)) == int(np.argmin(host))
    assert np.allclose(c.cpu().numpy(), host, rtol=0, atol=1e-13 * full)


# ----------------------------------------------------------------------------------------------- refusals
def test_return_codes_and_untouched_outputs(ctx):
    lib, h = ctx.lib, ctx._h
    N = 1025
    Y = torch.as_tensor(np.ascontiguousarray(R.sphere(np.random.default_rng(1), N, 2).T), device="cuda:0")
    hv = torch.full((17,), -5.0, dtype=torch.float64, device="cuda:0")
    cb = torch.full((N + 1,), -7.0, dtype=torch.float64, device="cuda:0")
    m = torch.ones(N, dtype=torch.uint8, device="cuda:0")
    r = (ctypes.c_double * 8)(*([1.1] * 8))
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)       # noqa: E731
    f, g = lib.omb_hypervolume, lib.omb_hypervolume_contrib
    # 1025 kept rows: refused after the first launch, nothing written
    assert f(h, 2, 1, P(Y), N, N, None, N, r, P(hv)) == OMB_EUNSUP
    assert b"1024" in lib.omb_last_error(h)
    assert g(h, 2, P(Y), N, N, P(m), r, P(hv), P(cb)) == OMB_EUNSUP
    torch.cuda.synchronize()
    assert hv.eq(-5.0).all() and cb.eq(-7.0).all()
    with pytest.raises(OMBError) as e:
        ctx.hypervolume(Y, [1.1, 1.1])
    assert e.value.code == OMB_EUNSUP
    with pytest.raises(OMBError) as e:
        ctx.hypervolume_contributions(Y, [1.1, 1.1])
    assert e.value.code == OMB_EUNSUP
    # one row fewer — through the mask, or below another reference point — is served
    m[3] = 0
    assert f(h, 2, 1, P(Y), N, N, P(m), N, r, P(hv)) == 0
    torch.cuda.synchronize()
    assert float(hv[0]) > 0 and hv[1:].eq(-5.0).all()
    hv.fill_(-5.0)
    # the work cap: k = 8, 30 rows in general position are 30^6·30 point tests per set, 16 such sets are above it
    Z = torch.as_tensor(np.ascontiguousarray(R.sphere(np.random.default_rng(2), 30, 8).T), device="cuda:0")
    Z16 = Z[:, None, :].expand(8, 16, 30).contiguous()
    assert 16 * 30 ** 7 > _lib.HV_MAX_WORK > 30 ** 7
    assert f(h, 8, 16, P(Z16), 30, 30, None, 30, r, P(hv)) == OMB_EUNSUP
    assert b"point tests" in lib.omb_last_error(h)
    torch.cuda.synchronize()
    assert hv.eq(-5.0).all()

    ok = (2, 1, P(Y), N, 40, P(m), 40, r, P(hv))
    assert f(h, *ok) == 0

    def with_(**kw):
        names = ("k", "S", "y", "ld", "N", "mask", "ldm", "r", "hv")
        a = dict(zip(names, ok))
        a.update(kw)
        return f(h, *[a[n] for n in names])
    hv.fill_(-5.0)
    torch.cuda.synchronize()
    bad_r = [(ctypes.c_double * 8)(*([1.1, v] + [1.1] * 6)) for v in (np.nan, np.inf, -np.inf)]
    for kw in [dict(k=0), dict(k=9), dict(S=0), dict(S=17), dict(N=-1), dict(ld=39), dict(ldm=39), dict(r=None),
               dict(hv=None), dict(y=None), dict(y=P(Y, 4)), dict(hv=P(hv, 4))] + [dict(r=b) for b in bad_r]:
        assert with_(**kw) == OMB_EINVAL, kw
        assert b"" != lib.omb_last_error(h)
    big = (1 << 24) + 1
    assert with_(N=big, ld=big, ldm=big) == OMB_EUNSUP
    assert with_(k=0, N=big, ld=big, ldm=big) == OMB_EINVAL and with_(N=big, ld=big, ldm=big - 1) == OMB_EINVAL
    assert with_(N=big, ld=big, ldm=big, r=bad_r[0]) == OMB_EINVAL
    assert with_(k=1, r=bad_r[0]) == 0                              # r_1 is not read at k = 1
    okc = (2, P(Y), N, 40, P(m), r, P(hv), P(cb))

    def withc(**kw):
        names = ("k", "y", "ld", "N", "mask", "r", "hv", "contrib")
        a = dict(zip(names, okc))
        a.update(kw)
        return g(h, *[a[n] for n in names])
    hv.fill_(-5.0)
    torch.cuda.synchronize()
    for kw in (dict(k=0), dict(k=9), dict(N=-1), dict(ld=39), dict(r=None), dict(r=bad_r[1]), dict(hv=None),
               dict(contrib=None), dict(y=None), dict(y=P(Y, 4)), dict(hv=P(hv, 4)), dict(contrib=P(cb, 4))):
        assert withc(**kw) == OMB_EINVAL, kw
    assert withc(N=big, ld=big) == OMB_EUNSUP
    torch.cuda.synchronize()
    assert hv.eq(-5.0).all() and cb.eq(-7.0).all()                   # refusals wrote nothing
    assert withc() == 0 and withc(mask=None) == 0 and withc(mask=P(m, 1)) == 0      # the mask is bytes, or absent
    torch.cuda.synchronize()
    assert float(hv[0]) > 0 and hv[1:].eq(-5.0).all() and cb[:40].ge(0).all() and cb[40:].eq(-7.0).all()
    # N = 0 writes the zeros alone, null y and mask allowed
    hv.fill_(-5.0)
    cb.fill_(-7.0)
    assert f(h, 3, 16, None, 0, 0, None, 0, r, P(hv)) == 0 and g(h, 3, None, 0, 0, None, r, P(hv, 128), P(cb)) == 0
    torch.cuda.synchronize()
    assert hv[:16].eq(0).all() and float(hv[16]) == 0.0 and cb.eq(-7.0).all()
    # through AcqContext
    for bad in (torch.zeros((2, 4), device="cuda:0", dtype=torch.float32), torch.zeros((2, 4), dtype=torch.float64),
                torch.zeros((4, 2), dtype=torch.float64, device="cuda:0").T):
        with pytest.raises(ValueError):
            ctx.hypervolume(bad, [1.0, 1.0])
        with pytest.raises(ValueError):
            ctx.hypervolume_contributions(bad, [1.0, 1.0])
    y4 = torch.zeros((2, 4), dtype=torch.float64, device="cuda:0")
    for bad_ref in ([1.0], [1.0, 1.0, 1.0]):
        with pytest.raises(ValueError, match="reference point"):
            ctx.hypervolume(y4, bad_ref)
    with pytest.raises(OMBError) as e:
        ctx.hypervolume(y4, [1.0, np.inf])
    assert e.value.code == OMB_EINVAL
    for bad_mask in (torch.ones(3, dtype=torch.bool, device="cuda:0"), torch.ones(4, dtype=torch.bool),
                     torch.ones(4, dtype=torch.float64, device="cuda:0")):
        with pytest.raises(ValueError, match="mask"):
            ctx.hypervolume(y4, [1.0, 1.0], mask=bad_mask)
    with pytest.raises(ValueError):
        ctx.hypervolume_contributions(torch.zeros((2, 3, 4), dtype=torch.float64, device="cuda:0"), [1.0, 1.0])
    e0 = ctx.hypervolume(torch.zeros((3, 0), dtype=torch.float64, device="cuda:0"), [1.0, 1.0, 1.0])
    assert tuple(e0.shape) == (1,) and float(e0[0]) == 0.0
    hv0, c0 = ctx.hypervolume_contributions(torch.zeros((3, 0), dtype=torch.float64, device="cuda:0"), [1.0] * 3)
    assert float(hv0[0]) == 0.0 and tuple(c0.shape) == (0,)


# ----------------------------------------------------------------------------------------------- the engine
@pytest.fixture(scope="module")
def engine():
    import _paths_reference as PR
    from optimobo_amd.acquisition import AcquisitionEngine
    states = [PR.make_state(30, 2, "matern52", 5 + o, noise=1e-3, obj=o) for o in range(3)]
    eng = AcquisitionEngine(0).load_models(states)
    eng.sample_paths(5, n_features=64, seed=1, lower=np.zeros(2), upper=np.ones(2))
    return eng


def test_path_front_hypervolumes(engine):
    eng = engine
    Xc = torch.as_tensor(np.random.default_rng(2).uniform(size=(3001, 2)), device="cuda:0")
    Y = eng.path_values(Xc)
    ref = (Y.amax(dim=(1, 2)) + 0.5).cpu().numpy()
    got = eng.path_front_hypervolumes(Xc, ref)
    assert tuple(got.shape) == (5,) and got.dtype == torch.float64 and got.is_cuda
    mask, _ = eng.nondominated(Y, 5)
    by_hand = eng.hypervolume(Y, ref, 5, mask)
    assert torch.equal(got, by_hand), "the three calls made by hand"
    fronts = eng.path_fronts(Xc)
    g = got.cpu().numpy()
    for s, (_, vals) in enumerate(fronts):
        F = vals.cpu().numpy()
        want = R.hv_grid(F, ref)
        assert abs(R.LD(g[s]) - want) <= bar(len(F), 3, want), (s, g[s], want)
        assert abs(g[s] - pareto.hypervolume(F, ref)) <= 1e-12 * g[s]
    assert len(set(g.tolist())) == 5                            # five draws, five fronts
    # host values take the same road, and the engine's other state is left alone
    F0 = fronts[0][1].T.contiguous()
    assert_bits(eng.hypervolume(F0.cpu().numpy(), ref).cpu().numpy(), g[0:1], "the front as host values")
    hv, c = eng.hypervolume_contributions(F0, ref)
    assert_bits(hv.cpu().numpy(), g[0:1], "the front's hypervolume through the contributions entry")
    assert bool((c >= 0).all()) and float(c.max()) > 0          # the points of a front add volume
    assert torch.equal(eng.path_values(Xc), Y)


# ----------------------------------------------------------------------------------------------- the driver
def _dtlz2(x, k):
    x = np.asarray(x, np.float64)
    g = np.sum((x[k - 1:] - 0.5) ** 2)
    F = np.empty(k)
    for i in range(k):
        f = 1.0 + g
        for j in range(k - 1 - i):
            f = f * np.cos(0.5 * np.pi * x[j])
        if i > 0:
            f = f * np.sin(0.5 * np.pi * x[k - 1 - i])
        F[i] = f
    return F


def _solve_k4(**kw):
    import optimobo_amd.algorithms.optimisers as opti
    from optimobo_amd.problem import ElementwiseProblem

    class DTLZ2(ElementwiseProblem):
        def __init__(self):
            super().__init__(n_var=6, n_obj=4, xl=np.zeros(6), xu=np.ones(6))

        def _evaluate(self, x, out, *args, **kwargs):
            out["F"] = _dtlz2(x, 4)

    np.random.seed(4)
    opt = opti.MultiSurrogateOptimiser(DTLZ2(), np.zeros(4), np.full(4, 2.5), mode="textbook", n_candidates=4096,
                                       seed=6, **kw)
    return opt, opt.solve(budget=3, n_init_samples=16)


def test_driver_trace_on_the_device():
    host_opt, host = _solve_k4()
    dev_opt, dev = _solve_k4(hypervolume="device")
    assert np.array_equal(dev.Xsample, host.Xsample) and np.array_equal(dev.ysample, host.ysample)
    assert dev_opt.hypervolume_fallbacks == 0 and host_opt.hypervolume_fallbacks == 0
    assert len(dev.hypervolume_convergence) == len(host.hypervolume_convergence) == 3
    r = np.full(4, 2.5)
    for i, (a, b) in enumerate(zip(dev.hypervolume_convergence, host.hypervolume_convergence)):
        Yi = host.ysample[:16 + i]
        want, n = R.hv_grid(Yi, r), int(R.kept_rows(Yi, r).sum())
        assert isinstance(a, float) and abs(R.LD(a) - want) <= bar(n, 4, want), (i, a, b)
        assert abs(a - b) <= 1e-12 * b
