"""GPU: omb_nondominated against the host definition — ``pareto.nondominated_mask`` less the NaN rows —
bit for bit: every k, S and tile edge on iid normals, heavy ties, the antichain and the chain (a dominator in the last
tile only), special values, the S-batching, the independence of pitch and column offset, 2^18 points against the
sort-and-sweep, a set large enough for three tile passes, the return codes and the state a call must leave alone.
The host definition costs 1.5 s at N = 5000: that size once, N ≤ 2049 elsewhere, one reference per (k, N) shared by
the three S."""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _nondominated_reference as R  # noqa: E402

from optimobo_amd import _lib, pareto  # noqa: E402
from optimobo_amd._lib import OMB_EINVAL, OMB_EUNSUP, OMBError  # noqa: E402

KINDS = ("iid", "ties", "antichain", "chain", "chain_dup")


@pytest.fixture(scope="module")
def ctx():
    from optimobo_amd.device import AcqContext
    c = AcqContext(0)
    yield c
    c.close()


def _kind(kind, N, k, rng):
    return {"iid": lambda: R.iid(rng, N, k), "ties": lambda: R.ties(rng, N, k), "antichain": lambda: R.antichain(N, k),
            "chain": lambda: R.chain(N, k), "chain_dup": lambda: R.chain(N, k, duplicate=True)}[kind]()


@functools.lru_cache(maxsize=None)
def pool(k, N):
    """16 different sets (N, k) and their masks by the definition: the five kinds, then each of them with its rows
    rolled by 1, 2, … places (the mask rolls with them), so that one reference per kind serves every S."""
    rng = np.random.default_rng(97 * k + N)
    sets = [_kind(kind, N, k, rng) for kind in KINDS]
    masks = [R.definition(Y) for Y in sets]
    for s in range(5, 16):
        sets.append(np.roll(sets[s % 5], s, axis=0))
        masks.append(np.roll(masks[s % 5], s))
    return sets, masks


def call(ctx, sets, pad=3, pad_m=5, col=0):
    """The sets (each (N, k)) as one pitched (k, S, N) view at column ``col`` of a buffer whose other columns hold
    −inf — a point that would dominate everything, were it read — into a pitched mask among sentinel bytes."""
    S, (N, k) = len(sets), sets[0].shape
    buf = torch.full((k, S, col + N + pad), -np.inf, dtype=torch.float64, device="cuda:0")
    buf[:, :, col:col + N] = torch.as_tensor(np.stack([Y.T for Y in sets], 1), device="cuda:0")
    out = torch.full((S, col + N + pad_m), 7, dtype=torch.uint8, device="cuda:0")
    mask, counts = ctx.nondominated(buf[:, :, col:col + N], S, out=out[:, col:])
    o = out.cpu().numpy()
    assert np.all(o[:, :col] == 7) and np.all(o[:, col + N:] == 7), "mask bytes outside the N columns were written"
    assert mask.dtype == torch.bool and tuple(mask.shape) == (S, N) and counts.dtype == torch.int64
    assert set(np.unique(o[:, col:col + N])) <= {0, 1}
    return mask.cpu().numpy(), counts.cpu().numpy()


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049])
@pytest.mark.parametrize("S", [1, 3, 16])
@pytest.mark.parametrize("k", [1, 2, 3, 5, 8])
def test_mask_and_count_are_the_definition(ctx, k, S, N):
    sets, masks = pool(k, N)
    groups = {1: [[s] for s in range(5)], 3: [[0, 1, 2], [3, 4, 5]], 16: [list(range(16))]}[S]
    for g in groups:
        mask, counts = call(ctx, [sets[s] for s in g])
        for row, s in enumerate(g):
            assert np.array_equal(mask[row], masks[s]), (k, S, N, s, int(mask[row].sum()), int(masks[s].sum()))
            assert counts[row] == masks[s].sum()
    if N >= 2 and k >= 2:       # what the inputs are there for
        assert masks[2].all() and masks[3].sum() == 1 and masks[3][-1] and masks[4].sum() == 2 and masks[4][0]
    assert N < 63 or all(not np.array_equal(sets[a], sets[b]) for a in range(16) for b in range(a))


def test_the_definitions_size_once(ctx):
    """N = 5000: five tiles, the last one short.  Front sizes of the inputs, by the definition: 333 of 5000 iid normals
    at k = 5 and 83 of 5000 integers in [0, 4) at k = 3 are the orders of magnitude."""
    rng = np.random.default_rng(5)
    for Y in (R.iid(rng, 5000, 5), R.ties(rng, 5000, 3)):
        want = R.definition(Y)
        mask, counts = call(ctx, [Y])
        print(f"k = {Y.shape[1]}: {int(want.sum())} of 5000 kept, sieve {ctx.nondominated_stats()}")
        assert 10 < want.sum() < 2500 and np.array_equal(mask[0], want) and counts[0] == want.sum()


def test_special_values(ctx):
    nan, inf = np.nan, np.inf
    core = np.array([[0, 1], [nan, 0], [-0.0, 1], [inf, -inf], [1, nan], [-inf, 5], [0, 1]])
    want = np.array([True, False, True, True, False, True, True])
    assert np.array_equal(R.definition(core), want)
    assert np.array_equal(pareto.nondominated_mask(core), [True] * 7)     # the host filter keeps the NaN rows
    mask, counts = call(ctx, [core])
    assert np.array_equal(mask[0], want) and counts[0] == 5
    # the core among 1500 ordinary points it does not meet (all worse than (0, 1), better than nothing of it), the NaN
    # rows in different tiles; an all-NaN set beside it; a set whose only finite point is +inf everywhere
    rng = np.random.default_rng(11)
    big = np.vstack([core[:3], 2.0 + rng.uniform(size=(1100, 2)), core[3:], 2.0 + rng.uniform(size=(397, 2))])
    sets = [big, np.full_like(big, nan), np.vstack([np.full((len(big) - 1, 2), nan), [[inf, inf]]])]
    refs = [R.definition(Y) for Y in sets]
    assert refs[0].sum() == 5 and refs[1].sum() == 0 and refs[2].sum() == 1
    mask, counts = call(ctx, sets)
    for s in range(3):
        assert np.array_equal(mask[s], refs[s]) and counts[s] == refs[s].sum()
    # k = 1 keeps every occurrence of the minimum, −0.0 and +0.0 alike
    y = np.array([[3.0], [-0.0], [0.0], [nan], [0.0], [inf]])
    mask, counts = call(ctx, [y])
    assert np.array_equal(mask[0], [False, True, True, False, True, False]) and counts[0] == 3


def test_row_s_is_the_single_set_call_on_its_slice(ctx):
    sets, masks = pool(3, 1025)
    together, counts = call(ctx, sets)
    for s in range(16):
        alone, c = call(ctx, [sets[s]])
        assert np.array_equal(alone[0], together[s]) and c[0] == counts[s] == masks[s].sum()


def test_the_mask_does_not_depend_on_pitch_offset_or_call(ctx):
    sets, masks = pool(5, 1025)
    base, _ = call(ctx, sets[:3])
    for pad, pad_m, col in ((0, 0, 0), (1, 2, 1), (61, 3, 7), (1024, 1029, 64)):
        for _ in range(2):
            got, counts = call(ctx, sets[:3], pad=pad, pad_m=pad_m, col=col)
            assert np.array_equal(got, base) and np.array_equal(counts, [m.sum() for m in masks[:3]])
    # (k, N) through the S = 1 form: contiguous, and as a pitched view between columns of −inf
    Yd = torch.as_tensor(np.ascontiguousarray(sets[0].T), device="cuda:0")
    wide = torch.full((5, 1025 + 9), -np.inf, dtype=torch.float64, device="cuda:0")
    wide[:, 4:4 + 1025] = Yd
    for Y in (Yd, wide[:, 4:4 + 1025]):
        m2, c2 = ctx.nondominated(Y)
        assert np.array_equal(m2.cpu().numpy()[0], base[0]) and int(c2[0]) == masks[0].sum()


def test_large_sets_against_the_sweep(ctx):
    rng = np.random.default_rng(18)
    Y = R.iid(rng, 1 << 18, 2)
    want = R.sweep_2d(Y)
    mask, counts = call(ctx, [Y])
    stats = ctx.nondominated_stats()
    print(f"2^18 iid, k = 2: {int(want.sum())} kept, survivors per tile pass {stats}")
    assert np.array_equal(mask[0], want) and counts[0] == want.sum() and 2 <= want.sum() <= 64
    assert len(stats) >= 2 and stats[0] > 1024 >= stats[-1]        # the second pass ran over the survivor list
    A = R.antichain(1 << 16, 2)
    mask, counts = call(ctx, [A, A[::-1].copy()])
    assert mask.all() and np.array_equal(counts, [1 << 16] * 2)
    assert ctx.nondominated_stats() == [1 << 16]                   # nothing to sieve: one pass, then all pairs


def test_three_tile_passes(ctx):
    """2^20 iid normals at k = 3: the list goes A → B → A.  No O(N log N) reference at k = 3, so the mask K is checked
    by what makes it the non-dominated set: K's points do not dominate one another, and every other point is dominated
    by one of them (were a member of K dominated from outside, that point's own dominator in K would dominate it too)."""
    rng = np.random.default_rng(20)
    Y = R.iid(rng, 1 << 20, 3)
    mask, counts = call(ctx, [Y])
    stats = ctx.nondominated_stats()
    K = Y[mask[0]]
    print(f"2^20 iid, k = 3: {len(K)} kept, survivors per tile pass {stats}")
    assert counts[0] == len(K) and 20 < len(K) < 2000 and R.definition(K).all()
    beaten = np.zeros(len(Y), bool)
    for p in K:
        beaten |= np.all(p <= Y, axis=1) & np.any(p < Y, axis=1)
    assert np.array_equal(beaten, ~mask[0])
    assert len(stats) >= 3, stats


def test_return_codes(ctx):
    lib, h = ctx.lib, ctx._h
    y = torch.zeros((2, 40), dtype=torch.float64, device="cuda:0")
    m = torch.full((48,), 7, dtype=torch.uint8, device="cuda:0")
    c = torch.full((17,), -5, dtype=torch.int64, device="cuda:0")
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)       # noqa: E731
    f = lib.omb_nondominated
    ok = (2, 1, P(y), 40, 40, P(m), 48, P(c))
    assert f(h, *ok) == 0

    def with_(**kw):
        names = ("k", "S", "y", "ld", "N", "mask", "ldm", "count")
        a = dict(zip(names, ok))
        a.update(kw)
        return f(h, *[a[n] for n in names])
    for kw in (dict(k=0), dict(k=9), dict(S=0), dict(S=17), dict(N=-1), dict(ld=39), dict(ldm=39), dict(count=None),
               dict(y=None), dict(mask=None), dict(y=P(y, 4)), dict(count=P(c, 4))):
        assert with_(**kw) == OMB_EINVAL, kw
        assert b"" != lib.omb_last_error(h)
    big = (1 << 24) + 1
    assert with_(N=big, ld=big, ldm=big) == OMB_EUNSUP
    assert with_(k=0, N=big, ld=big, ldm=big) == OMB_EINVAL and with_(N=big, ld=big, ldm=big - 1) == OMB_EINVAL
    assert with_(mask=P(m, 1)) == 0                                  # the mask is bytes
    # refusals wrote nothing; N = 0 writes the counts alone, null y and mask allowed
    torch.cuda.synchronize()
    assert int(c[1]) == -5
    m.fill_(7)
    assert f(h, 2, 16, None, 0, 0, None, 0, P(c)) == 0
    torch.cuda.synchronize()
    assert c[:16].eq(0).all() and int(c[16]) == -5 and m.eq(7).all()
    assert ctx.nondominated_stats() == []
    # through AcqContext
    with pytest.raises(OMBError) as e:
        ctx.nondominated(torch.zeros((9, 4), dtype=torch.float64, device="cuda:0"))
    assert e.value.code == OMB_EINVAL
    with pytest.raises(OMBError) as e:
        ctx.nondominated(torch.zeros((1, 17, 4), dtype=torch.float64, device="cuda:0"), 17)
    assert e.value.code == OMB_EINVAL
    for bad in (torch.zeros((2, 4), device="cuda:0", dtype=torch.float32), torch.zeros((2, 4), dtype=torch.float64),
                torch.zeros((2, 3, 4, 5), dtype=torch.float64, device="cuda:0"),
                torch.zeros((4, 2), dtype=torch.float64, device="cuda:0").T):
        with pytest.raises(ValueError):
            ctx.nondominated(bad)
    with pytest.raises(ValueError):
        ctx.nondominated(y, out=torch.zeros((1, 39), dtype=torch.uint8, device="cuda:0"))
    mask, counts = ctx.nondominated(torch.zeros((3, 0), dtype=torch.float64, device="cuda:0"))
    assert tuple(mask.shape) == (1, 0) and int(counts[0]) == 0
    assert _lib.NONDOM_SETS == 16 and _lib.NONDOM_POINTS == 1 << 24


def test_a_call_leaves_plan_posterior_and_paths_alone():
    import _paths_reference as PR
    from optimobo_amd.acquisition import AcquisitionEngine
    states = [PR.make_state(30, 2, "matern52", 5 + o, noise=1e-3, obj=o) for o in range(2)]
    eng = AcquisitionEngine(0).load_models(states)
    rng = np.random.default_rng(2)
    Xc = torch.as_tensor(rng.uniform(size=(777, 2)), device="cuda:0")
    eng.sample_paths(3, n_features=64, seed=1, lower=np.zeros(2), upper=np.ones(2))
    eng.ctx.plan_ei(0.1, 1e-6)
    before = [t.clone() for t in (*eng.ctx.posterior(Xc, 2), eng.ctx.eval(Xc), eng.path_values(Xc))]
    mask, counts = eng.nondominated(before[0])
    want = R.definition(before[0].cpu().numpy().T)
    assert np.array_equal(mask.cpu().numpy()[0], want) and int(counts[0]) == want.sum()
    m2, _ = eng.nondominated(before[0].cpu().numpy())                # host values take the same road
    assert torch.equal(m2, mask)
    after = [*eng.ctx.posterior(Xc, 2), eng.ctx.eval(Xc), eng.path_values(Xc)]
    for a, b in zip(before, after):
        assert torch.equal(a, b)
    assert eng.ctx.plan_kind == ("omb_plan_ei", None)
