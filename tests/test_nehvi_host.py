"""CPU checks behind the noisy EHVI / noisy EI:

  * ``pareto.pack_box_lists`` / ``pareto.threshold_lists``: shapes, offsets and padding over S ∈ {1, 3, 16} lists of
    different C and B, an empty front among them;
  * the numpy restatement's t_s (tests/_nehvi_reference.py) against the hypervolume difference
    HV(PF_s ∪ {y}) − HV(PF_s) for k = 2, 3 and fronts of 200 points, at 1e-10·Π_j(r_j − min PF_j) — the difference
    cancels: about 10^5 roundings of the larger hypervolume — and for k = 1 against (b_s − y)⁺ exactly;
  * the drivers' ValueErrors for acquisition="nehvi" / "nei", and that the new acquisitions leave vars() with the
    attribute set of acquisition=None;
  * the two entries through the library as it loads without a GPU: exported, typed, and refusing a null context
    whatever else they are given (the order of the argument refusals is swept by tests/asan/omb_nehvi_check.cpp on the
    CPU and checked through ctypes on the GPU by tests/test_gpu_hvi_paths.py).
"""
import ctypes
import os
import re

import numpy as np
import pytest

import _constraints_fixture as cf
import _nehvi_reference as R
from optimobo_amd import pareto

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------------------------- packing
@pytest.mark.parametrize("S", [1, 3, 16])
@pytest.mark.parametrize("k", [2, 3, 4])
def test_pack_box_lists_shapes_offsets_and_padding(k, S):
    rng = np.random.default_rng(100 * k + S)
    sizes = ([9, 0, 4] + list(rng.integers(1, 12, size=16)))[:S]
    r = np.full(k, 1.1)
    fronts = [R.front(k, P, rng) for P in sizes]
    decomps = [pareto.box_decomposition(f, r) for f in fronts]
    coords, off, boxes = pareto.pack_box_lists(decomps)
    C = max(d[0].shape[1] for d in decomps)
    assert coords.shape == (S, k, C) and coords.dtype == np.float64 and coords.flags.c_contiguous
    assert off.shape == (S + 1,) and off.dtype == np.int32 and off[0] == 0
    assert boxes.shape == (off[-1], 2 * k) and boxes.dtype == np.uint16 and boxes.flags.c_contiguous
    assert np.array_equal(np.diff(off), [len(d[2]) for d in decomps]) and np.all(np.diff(off) >= 1)
    for s, (c, n, b) in enumerate(decomps):
        assert np.array_equal(boxes[off[s]:off[s + 1]], b)
        assert np.array_equal(coords[s, :, :c.shape[1]], c)
        assert np.all(coords[s, :, c.shape[1]:] == c[:, -1:]) and np.all(coords[s, :, 0] == -np.inf)
        assert np.all(coords[s, :, -1] == r)
        if sizes[s] == 0:                                # the empty front: one box, the whole of (−∞, r]
            assert len(b) == 1 and np.array_equal(b[0], [0, 1] * k) and n.tolist() == [2] * k
    if S >= 3:
        assert len({d[0].shape[1] for d in decomps}) > 1 and len({len(d[2]) for d in decomps}) > 1
    # the packed lists say what the separate ones say
    y = R.candidates(k, S, 17, rng)
    ts = R.path_values(y, coords, off, boxes)
    for s, (c, _, b) in enumerate(decomps):
        assert np.array_equal(ts[s], R.t_path(y[:, s, :], c, b))


@pytest.mark.parametrize("S", [1, 3, 16])
def test_threshold_lists(S):
    rng = np.random.default_rng(S)
    b, (coords, off, boxes) = R.thresholds_for(S, rng)
    assert coords.shape == (S, 1, 2) and np.all(coords[:, 0, 0] == -np.inf) and np.array_equal(coords[:, 0, 1], b)
    assert np.array_equal(off, np.arange(S + 1)) and off.dtype == np.int32
    assert boxes.shape == (S, 2) and boxes.dtype == np.uint16 and np.all(boxes == [0, 1])
    y = np.concatenate([rng.normal(size=40), b, [np.inf, -np.inf]])
    Y = np.broadcast_to(y, (1, S, y.size))
    ts = R.path_values(Y, coords, off, boxes)
    assert np.array_equal(ts, np.maximum(b[:, None] - y[None, :], 0.0))          # (b_s − y)⁺ exactly
    a = R.alpha(Y, coords, off, boxes)
    assert np.array_equal(a, R.mean_in_order(np.maximum(b[:, None] - y[None, :], 0.0)))
    assert np.all(a[-2] == 0.0) and a[-1] == np.inf


def test_pack_box_lists_refusals():
    d2 = pareto.box_decomposition(np.zeros((0, 2)), [1.0, 1.0])
    d3 = pareto.box_decomposition(np.zeros((0, 3)), [1.0, 1.0, 1.0])
    with pytest.raises(ValueError, match="disagree"):
        pareto.pack_box_lists([d2, d3])
    with pytest.raises(ValueError, match="no decompositions"):
        pareto.pack_box_lists([])
    with pytest.raises(ValueError, match="empty box list"):
        pareto.pack_box_lists([(d2[0], d2[1], d2[2][:0])])


# ----------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("k", [2, 3])
def test_t_s_is_the_hypervolume_difference(k):
    rng = np.random.default_rng(7 + k)
    r = np.full(k, 1.1)
    pf = R.front(k, 200, rng)
    assert len(pareto.calc_pf(pf)) == 200
    coords, _, boxes = pareto.box_decomposition(pf, r)
    y = np.concatenate([R.candidates(k, 1, 12, rng)[:, 0, :].T, pf[:2] - 1e-3, pf[2:4] + 1e-3, r[None, :]])
    t = R.t_path(y.T, coords, boxes)
    hv0 = pareto.hypervolume(pf, r)
    want = np.array([pareto.hypervolume(np.vstack((pf, p[None, :])), r) - hv0 for p in y])
    bar = 1e-10 * np.prod(r - pf.min(axis=0))
    worst = np.abs(t - want).max()
    print(f"k = {k}: {len(boxes)} boxes, worst |t_s - dHV| {worst:.3g}, bar {bar:.3g}")
    assert worst <= bar
    assert np.all(t >= 0.0) and t[-1] == 0.0 and np.any(t > 0.0)
    assert np.all(t[-3:-1] == 0.0)                       # points behind the front improve nothing
    assert np.abs(R.t_path(y.T, coords, boxes, np.longdouble) - t).max() <= bar


def test_nan_and_order_of_the_restatement():
    rng = np.random.default_rng(3)
    _, (coords, off, boxes) = R.lists_for(2, [5, 0, 3], rng)
    y = R.candidates(2, 3, 9, rng)
    y[1, 2, 4] = np.nan
    a = R.alpha(y, coords, off, boxes)
    assert np.isnan(a[4]) and np.isfinite(np.delete(a, 4)).all()
    ts = R.path_values(y, coords, off, boxes)
    assert np.array_equal(np.delete(a, 4), np.delete(((0.0 + ts[0]) + ts[1] + ts[2]) / 3.0, 4))
    assert np.all(R.alpha(np.full((2, 3, 4), 1.1), coords, off, boxes) == 0.0)   # y ≥ r in every path


# ----------------------------------------------------------------------------------------------- drivers
def _wide(n_var):
    from optimobo_amd.problem import ElementwiseProblem

    class Wide(ElementwiseProblem):
        def __init__(self):
            super().__init__(n_var=n_var, n_obj=2, xl=np.zeros(n_var), xu=np.ones(n_var))

        def _evaluate(self, x, out, *args, **kwargs):
            out["F"] = [x.sum(), (1 - x).sum()]
    return Wide()


def test_noisy_acquisition_value_errors():
    import optimobo_amd.algorithms.optimisers as opti
    from optimobo_amd.algorithms import cparego, emo, keep, parego
    M, S = opti.MultiSurrogateOptimiser, opti.MonoSurrogateOptimiser
    p = cf.driver_problem
    for cls, name, other in ((M, "nehvi", "nei"), (S, "nei", "nehvi")):
        for kw in (dict(), dict(mode="textbook"), dict(batch_size=2)):
            o = cls(p(), [0, 0], [2, 2], acquisition=name, **kw)
            assert o.acquisition == name and o.nehvi_samples == 16 and o.nehvi_features == 1024
        o.nehvi_samples = 4                              # class attributes, settable on the instance
        assert o.nehvi_samples == 4 and cls.nehvi_samples == 16
        with pytest.raises(ValueError, match="does not support acquisition="):
            cls(p(), [0, 0], [2, 2], acquisition=other)
        with pytest.raises(ValueError, match="pof"):
            cls(p(), [0, 0], [2, 2], acquisition=name, constraints="pof")
        with pytest.raises(ValueError, match="thompson"):
            cls(p(), [0, 0], [2, 2], acquisition=name, batch_strategy="thompson")
        with pytest.raises(ValueError, match="log_acquisition"):
            cls(p(), [0, 0], [2, 2], acquisition=name, mode="textbook", log_acquisition=True)
        with pytest.raises(ValueError, match="n_var <= 64"):
            cls(_wide(65), [0, 0], [65, 65], acquisition=name)
        assert cls(_wide(64), [0, 0], [64, 64], acquisition=name).acquisition == name
        for bad in ("pes", "NEHVI", 1, ("nehvi",)):
            with pytest.raises(ValueError, match="None or 'mes', 'nehvi' or 'nei'"):
                cls(p(), [0, 0], [2, 2], acquisition=bad)
    with pytest.raises(ValueError, match="acquisition_func"):
        M(p(), [0, 0], [2, 2], acquisition="nehvi").solve(budget=1, acquisition_func=lambda y, w: float(np.dot(y, w)))
    for cls in (parego.ParEGO, keep.KEEP, emo.EMO, cparego.ParEGO_C1, cparego.ParEGO_C2):
        for name in ("nehvi", "nei"):
            with pytest.raises(ValueError, match="does not support acquisition="):
                cls(p(), [0, 0], [2, 2], acquisition=name)


def test_noisy_acquisitions_add_no_instance_attribute():
    import optimobo_amd.algorithms.optimisers as opti
    for cls, name in ((opti.MultiSurrogateOptimiser, "nehvi"), (opti.MonoSurrogateOptimiser, "nei")):
        kw = dict(mode="textbook", seed=5, batch_size=2, polish="auto")
        a = vars(cls(cf.driver_problem(), [0, 0], [2, 2], acquisition=None, **kw))
        b = vars(cls(cf.driver_problem(), [0, 0], [2, 2], acquisition=name, **kw))
        assert set(a) == set(b) and "nehvi_samples" not in b and "nehvi_features" not in b
        for key in set(a) - {"acquisition", "test_problem"}:
            assert np.array_equal(a[key], b[key]), key
        assert a["acquisition"] is None and b["acquisition"] == name and b["_mes_picks"] == 0


# ----------------------------------------------------------------------------------------------- the library
def test_entries_are_exported_typed_and_refuse_a_null_context():
    from optimobo_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("liboptimobo_hip.so not built (run __graft_entry__.build())")
    lib = _lib.load()
    src = open(os.path.join(REPO, "include", "optimobo_hip.h")).read()
    for name, nargs in (("omb_hvi_paths", 11), ("omb_plan_hvi_paths", 7)):
        assert re.search(r"^int " + name + r"\(", src, re.M) and hasattr(lib, name)
        assert len(_lib.SIGNATURES[name][1]) == nargs
    off = (ctypes.c_int32 * 2)(0, 1)
    buf = (ctypes.c_double * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    # no context: OMB_EINVAL before any argument is looked at, valid or hostile
    for k, S, N, C in ((2, 1, 0, 2), (0, 0, -1, 0), (2 ** 31 - 1, -2 ** 31, 2 ** 62, 2 ** 31 - 1)):
        assert lib.omb_hvi_paths(None, k, S, p, N, N, p, C, ctypes.cast(off, ctypes.c_void_p), p, p) == _lib.OMB_EINVAL
        assert lib.omb_hvi_paths(None, k, S, None, N, N, None, C, None, None, None) == _lib.OMB_EINVAL
        assert lib.omb_plan_hvi_paths(None, k, S, p, C, ctypes.cast(off, ctypes.c_void_p), p) == _lib.OMB_EINVAL
        assert lib.omb_plan_hvi_paths(None, k, S, None, C, None, None) == _lib.OMB_EINVAL


def test_chunk_constant_matches_the_header():
    from optimobo_amd import _lib
    src = open(os.path.join(REPO, "include", "optimobo_hip.h")).read()
    m = re.search(r"#define OMB_HVI_PATHS_CHUNK\s+(\d+)", src)
    assert m and int(m.group(1)) == _lib.HVI_PATHS_CHUNK
    assert re.search(r"OMB_DEBUG_HVI_PATHS_CHUNK\s*=\s*(\d+)", src).group(1) == str(_lib.DEBUG_HVI_PATHS_CHUNK)
