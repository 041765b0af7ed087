"""CPU checks behind the device hypervolume:

  * the grid-sweep formula of tests/_hypervolume_reference.py — in ``np.longdouble`` the reference of the GPU tests, in
    ``np.float64`` the plain restatement of the kernel — against ``pareto.hypervolume``, the independent algorithm (a
    recursive sweep of the last objective), on unit-sphere and integer-lattice inputs with duplicates, dominated rows
    and rows on, beyond and far from the reference point, k = 1..6, to 1e-12 relative;
  * its contributions against differences of ``pareto.hypervolume``, and the rows that must get 0;
  * ``omb_hypervolume`` / ``omb_hypervolume_contrib`` through the library as it loads without a GPU: exported, typed,
    and refusing a null context whatever else they are given (the order of the argument refusals is swept by
    tests/asan/omb_hypervolume_check.cpp on the CPU and checked through ctypes on the GPU by
    tests/test_gpu_hypervolume.py);
  * the ``hypervolume`` keyword's validation on every driver class.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import _constraints_fixture as cf
import _hypervolume_reference as R

from optimobo_amd import pareto

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (1, 9), (2, 1), (2, 40), (3, 2), (3, 40), (4, 20), (5, 12), (6, 8)]


def _finite_keepers(P, r):
    """``pareto.hypervolume`` keeps a −inf row (and returns inf): the contract drops it, so the comparison does too."""
    return P[~np.isneginf(P).any(axis=1)]


# ----------------------------------------------------------------------------------------------- the references
@pytest.mark.parametrize("kind", ["sphere", "lattice"])
@pytest.mark.parametrize("k,n", SHAPES)
def test_grid_sweep_is_the_hypervolume(kind, k, n):
    assert np.finfo(R.LD).nmant >= 63, "the reference needs an extended-precision long double"
    P, r = R.dressed(np.random.default_rng(31 * k + n), kind, n, k)
    want = pareto.hypervolume(_finite_keepers(P, r), r)
    assert want > 0
    for dtype in (R.LD, np.float64):
        got = R.hv_grid(P, r, dtype)
        assert got.dtype == dtype
        assert abs(float(got) - want) <= 1e-12 * want, (dtype, float(got), want)
    # the restatement in fp64 against the same formula in extended precision: a few ulp (the bar of the GPU tests,
    # (n + k + 48) ulp, leaves the kernel's tree of additions its room)
    ld, f64 = R.hv_grid(P, r, R.LD), R.hv_grid(P, r, np.float64)
    assert abs(R.LD(f64) - ld) <= 16 * 2.0 ** -53 * ld


def test_grid_sweep_edge_sets():
    r = np.array([1.0, 2.0, 3.0])
    assert R.hv_grid(np.zeros((0, 3)), r) == 0 and R.hv_grid(np.zeros((0, 3)), r, np.float64) == 0
    assert R.hv_grid([[1.0, 0, 0], [0, 2.5, 0], [np.nan, 0, 0], [0, 0, np.inf], [-np.inf, 0, 0]], r) == 0
    assert float(R.hv_grid([[0.5, 1.0, 1.0]], r)) == 0.5 * 1.0 * 2.0
    assert float(R.hv_grid([[0.5, 1.0, 1.0]] * 3 + [[0.75, 1.5, 2.0]], r)) == 1.0        # duplicates, a dominated row
    two = [[0.0, 1.0, 1.0], [0.5, 0.0, 0.0]]                                             # 1·1·2 + 0.5·2·3 − 0.5·1·2
    assert float(R.hv_grid(two, r)) == 4.0 == pareto.hypervolume(np.array(two), r)
    assert float(R.hv_grid([[3.0], [1.25], [7.0]], [4.0])) == 2.75                       # k = 1


@pytest.mark.parametrize("kind", ["sphere", "lattice"])
@pytest.mark.parametrize("k,n", [(1, 9), (2, 12), (3, 12), (4, 10), (5, 8)])
def test_contributions_are_hypervolume_differences(kind, k, n):
    P, r = R.dressed(np.random.default_rng(7 * k + n), kind, n, k)
    hv, c = R.contributions(P, r)
    fin = _finite_keepers(P, r)
    assert abs(float(hv) - pareto.hypervolume(fin, r)) <= 1e-12 * float(hv)
    kept = R.kept_rows(P, r)
    for i in range(len(P)):
        rest = np.delete(P, i, axis=0)
        want = pareto.hypervolume(fin, r) - pareto.hypervolume(_finite_keepers(rest, r), r)
        assert abs(float(c[i]) - want) <= 1e-12 * float(hv), (i, float(c[i]), want)
        if not kept[i]:
            assert c[i] == 0
    # a duplicate adds nothing — exactly, in any precision: its removal changes neither the grid nor a cell's walk; a
    # dominated row's removal takes its values out of the recomputed grid, so here its 0 carries the two sums'
    # rounding (the kernel keeps the whole set's grid for every subset: its 0.0 is exact for both)
    Q = np.vstack((P, P[kept][:1], np.minimum(P[kept][:1] + 1e-3, r - 1e-3)))
    for dtype in (R.LD, np.float64):
        hq, cq = R.contributions(Q, r, dtype, rows=[len(Q) - 2, len(Q) - 1])
        assert cq[0] == 0 and abs(cq[1]) <= 64 * np.finfo(dtype).eps * hq


# ----------------------------------------------------------------------------------------------- the library
def test_entries_are_exported_typed_and_refuse_a_null_context():
    from optimobo_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("liboptimobo_hip.so not built (run __graft_entry__.build())")
    lib = _lib.load()
    src = open(os.path.join(REPO, "include", "optimobo_hip.h")).read()
    for name, nargs in (("omb_hypervolume", 10), ("omb_hypervolume_contrib", 9)):
        assert re.search(r"^int " + name + r"\(", src, re.M) and hasattr(lib, name)
        assert len(_lib.SIGNATURES[name][1]) == nargs
    buf = (ctypes.c_double * 8)(*([1.0] * 8))
    p = ctypes.cast(buf, ctypes.c_void_p)
    # no context: OMB_EINVAL before any argument is looked at, valid or hostile
    for k, S, N in ((2, 1, 0), (0, 0, -1), (2 ** 31 - 1, -2 ** 31, 2 ** 62)):
        assert lib.omb_hypervolume(None, k, S, p, N, N, p, N, buf, p) == _lib.OMB_EINVAL
        assert lib.omb_hypervolume(None, k, S, None, N, N, None, N, None, None) == _lib.OMB_EINVAL
        assert lib.omb_hypervolume_contrib(None, k, p, N, N, p, buf, p, p) == _lib.OMB_EINVAL
        assert lib.omb_hypervolume_contrib(None, k, None, N, N, None, None, None, None) == _lib.OMB_EINVAL
    assert lib.omb_abi_version() == 1


def test_limits_match_the_header():
    from optimobo_amd import _lib
    src = open(os.path.join(REPO, "include", "optimobo_hip.h")).read()
    assert int(re.search(r"#define OMB_HV_POINTS\s+(\d+)", src).group(1)) == _lib.HV_POINTS == 1024
    assert int(re.search(r"#define OMB_HV_MAX_WORK\s+(\d+)LL", src).group(1)) == _lib.HV_MAX_WORK


# ----------------------------------------------------------------------------------------------- drivers
def test_hypervolume_keyword_validation():
    import optimobo_amd.algorithms.optimisers as opti
    from optimobo_amd.algorithms import cparego, emo, keep, parego, turbo
    p = cf.driver_problem
    for cls in (opti.MultiSurrogateOptimiser, opti.MonoSurrogateOptimiser, parego.ParEGO, keep.KEEP, emo.EMO):
        o = cls(p(), [0, 0], [2, 2], hypervolume="device")
        assert o.hypervolume == "device" and o.hypervolume_fallbacks == 0
        assert cls(p(), [0, 0], [2, 2]).hypervolume == "host" and cls.hypervolume == "host"
        for bad in ("gpu", "", None, True, 1, b"device"):
            with pytest.raises(ValueError, match="hypervolume must be 'host' or 'device'"):
                cls(p(), [0, 0], [2, 2], hypervolume=bad)
        # off: the instance is the one built without the keyword
        a, b = vars(cls(p(), [0, 0], [2, 2], seed=5)), vars(cls(p(), [0, 0], [2, 2], seed=5, hypervolume="host"))
        assert set(a) == set(b) and "hypervolume" not in b and "hypervolume_fallbacks" not in b
        assert cls.hypervolume_fallbacks == 0 and set(vars(o)) == set(a) | {"hypervolume", "hypervolume_fallbacks"}
    makers = [lambda **kw: cparego.ParEGO_C1(p(), [0, 0], [2, 2], **kw),
              lambda **kw: cparego.ParEGO_C2(p(), [0, 0], [2, 2], **kw),
              lambda **kw: turbo.TuRBO_1(p(), 2, [0, 0], [2, 2], **kw),
              lambda **kw: turbo.TuRBO_M(p(), [0, 0], [2, 2], 2, 2, **kw)]
    for make in makers:
        with pytest.raises(ValueError, match="does not support hypervolume='device'"):
            make(hypervolume="device")
        with pytest.raises(ValueError, match="hypervolume must be 'host' or 'device'"):
            make(hypervolume="gpu")
        make(hypervolume="host")


def test_host_trace_is_untouched_and_empty_sets_stay_on_the_host(monkeypatch):
    """hypervolume="host" never asks for an engine; "device" does not either for a sample without rows (the
    constrained drivers' trace before anything is feasible)."""
    import optimobo_amd.algorithms._base as base
    import optimobo_amd.algorithms.optimisers as opti

    def no_engine(*a, **kw):
        raise AssertionError("the host trace asked for a device engine")
    monkeypatch.setattr(base, "device_engine", no_engine)
    Y = R.sphere(np.random.default_rng(3), 12, 2)
    o = opti.MultiSurrogateOptimiser(cf.driver_problem(), [0, 0], [1.1, 1.1])
    assert o._hypervolume(Y) == pareto.hypervolume(Y, [1.1, 1.1])
    o = opti.MultiSurrogateOptimiser(cf.driver_problem(), [0, 0], [1.1, 1.1], hypervolume="device")
    assert o._hypervolume(Y[:0]) == 0.0 and o.hypervolume_fallbacks == 0


def test_device_trace_falls_back_on_unsupported_and_counts_it(monkeypatch):
    import optimobo_amd.algorithms._base as base
    import optimobo_amd.algorithms.optimisers as opti
    from optimobo_amd._lib import OMB_EINVAL, OMB_EUNSUP, OMBError

    class Engine:
        def __init__(self, code):
            self.code, self.seen = code, []

        def hypervolume(self, Y, ref):
            self.seen.append((np.array(Y), np.array(ref)))
            raise OMBError(self.code, "refused")
    Y = R.sphere(np.random.default_rng(4), 9, 3)
    o = opti.MultiSurrogateOptimiser(cf.driver_problem(), [0, 0, 0], [1.1, 1.1, 1.1], hypervolume="device")
    eng = Engine(OMB_EUNSUP)
    monkeypatch.setattr(base, "device_engine", lambda device=None: eng)
    assert o._hypervolume(Y) == pareto.hypervolume(Y, [1.1] * 3) and o.hypervolume_fallbacks == 1
    assert eng.seen[0][0].shape == (3, 9) and np.array_equal(eng.seen[0][0], Y.T)       # coordinates along axis 0
    eng.code = OMB_EINVAL                                                               # anything else is an error
    with pytest.raises(OMBError):
        o._hypervolume(Y)
    assert o.hypervolume_fallbacks == 1
