"""CPU checks behind the non-dominated filter and the predicted Pareto set:

  * the O(N log N) sort-and-sweep of tests/_nondominated_reference.py against the definition
    (``pareto.nondominated_mask`` less the NaN rows) at N ∈ {1, 2, 257, 2049}, on iid normals, on integers in [0, 4)
    (heavy ties and duplicates) and on the antichain — the sweep is the reference of the GPU tests at sizes the O(N²)
    form cannot reach;
  * ``omb_nondominated`` through the library as it loads without a GPU: exported, typed, and refusing a null context
    whatever else it is given (the order of the argument refusals is swept by tests/asan/omb_nondominated_check.cpp
    on the CPU and checked through ctypes on the GPU by tests/test_gpu_nondominated.py);
  * the ``model_front`` keyword's validation on every driver class, and ``Res().model_pf_*`` defaulting to None;
  * ``AcquisitionEngine.predicted_front``'s independence of ``chunk`` on an engine whose posterior, feasibility,
    Sobol' points and filter are numpy functions.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _constraints_fixture as cf
import _nondominated_reference as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------------------------- the references
@pytest.mark.parametrize("N", [1, 2, 257, 2049])
@pytest.mark.parametrize("kind", ["iid", "ties", "antichain"])
def test_sweep_is_the_definition(kind, N):
    rng = np.random.default_rng(1000 * N + len(kind))
    Y = {"iid": lambda: R.iid(rng, N, 2), "ties": lambda: R.ties(rng, N, 2), "antichain": lambda: R.antichain(N, 2)}[kind]()
    want = R.definition(Y)
    got = R.sweep_2d(Y)
    assert got.dtype == bool and np.array_equal(got, want)
    if kind == "antichain":
        assert want.all()
    if kind == "ties" and N >= 257:
        assert 1 < want.sum() < N and len(np.unique(Y[want], axis=0)) < want.sum()      # duplicates, all kept


def test_definition_special_values():
    Y = np.array([[0, 1], [np.nan, 0], [-0.0, 1], [np.inf, -np.inf], [1, np.nan], [-np.inf, 5], [0, 1]])
    assert np.array_equal(R.definition(Y), [True, False, True, True, False, True, True])
    assert np.array_equal(R.sweep_2d(np.delete(Y, [1, 4], axis=0)), [True] * 5)
    assert not R.definition(np.full((4, 3), np.nan)).any()
    assert np.array_equal(R.definition(np.array([[2.0], [1.0], [1.0], [3.0]])), [False, True, True, False])
    assert np.array_equal(R.definition(R.chain(5, 3)), [False] * 4 + [True])
    assert np.array_equal(R.definition(R.chain(5, 3, duplicate=True)), [True] + [False] * 3 + [True])


# ----------------------------------------------------------------------------------------------- the library
def test_entry_is_exported_typed_and_refuses_a_null_context():
    from optimobo_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("liboptimobo_hip.so not built (run __graft_entry__.build())")
    lib = _lib.load()
    src = open(os.path.join(REPO, "include", "optimobo_hip.h")).read()
    for name, nargs in (("omb_nondominated", 9), ("omb_nondominated_stats", 3)):
        assert re.search(r"^int " + name + r"\(", src, re.M) and hasattr(lib, name)
        assert len(_lib.SIGNATURES[name][1]) == nargs
    buf = (ctypes.c_double * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    # no context: OMB_EINVAL before any argument is looked at, valid or hostile
    for k, S, N in ((2, 1, 0), (0, 0, -1), (2 ** 31 - 1, -2 ** 31, 2 ** 62)):
        assert lib.omb_nondominated(None, k, S, p, N, N, p, N, p) == _lib.OMB_EINVAL
        assert lib.omb_nondominated(None, k, S, None, N, N, None, N, None) == _lib.OMB_EINVAL
    assert lib.omb_nondominated_stats(None, None, None) == _lib.OMB_EINVAL


def test_limits_match_the_header():
    from optimobo_amd import _lib
    src = open(os.path.join(REPO, "include", "optimobo_hip.h")).read()
    assert int(re.search(r"#define OMB_NONDOM_SETS\s+(\d+)", src).group(1)) == _lib.NONDOM_SETS == 16
    assert int(re.search(r"#define OMB_NONDOM_POINTS\s+(\d+)", src).group(1)) == _lib.NONDOM_POINTS == 1 << 24


# ----------------------------------------------------------------------------------------------- drivers
def test_model_front_keyword_validation():
    import optimobo_amd.algorithms.optimisers as opti
    from optimobo_amd.algorithms import cparego, emo, keep, parego
    M = opti.MultiSurrogateOptimiser
    p = cf.driver_problem
    o = M(p(), [0, 0], [2, 2], model_front=True)
    assert o.model_front is True and o.model_front_candidates == 1 << 18
    o = M(p(), [0, 0], [2, 2], model_front=True, model_front_candidates=4096, constraints="pof", mode="textbook")
    assert o.model_front is True and o.model_front_candidates == 4096
    for bad in (1, 0, "yes", None):
        with pytest.raises(ValueError, match="model_front must be True or False"):
            M(p(), [0, 0], [2, 2], model_front=bad)
    for bad in (0, -1, 2.5, True, "many", None):
        with pytest.raises(ValueError, match="model_front_candidates"):
            M(p(), [0, 0], [2, 2], model_front=True, model_front_candidates=bad)
    for cls in (opti.MonoSurrogateOptimiser, parego.ParEGO, keep.KEEP, emo.EMO, cparego.ParEGO_C1, cparego.ParEGO_C2):
        with pytest.raises(ValueError, match="does not support model_front=True"):
            cls(p(), [0, 0], [2, 2], model_front=True)
        assert cls(p(), [0, 0], [2, 2], model_front=False).model_front is False
    # off: the instance is the one built without the keyword
    a = vars(M(p(), [0, 0], [2, 2], seed=5))
    b = vars(M(p(), [0, 0], [2, 2], seed=5, model_front=False, model_front_candidates=7))
    assert set(a) == set(b) and "model_front" not in b and "model_front_candidates" not in b
    assert M.model_front is False and M.model_front_candidates == 1 << 18


def test_result_attributes_default_to_none():
    from optimobo_amd.result import Constrained_Res, Res
    r = Res(None, None, None, None, None, 2, 5)
    c = Constrained_Res(*([None] * 9), 2, 5)
    for obj in (r, c):
        assert obj.model_pf_inputs is None and obj.model_pf_mean is None and obj.model_pf_var is None
        assert not any(key.startswith("model_pf") for key in vars(obj))


# ----------------------------------------------------------------------------------------------- predicted_front
class _HostContext:
    """AcqContext's part in ``predicted_front`` as numpy functions on CPU tensors."""

    def __init__(self, d):
        self.d, self.calls = d, []

    def set_sobol(self, d, lo, hi, seed=None):
        self.lo, self.hi, self.seed = np.asarray(lo, float), np.asarray(hi, float), seed

    def sobol(self, start, N):
        # a fixed sequence addressed by index, as the device's is
        i = np.arange(start, start + N, dtype=np.float64)[:, None]
        u = np.modf((i + 1.0) * np.array([0.6180339887498949, 0.7548776662466927, 0.5698402909980532])[:self.d])[0]
        return torch.as_tensor(self.lo + u * (self.hi - self.lo))

    def feasibility(self, mu, var, pof_eps):
        return torch.as_tensor(cf.pof(mu.numpy(), var.numpy(), pof_eps))

    def nondominated(self, Y, S=1):
        self.calls.append(Y.shape[1])
        m = R.definition(Y.numpy().T)
        return torch.as_tensor(m[None, :]), torch.as_tensor([int(m.sum())])


def _host_engine(d, k, n_con):
    from optimobo_amd.acquisition import AcquisitionEngine
    eng = object.__new__(AcquisitionEngine)
    eng.device = torch.device("cpu")
    eng.ctx = _HostContext(d)
    eng.n_obj = k + n_con

    def posterior(X):
        x = X.numpy()
        f = [x[:, 0] + 0.1 * np.sin(7 * x[:, 1]), 1.0 - np.sqrt(np.abs(x[:, 0])) + x[:, 1] ** 2,
             np.cos(3 * x.sum(1))][:k]
        g = [0.8 - x[:, 0] - x[:, 1], x[:, 1] - 0.9][:n_con]
        mu = np.array(f + g)
        return torch.as_tensor(mu), torch.as_tensor(0.01 + 0.02 * np.abs(np.sin(5 * mu)))
    eng.posterior = posterior
    return eng


@pytest.mark.parametrize("k, n_con", [(2, 0), (3, 0), (2, 2)])
def test_predicted_front_does_not_depend_on_chunk(k, n_con):
    d = 2
    inc = np.random.default_rng(k).uniform(0, 1, (40, d))
    inc[7] = inc[3]                                      # a duplicated row: both stay or both go
    kw = dict(n_candidates=3000, seed=4, n_con=n_con, include=inc)
    eng = _host_engine(d, k, n_con)
    one = eng.predicted_front([0, 0], [1, 1], chunk=1 << 18, **kw)
    assert eng.ctx.calls[0] <= 3040 and len(eng.ctx.calls) == 2
    # the host recomputation: every candidate at once
    X = np.vstack([inc, eng.ctx.sobol(0, 3000).numpy()])
    mu, var = (t.numpy() for t in eng.posterior(torch.as_tensor(X)))
    feas = cf.pof(mu[k:], var[k:], 1e-5) >= 0.5 if n_con else np.ones(len(X), bool)
    idx = np.flatnonzero(feas)[R.definition(mu[:k, feas].T)]
    assert 3 < len(idx) < len(X) and np.array_equal(one["index"], idx)
    assert np.array_equal(one["X"], X[idx]) and np.array_equal(one["mean"], mu[:k, idx].T)
    assert np.array_equal(one["var"], var[:k, idx].T) and one["info"]["feasible"] == feas.sum()
    assert one["info"]["candidates"] == 3040 and one["info"]["chunk_survivors"] == [len(idx)]
    if n_con:
        assert 0 < feas.sum() < len(X)
    for chunk in (1000, 37, 3040, 13):                  # pieces inside the included rows, across their end, one piece
        eng = _host_engine(d, k, n_con)
        got = eng.predicted_front([0, 0], [1, 1], chunk=chunk, **kw)
        assert len(got["info"]["chunk_survivors"]) == -(-3040 // chunk)
        for key in ("X", "mean", "var", "index"):
            assert np.array_equal(got[key], one[key]), (chunk, key)
        assert got["info"]["feasible"] == one["info"]["feasible"]


def test_predicted_front_without_a_feasible_candidate_is_empty():
    eng = _host_engine(2, 2, 2)
    out = eng.predicted_front([0, 0], [1, 1], n_candidates=500, n_con=2, min_feasibility=1.5, include=np.zeros((3, 2)),
                              chunk=128)
    assert out["info"]["feasible"] == 0 and out["info"]["chunk_survivors"] == [0, 0, 0, 0]
    assert out["X"].shape == (0, 2) and out["mean"].shape == (0, 2) and out["var"].shape == (0, 2)
    assert out["index"].shape == (0,) and out["index"].dtype == np.int64
    with pytest.raises(ValueError, match="n_con"):
        eng.predicted_front([0, 0], [1, 1], n_con=4)
    with pytest.raises(ValueError, match="columns"):
        eng.predicted_front([0, 0], [1, 1], include=np.zeros((3, 3)))
