"""CPU: constraints through sample paths — what needs no GPU.

  * ``pareto.feasible_fronts`` on hand-made path values: a path with no feasible row, one with all rows feasible,
    k = 1 and k = 2.
  * tests/_nehvi_con_reference.py: at eta = 0 it is mean_s(t_s·1[feasible]) of tests/_nehvi_reference.py exactly; the
    violation score ranks every feasible candidate above every infeasible one and the infeasible ones by their total
    violation; the sigmoid tends to the indicator.
  * the drivers' ``constraints="paths"``: the ValueErrors, the accepted combinations, and that ``constraints=None`` /
    ``"pof"`` instances carry the attributes they carried before.
  * the library's new symbols are typed as the header declares them.
"""
import ctypes
import os

import numpy as np
import pytest

import _constraints_fixture as cf
import _nehvi_con_reference as RC
import _nehvi_reference as R

from optimobo_amd import _lib, pareto


def _opti():
    from optimobo_amd.algorithms import optimisers
    return optimisers


# --------------------------------------------------------------------------------------------- feasible_fronts
def test_feasible_fronts_two_objectives():
    #            row:   0     1     2     3
    F = np.array([[[0.1, 0.5, 0.9, 0.4], [0.1, 0.5, 0.9, 0.4], [0.2, 0.6, 0.8, 0.3]],
                  [[0.9, 0.5, 0.1, 0.4], [0.9, 0.5, 0.1, 0.4], [0.7, 0.6, 0.2, 0.9]]])          # (2, 3, 4)
    G = np.array([[[-1.0, -1.0, -1.0, -1.0], [1.0, 0.5, 0.1, 2.0], [-0.1, 0.0, 0.3, -2.0]],
                  [[-1.0, -0.5, -0.1, 0.0], [-1.0, -1.0, -1.0, -1.0], [-0.1, -0.2, -0.3, 0.4]]])  # (2, 3, 4)
    r = np.array([1.0, 1.0])
    fronts, decomps = pareto.feasible_fronts(F, G, r)
    # path 0: every row feasible (g = 0 counts) — the front of all four rows, row 1 dominated by row 3
    want0 = pareto.calc_pf(np.ascontiguousarray(F[:, 0, :].T))
    assert sorted(map(tuple, fronts[0])) == sorted(map(tuple, want0)) and len(want0) == 3
    # path 1: constraint 0 is violated everywhere — the empty front and its one box
    assert fronts[1].shape == (0, 2) and len(decomps[1][2]) == 1
    # path 2: rows 0 and 1 (row 2 fails constraint 0, row 3 constraint 1)
    assert sorted(map(tuple, fronts[2])) == [(0.2, 0.7), (0.6, 0.6)]
    for pf, d in zip(fronts, decomps):
        ref = pareto.box_decomposition(pf, r)
        assert all(np.array_equal(a, b) for a, b in zip(d, ref))
    coords, off, boxes = pareto.pack_box_lists(decomps)
    assert coords.shape[:2] == (3, 2) and off[0] == 0 and off[-1] == len(boxes)
    # the empty front's box is the whole of (−∞, r]: its improvement is Π (r − y)
    y = np.array([[0.25], [0.5]])
    assert R.t_path(y, *[decomps[1][0], decomps[1][2]])[0] == 0.75 * 0.5


def test_feasible_fronts_one_objective():
    F = np.array([[[3.0, 1.0, 2.0], [3.0, 1.0, 2.0], [5.0, 4.0, 7.0]]])                      # (1, 3, 3)
    G = np.array([[[-1.0, 1.0, -1.0], [-1.0, -1.0, 0.0], [0.1, 0.2, 0.3]]])
    b, decomps = pareto.feasible_fronts(F, G, None)
    # the feasible minimum; every row feasible: the minimum; no feasible row: the path's maximum over all rows
    assert np.array_equal(b, [2.0, 1.0, 7.0])
    want = pareto.threshold_lists(b)
    assert all(np.array_equal(a, c) for d, w in zip(decomps, want) for a, c in zip(d, w))
    nan = G.copy()
    nan[0, 1, 1] = np.nan                                                    # a NaN constraint value is not feasible
    assert np.array_equal(pareto.feasible_fronts(F, nan, None)[0], [2.0, 2.0, 7.0])
    with pytest.raises(ValueError, match="max_point"):
        pareto.feasible_fronts(F, G, np.array([1.0]))
    with pytest.raises(ValueError, match="max_point"):
        pareto.feasible_fronts(np.concatenate([F, F]), G, None)
    with pytest.raises(ValueError, match="feasible_fronts"):
        pareto.feasible_fronts(F, G[:, :2], None)


# ------------------------------------------------------------------------------------------------ restatement
@pytest.mark.parametrize("k,c,S", [(1, 1, 3), (2, 1, 16), (2, 2, 3), (3, 2, 3), (1, 7, 16)])
def test_restatement_at_eta_0_is_the_mean_of_the_feasible_paths_improvements(k, c, S):
    packed, y = RC.case(k, c, S, N=200)
    feas = RC.check_mix(y[k:])
    ts = R.path_values(y[:k], *packed)
    a, u = RC.alpha(y, c, *packed)
    assert np.array_equal(u, ts * feas) and np.array_equal(a, R.mean_in_order(ts * feas))
    assert np.any(a > 0) and np.any(u[feas] > 0) and np.all(u[~feas] == 0.0)
    # no constraints: _nehvi_reference itself
    a0, u0 = RC.alpha(y[:k], 0, *packed)
    assert np.array_equal(a0, R.alpha(y[:k], *packed)) and np.array_equal(u0, ts)


def test_violation_score_orders_feasible_above_infeasible():
    packed, y = RC.case(2, 2, 3, N=200)
    feas = RC.check_mix(y[2:])
    _, u = RC.alpha(y, 2, *packed, violation=True)
    _, plain = RC.alpha(y, 2, *packed)
    assert np.array_equal(u[feas], plain[feas]) and np.all(u[feas] >= 0) and np.all(u[~feas] < 0)
    viol = np.maximum(y[2], 0) + np.maximum(y[3], 0)
    assert np.array_equal(u[~feas], -viol[~feas])
    for s in range(3):                                   # under every draw: feasible first, then by violation
        order = np.argsort(-u[s], kind="stable")
        nf = int(feas[s].sum())
        assert np.all(feas[s][order[:nf]]) and not np.any(feas[s][order[nf:]])
        assert np.all(np.diff(viol[s][order[nf:]]) >= 0)


def test_sigmoid_and_nan_rules():
    g = np.array([-300.0, -1.0, -0.0, 0.0, 1e-300, 1.0, 300.0])
    w = RC.omega(g, 0.5)
    assert w[0] == 1.0 and w[2] == 0.5 and w[3] == 0.5 and 0 < w[-1] < 1e-200 and np.all(np.diff(w) <= 0)
    assert np.array_equal(RC.omega(g, 1e-3)[[0, 1, 5, 6]], [1.0, 1.0, 0.0, 0.0])       # underflow: the indicator
    assert abs(w[1] + w[5] - 1.0) <= 8 * 2.0 ** -53        # ω(−g) + ω(g) = 1: three roundings each, and the sum's
    assert np.array_equal(RC.omega(g, 0.0), [1, 1, 1, 1, 0, 0, 0])
    lw = RC.omega(g, 0.5, np.longdouble)
    assert lw.dtype == np.longdouble and abs(float(lw[1]) - w[1]) <= 4 * 2.0 ** -53
    packed, y = RC.case(1, 1, 3, N=50)
    y = y.copy()
    y[1, 1, 4] = np.nan                                  # a constraint value of path 1
    y[0, 2, 9] = np.nan                                  # an objective value of path 2
    for kw in (dict(), dict(violation=True), dict(eta=0.5)):
        a, u = RC.alpha(y, 1, *packed, **kw)
        assert np.isnan(u[1, 4]) and np.isnan(u[2, 9]) and np.isnan(a[4]) and np.isnan(a[9])
        assert np.isnan(u).sum() == 2 and np.isnan(a).sum() == 2


# ----------------------------------------------------------------------------------------------------- drivers
def test_constraints_paths_value_errors_and_accepted_combinations():
    opti = _opti()
    from optimobo_amd.algorithms import cparego, emo, keep, parego
    M, S = opti.MultiSurrogateOptimiser, opti.MonoSurrogateOptimiser
    P = cf.driver_problem

    def mk(cls, **kw):
        return cls(P(), [0, 0], [2, 2], constraints="paths", **kw)
    # accepted: the sampled-front acquisition (any batch size, believer) or a Thompson batch (either sampler)
    for kw in (dict(acquisition="nehvi"), dict(acquisition="nehvi", batch_size=3), dict(batch_strategy="thompson"),
               dict(batch_strategy="thompson", batch_size=4, thompson_sampler="paths"),
               dict(acquisition="nehvi", mode="textbook")):
        o = mk(M, **kw)
        assert o.constraints == "paths" and o.n_con == 1 and o.paths_eta == 0.0 and "paths_eta" not in vars(o)
    for kw in (dict(acquisition="nei"), dict(acquisition="nei", batch_size=2), dict(batch_strategy="thompson"),
               dict(batch_strategy="thompson", thompson_sampler="paths", batch_size=2)):
        assert mk(S, **kw).constraints == "paths"
    assert S(P(n_ieq_constr=7), [0, 0], [2, 2], constraints="paths", acquisition="nei").n_con == 7
    assert M.paths_eta == 0.0 and S.paths_eta == 0.0
    # refused: saying what it needs
    for cls in (M, S):
        for kw in (dict(), dict(batch_size=2), dict(acquisition="mes"),
                   dict(log_acquisition=True, mode="textbook")):
            with pytest.raises(ValueError, match="constraints='paths'.*needs acquisition='nehvi'"):
                mk(cls, **kw)
        with pytest.raises(ValueError, match="n_ieq_constr"):
            cls(P(n_ieq_constr=0), [0, 0], [2, 2], constraints="paths", batch_strategy="thompson")
        with pytest.raises(ValueError, match="equality"):
            cls(P(n_eq_constr=1), [0, 0], [2, 2], constraints="paths", batch_strategy="thompson")
        with pytest.raises(ValueError, match="None or 'pof'"):
            cls(P(), [0, 0], [2, 2], constraints="path")
        with pytest.raises(ValueError, match="None or 'pof'"):
            cls(P(), [0, 0], [2, 2], constraints=["paths"])
    with pytest.raises(ValueError, match="does not support acquisition='nei'"):
        mk(M, acquisition="nei")
    with pytest.raises(ValueError, match="does not support acquisition='nehvi'"):
        mk(S, acquisition="nehvi")
    with pytest.raises(ValueError, match="8 models"):
        M(P(n_ieq_constr=7), [0, 0], [2, 2], constraints="paths", acquisition="nehvi")
    with pytest.raises(ValueError, match="path_gradients=True does not support constraints='paths'"):
        mk(M, acquisition="nehvi", path_gradients=True)
    with pytest.raises(ValueError, match="path_gradients=True does not support constraints='paths'"):
        mk(S, batch_strategy="thompson", thompson_sampler="paths", path_gradients=True)
    with pytest.raises(ValueError, match="batch_strategy='thompson'"):          # the existing refusal stands
        mk(M, acquisition="nehvi", batch_strategy="thompson")
    for cls in (emo.EMO, parego.ParEGO, keep.KEEP, cparego.ParEGO_C1, cparego.ParEGO_C2):
        with pytest.raises(ValueError, match="does not support constraints='paths'"):
            cls(P(), [0, 0], [2, 2], constraints="paths")
    # the refusals of "pof" with the sampled-front acquisitions and Thompson batches: as they were
    with pytest.raises(ValueError, match="computes no posterior for the constraint models"):
        M(P(), [0, 0], [2, 2], constraints="pof", acquisition="nehvi")
    with pytest.raises(ValueError, match="computes no posterior for the constraint models"):
        S(P(), [0, 0], [2, 2], constraints="pof", acquisition="nei")
    for cls in (M, S):
        with pytest.raises(ValueError, match="batch_strategy='thompson' does not support constraints='pof'"):
            cls(P(), [0, 0], [2, 2], constraints="pof", batch_strategy="thompson")


_VARS = ['_iteration', '_mes_picks', 'acquisition', 'batch_size', 'batch_strategy', 'constraints', 'device',
         'ideal_point', 'is_ideal_known', 'is_max_known', 'log_acquisition', 'lower', 'max_point', 'mes_candidates',
         'mes_samples', 'mode', 'n_candidates', 'n_obj', 'n_vars', 'noise', 'polish', 'refine_rounds', 'seed', 'starts',
         'test_problem', 'thompson_fallbacks', 'thompson_sampler', 'upper']


def test_other_instances_carry_the_attributes_they_carried():
    opti = _opti()
    for cls in (opti.MultiSurrogateOptimiser, opti.MonoSurrogateOptimiser):
        a = vars(cls(cf.driver_problem(), [0, 0], [2, 2], seed=3))
        b = vars(cls(cf.driver_problem(), [0, 0], [2, 2], seed=3, constraints="pof"))
        c = vars(cls(cf.driver_problem(), [0, 0], [2, 2], seed=3, constraints="paths", batch_strategy="thompson"))
        assert sorted(a) == _VARS and sorted(b) == sorted(_VARS + ["n_con"]) and sorted(c) == sorted(b)
        assert a["constraints"] is None and b["constraints"] == "pof" and c["constraints"] == "paths"
        same = [k for k in _VARS if k not in ("test_problem", "constraints", "batch_strategy")]
        assert all(np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]) for k in same)


# -------------------------------------------------------------------------------------------------- the library
def test_signatures_match_the_header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "optimobo_hip.h")).read()
    for name, nargs in (("omb_hvi_paths_con", 15), ("omb_plan_hvi_paths_con", 9)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        decl = src[src.index(f"int {name}("):]
        assert decl[:decl.index(";")].count(",") == nargs - 1
    assert "#define OMB_CON_VIOLATION 1u" in src and _lib.CON_VIOLATION == 1


def test_null_context_is_einval():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = _lib.load()
    off = (ctypes.c_int32 * 3)(0, 1, 2)
    buf = (ctypes.c_double * 8)()
    p, o = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(off, ctypes.c_void_p)
    assert lib.omb_hvi_paths_con(None, 1, 2, 1, p, 4, 4, p, 2, o, p, 0.0, 0, p, p) == _lib.OMB_EINVAL
    assert lib.omb_plan_hvi_paths_con(None, 1, 2, 1, 0.0, p, 2, o, p) == _lib.OMB_EINVAL
