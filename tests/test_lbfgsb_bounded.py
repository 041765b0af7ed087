"""CPU: optimobo_amd.gp._LbfgsbRun with bounds (nbd = 2) takes bitwise the path of
scipy.optimize.minimize(method="L-BFGS-B", bounds=…) — same optimum and evaluation count — on problems whose
optimum has active bounds, and runs advanced in lockstep (AcquisitionEngine.polish_batch's schedule: one
evaluation round for all runs still active) end where the same runs end one after another."""
import numpy as np
import pytest
from scipy import optimize

from optimobo_amd.gp import _LbfgsbRun


def _quartic(x):
    return float(np.sum((x - 1.5) ** 4) + np.sum(np.cos(x))), 4 * (x - 1.5) ** 3 - np.sin(x)


def _rosen(x):
    return float(optimize.rosen(x)), optimize.rosen_der(x)


# (function, x0, lower, upper): the unconstrained optima (≈ 2.2 per coordinate; (1, 1, 1, 1)) lie outside the boxes
PROBLEMS = [
    (_quartic, np.array([0.3, -1.0, 2.0]), np.array([-1.0, -1.0, 0.0]), np.array([1.0, 3.0, 1.2])),
    (_rosen, np.array([-1.2, 1.0, 0.4, 2.5]), np.array([-2.0, -2.0, -2.0, 1.5]), np.array([0.5, 2.0, 2.0, 3.0])),
]


def _drive(run, fun):
    while True:
        x = run.advance()
        if x is None:
            return run
        run.supply(x, *fun(x))


@pytest.mark.parametrize("fun,x0,lo,hi", PROBLEMS)
@pytest.mark.parametrize("maxiter", [100, 3])
def test_bounded_run_equals_scipy(fun, x0, lo, hi, maxiter):
    ref = optimize.minimize(fun, x0, jac=True, method="L-BFGS-B", bounds=list(zip(lo, hi)),
                            options={"maxiter": maxiter})
    xc = np.clip(x0, lo, hi)
    r = _drive(_LbfgsbRun(xc, *fun(xc), 15000, maxiter, bounds=(lo, hi)), fun)
    assert np.array_equal(ref.x, r.x)
    assert ref.nfev == r.nfev and ref.nit == r.nit and ref.fun == r.f
    assert np.all(r.x >= lo) and np.all(r.x <= hi)
    if maxiter == 100:
        assert np.any((r.x == lo) | (r.x == hi)), "the optimum should have an active bound"


def test_start_outside_the_box_is_clipped_like_scipy():
    fun, _, lo, hi = PROBLEMS[0]
    x0 = np.array([5.0, -4.0, 0.5])
    ref = optimize.minimize(fun, x0, jac=True, method="L-BFGS-B", bounds=list(zip(lo, hi)))
    xc = np.clip(x0, lo, hi)
    r = _drive(_LbfgsbRun(x0, *fun(xc), 15000, 15000, bounds=(lo, hi)), fun)
    assert np.array_equal(ref.x, r.x) and ref.nfev == r.nfev


def test_three_runs_in_lockstep_equal_the_runs_alone():
    fun, _, lo, hi = PROBLEMS[0]
    starts = [np.array([0.3, -1.0, 1.0]), np.array([-0.9, 2.5, 0.1]), np.array([1.0, 0.0, 1.2])]
    alone = [_drive(_LbfgsbRun(x, *fun(x), 15000, 100, bounds=(lo, hi)), fun) for x in starts]
    runs = {s: _LbfgsbRun(x, *fun(x), 15000, 100, bounds=(lo, hi)) for s, x in enumerate(starts)}
    done, rounds = {}, 0
    while runs:
        ask = {}
        for s in sorted(runs):
            x = runs[s].advance()
            if x is None:
                done[s] = runs.pop(s)
            else:
                ask[s] = x
        rounds += 1
        for s, x in ask.items():           # one round of evaluations for every run still active
            runs[s].supply(x, *fun(x))
    assert len({a.nfev for a in alone}) > 1, "the runs should stop at different rounds"
    for s, a in enumerate(alone):
        assert np.array_equal(a.x, done[s].x) and a.nfev == done[s].nfev and a.nit == done[s].nit


def test_unbounded_run_is_unchanged():
    """bounds=None leaves nbd = 0 and the start as given."""
    r = _LbfgsbRun(np.array([5.0, -7.0]), 0.0, np.zeros(2), 10, 10)
    assert np.all(r.nbd == 0) and np.array_equal(r.x, [5.0, -7.0])
