"""CPU: the hypervolume-improvement box sum against the hypervolume difference, and the drivers'
``batch_strategy`` keyword — validation, refusals and the fallback of a Thompson iteration to the believer batch."""
import warnings

import numpy as np
import pytest

from _hvi_fixture import CASES, fixture, hvi_numpy

from optimobo_amd import pareto
from optimobo_amd._lib import OMB_EHIP, OMB_ENOTPD, OMBError

BOXES = {(2, 1, 0): 2, (2, 9, 1): 10, (3, 12, 2): 56, (4, 20, 3): 908, (5, 12, 4): 780, (8, 6, 5): 1434}


@pytest.mark.parametrize("case", CASES)
def test_box_sum_is_the_hypervolume_difference(case):
    """Σ_b Π_j (hi_bj − max(y_j, lo_bj))⁺ = HV(F ∪ {y}) − HV(F) on the six fixtures.

    The box sum's own error is bounded by (B + 3k)·2^-52 relative; pareto.hypervolume's rounding has no bound on
    record, so the assertion is 100× the largest deviation measured on the CPU, 8.9e-16 absolute (at values up to
    3.7), taken relative to HV(F ∪ {y})."""
    f = fixture(*case)
    assert len(f["boxes"]) == BOXES[case]
    ref = f["ref"]
    assert (ref > 0).mean() >= 0.5
    assert ref[0] == 0.0 and ref[1] == 0.0 and ref[2] == 0.0 and ref[3] > 0.0
    if case[1] > 1:       # with a one-point front, F.min(0) − 0.1 is that point − 0.1, and a noisy copy can beat it
        assert ref[3] == ref.max()
    hv_f = pareto.hypervolume(f["F"], f["r"])
    worst = 0.0
    for y, h in zip(f["Y"], ref):
        hv_y = pareto.hypervolume(np.vstack((f["F"], y)), f["r"])
        worst = max(worst, abs(h - (hv_y - hv_f)))
        assert abs(h - (hv_y - hv_f)) <= 100 * 8.9e-16 * hv_y, (y, h, hv_y - hv_f)
    print(f"case {case}: B={len(f['boxes'])} share>0={(ref > 0).mean():.2f} max={ref.max():.3g} "
          f"worst |box sum − ΔHV| = {worst:.3g}")


def test_hvi_numpy_chunking_is_exact_enough():
    f = fixture(4, 20, 3)
    np.testing.assert_allclose(hvi_numpy(f["Y"], f["coords"], f["boxes"], chunk=37), f["ref"], rtol=1e-13, atol=0)


# ------------------------------------------------------------------------------------------ the drivers' keyword
class _Problem:
    n_var, n_obj = 2, 2
    xl, xu = np.zeros(2), np.ones(2)
    n_ieq_constr = 0

    def evaluate(self, x):
        return np.array([x[0], 1.0 - x[0] + x[1]])


class _Constrained(_Problem):
    n_ieq_constr = 1


def test_batch_strategy_values():
    from optimobo_amd.algorithms.optimisers import MonoSurrogateOptimiser, MultiSurrogateOptimiser
    for cls in (MultiSurrogateOptimiser, MonoSurrogateOptimiser):
        assert cls(_Problem(), [0, 0], [1, 2], seed=1).batch_strategy == "believer"
        assert cls(_Problem(), [0, 0], [1, 2], seed=1, batch_size=3, batch_strategy="thompson").batch_strategy == \
            "thompson"
        for bad in ("Thompson", "greedy", None, 1, ""):
            with pytest.raises(ValueError, match="batch_strategy"):
                cls(_Problem(), [0, 0], [1, 2], seed=1, batch_strategy=bad)


def test_thompson_refused_with_pof_constraints():
    from optimobo_amd.algorithms.optimisers import MonoSurrogateOptimiser, MultiSurrogateOptimiser
    for cls in (MultiSurrogateOptimiser, MonoSurrogateOptimiser):
        with pytest.raises(ValueError, match="constraints"):
            cls(_Constrained(), [0, 0], [1, 2], seed=1, constraints="pof", batch_strategy="thompson")
        assert cls(_Constrained(), [0, 0], [1, 2], seed=1, constraints="pof").batch_strategy == "believer"


def test_thompson_refused_by_the_drivers_that_ignore_batch_size():
    from optimobo_amd.algorithms.cparego import ParEGO_C2
    from optimobo_amd.algorithms.emo import EMO
    from optimobo_amd.algorithms.keep import KEEP
    from optimobo_amd.algorithms.parego import ParEGO
    for cls in (EMO, ParEGO, KEEP, ParEGO_C2):
        with pytest.raises(ValueError, match="believer"):
            cls(_Problem(), [0, 0], [1, 2], seed=1, batch_strategy="thompson")
        assert cls(_Problem(), [0, 0], [1, 2], seed=1, batch_size=2).batch_strategy == "believer"


def test_thompson_refused_for_a_scalarised_multi_surrogate_run():
    """The acquisition is only known at solve(): the refusal comes there, before anything is evaluated."""
    from optimobo_amd.algorithms.optimisers import MultiSurrogateOptimiser
    from optimobo_amd.scalarisations import Tchebicheff
    opt = MultiSurrogateOptimiser(_Problem(), [0, 0], [1, 2], seed=1, batch_size=2, batch_strategy="thompson")
    with pytest.raises(ValueError, match="EHVI"):
        opt.solve(budget=2, n_init_samples=4, acquisition_func=Tchebicheff([0, 0], [1, 2]))


class _Engine:
    def __init__(self, exc=None):
        self.exc, self.calls = exc, []

    def thompson_batch(self, q, lower, upper, **kw):
        self.calls.append(dict(q=q, **kw))
        if self.exc is not None:
            raise self.exc
        return np.full((q, 2), 0.25), dict(indices=np.arange(q), zero_draws=0)


def test_thompson_picks_fall_back_on_a_failed_factorisation_or_box_budget():
    from optimobo_amd.algorithms.optimisers import MultiSurrogateOptimiser
    opt = MultiSurrogateOptimiser(_Problem(), [0, 0], [1, 2], seed=5, batch_size=3, batch_strategy="thompson")
    pf = np.array([[0.2, 0.8], [0.7, 0.3]])
    ok = _Engine()
    picks = opt._thompson_picks(ok, 3, pf)
    assert len(picks) == 3 and opt.thompson_fallbacks == 0
    assert ok.calls[0]["seed"] == 5 and ok.calls[0]["q"] == 3
    for n, exc in enumerate((OMBError(OMB_ENOTPD, "not positive definite"),
                             pareto.BoxBudgetError("more than 131072 boxes")), 1):
        eng = _Engine(exc)
        with pytest.warns(RuntimeWarning, match="believer"):
            assert opt._thompson_picks(eng, 3, pf) is None
        assert opt.thompson_fallbacks == n
        assert eng.calls[0]["seed"] == 5 + 7919 * n          # seeded as _maximise seeds a search
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with pytest.raises(OMBError):                          # any other device error is not a fallback
            opt._thompson_picks(_Engine(OMBError(OMB_EHIP, "hip")), 3, pf)
        with pytest.raises(ValueError, match="outside"):       # nor is an argument error: it reaches the caller
            opt._thompson_picks(_Engine(ValueError("thompson_batch: q=300 outside [1, 200] candidates")), 3, pf)
    assert opt.thompson_fallbacks == 2


def test_box_budget_error_is_the_value_error_it_was():
    f = fixture(4, 20, 3)
    with pytest.raises(ValueError, match="max_boxes") as e:
        pareto.box_decomposition(f["F"], f["r"], max_boxes=100)
    assert isinstance(e.value, pareto.BoxBudgetError)
