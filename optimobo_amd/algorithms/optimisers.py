"""Drop-in ``optimobo.algorithms.optimisers`` (optimisers.py:18-527).

``MultiSurrogateOptimiser(problem, ideal, max).solve(budget, n_init_samples,
sample_exponent, acquisition_func)`` and ``MonoSurrogateOptimiser(...).solve(aggregation_func,
budget, n_init_samples)`` keep the reference signatures and return ``Res``.  Extra keyword
arguments select the device maximiser: ``mode`` ("reference" = bug-compatible acquisition
values, "textbook" = exact EHVI for every ``n_obj`` from 2 to 8), ``n_candidates`` (Sobol batch per
iteration), ``refine_rounds``, ``seed`` and ``device``.

The exact EHVI at ``n_obj`` ≥ 4 sums over a box decomposition of the non-dominated region whose size grows
steeply with the front (pareto.box_decomposition).  ``MultiSurrogateOptimiser.exact_max_boxes`` bounds it: an
iteration whose front needs more boxes, or a grid larger than the kernel holds, uses the reference's
Monte-Carlo estimate instead and says so in one ``RuntimeWarning`` per optimiser.
"""
import warnings

import numpy as np

from .. import pareto
from ..refdirs import get_reference_directions
from .._lib import OMB_EUNSUP, OMBError
from ..acquisition import engine_for
from ._base import BODriver


class MultiSurrogateOptimiser(BODriver):
    """One GP per objective; EHVI (2-D, or k-D for n_obj ≥ 3) or expected decomposition as the acquisition.

    mode "textbook": the exact EHVI for 2 ≤ n_obj ≤ 8; at n_obj ≥ 4 while the front's box decomposition
    stays within ``exact_max_boxes`` (else the Monte-Carlo estimate, with one RuntimeWarning).
    """

    exact_max_boxes = 1 << 17       # boxes of one iteration's exact EHVI at n_obj ≥ 4
    _pof_objective_models = "n_obj"
    _batch_strategies = ("believer", "thompson")
    _log_acquisition_modes = ("textbook",)     # the exact EHVI over boxes; reference mode plans EHVI-2D / Monte-Carlo
    _acquisitions = ("mes", "nehvi")           # MESMO / the noisy EHVI in place of EHVI, in either mode
    _model_front = True                        # model_front=True: the posterior mean's Pareto set on the result

    def _get_cached_samples(self, dimensions, sample_exponent):
        """optimisers.py:121-141 — scrambled Sobol mapped through the normal ppf."""
        return pareto.cached_samples(dimensions, sample_exponent, seed=self.seed)

    def _get_proposed_EHVI(self, function, models, ideal_point, max_point, pf, cache, eng=None):
        """optimisers.py:91-119 on the device: returns (x, −EHVI(x)).  ``eng``: as in ``_maximise``."""
        self._plan_EHVI(engine_for(models, self.device) if eng is None else eng, function, max_point, pf, cache)
        x, v = self._maximise_plan(models, eng)
        return x, -v

    def _plan_EHVI(self, eng, function, max_point, pf, cache):
        """The EHVI plan of one proposal on ``eng``: 2-D, Monte-Carlo or exact, as mode and n_obj ask."""
        if self.acquisition == "mes":
            self._plan_mes(eng, self.n_obj)             # acquisition="mes": MESMO over the objectives' sampled minima
            return
        if self.acquisition == "nehvi":
            self._plan_nehvi(eng, self.n_obj)           # the noisy EHVI: fronts sampled at the training inputs, not pf
            return
        mc = function == "EHVI_3D" or self.n_obj >= 3          # optimisers.py:245-248: EHVI_3D for n_obj != 2
        if self.log_acquisition and self.n_obj <= 3:
            # log_acquisition (textbook mode): the box form at k = 2 as well — EHVI-2D's stripes have no log kernel
            eng.plan_ehvi_exact(max_point, pf)
            eng.plan_log()
        elif mc and self.mode == "textbook" and self.n_obj <= 3:
            eng.plan_ehvi_exact(max_point, pf)          # exact EHVI in place of the MC estimate (k = 2, 3)
        elif mc and self.mode == "textbook":
            # exact for 4 ≤ k ≤ 8 while the box budget allows; an iteration on the Monte-Carlo fallback stays linear
            if self._plan_exact_kd(eng, max_point, pf, cache) and self.log_acquisition:
                eng.plan_log()
        elif mc:
            eng.plan_ehvi3d(max_point, pf, cache)       # the reference's Monte-Carlo form, any k ≥ 3
        else:
            eng.plan_ehvi(max_point, pf, cache, mode=self.mode)

    def _plan_exact_kd(self, eng, max_point, pf, cache):
        """Plans the exact EHVI at n_obj ≥ 4; when the box budget or the kernel's grid limit rules it out, the
        Monte-Carlo plan stands in, after one RuntimeWarning per optimiser.  True when the exact plan is set."""
        try:
            eng.plan_ehvi_exact(max_point, pf, max_boxes=self.exact_max_boxes)
            return True
        except ValueError as e:                          # box_decomposition: over the box budget
            reason = str(e)
        except OMBError as e:                            # omb_plan_ehvi_boxes_k: grid or box count past the kernel's
            if e.code != OMB_EUNSUP:
                raise
            reason = str(e)
        if not getattr(self, "_warned_exact_fallback", False):
            self._warned_exact_fallback = True
            warnings.warn(f"exact EHVI unavailable at n_obj={self.n_obj} ({reason}); using the Monte-Carlo "
                          "estimate of the reference", RuntimeWarning, stacklevel=3)
        eng.plan_ehvi3d(max_point, pf, cache)
        return False

    def _get_proposed_scalarisation(self, function, models, min_val, scalar_func, ref_dir, cache, eng=None):
        """optimisers.py:62-88 on the device: returns (x, −value, ref_dir).  ``eng``: as in ``_maximise``."""
        planned = engine_for(models, self.device) if eng is None else eng
        planned.plan_expected_decomposition(ref_dir, scalar_func, min_val, cache)
        x, v = self._maximise_plan(models, eng)
        return x, -v, ref_dir

    def solve(self, budget=100, n_init_samples=5, sample_exponent=5, acquisition_func=None):
        """``budget`` true evaluations in ⌈budget/q⌉ iterations of q = ``batch_size`` proposals (the last one
        truncated; 1 is the reference's loop, call for call), one ``hypervolume_convergence`` entry per iteration.

        One iteration: one fit, then the batch.  The Kriging believer builds it greedily: every pick draws a fresh
        reference direction, plans the acquisition from the samples plus the fantasies so far (their front, or the
        scalarisation's minimum) and maximises it through ``_get_proposed_EHVI`` / ``_get_proposed_scalarisation``;
        before the next pick the resident GPs are conditioned on the point with their own posterior mean as its
        value (AcquisitionEngine.condition: μ stays, σ² collapses around the pick, so the next arg-max moves on),
        and that pick searches the engine as it stands (``eng=``).  The picks are then evaluated for real; the next
        fit uploads the fitted states again, so no fantasy outlives its batch.

        ``batch_strategy="thompson"`` (EHVI acquisitions): one AcquisitionEngine.thompson_batch over the true
        samples' front proposes all the iteration's points at once (``_thompson_picks``) and draws no reference
        direction; an iteration it cannot serve is built by the believer instead.

        ``constraints="pof"`` returns a ``Constrained_Res``: one more GP per inequality constraint on the same
        inputs, every pick's acquisition weighted by their probability of feasibility (``_maximise_plan``), and the
        believer conditions them as well.  A row is feasible when every g ≤ 0; the front, the scalarisation's minimum
        and the hypervolume trace (0.0 while nothing is feasible) use feasible rows only — fantasies count as
        feasible by the constraint models' means.  While no row is feasible the pick maximises the probability of
        feasibility alone (``_maximise_feasibility``).  Without the keyword G has no columns: every row is feasible.

        ``log_acquisition=True`` (textbook mode, ``acquisition_func`` None): every pick maximises the logarithm of
        the exact EHVI (plus log F under ``constraints="pof"``; log F alone while no row is feasible).

        ``model_front=True``: after the loop the surrogates (the constraint models too) are fitted once more on
        everything evaluated and the result carries the model's Pareto set — ``model_pf_inputs``, ``model_pf_mean``,
        ``model_pf_var`` (``_with_model_front``); the samples are the run's without it, bit for bit."""
        if self.acquisition is not None and acquisition_func is not None:
            raise ValueError(f"acquisition={self.acquisition!r} takes the place of the EHVI (acquisition_func=None), "
                             "not of a scalarised expected decomposition")
        if self.log_acquisition and acquisition_func is not None:
            raise ValueError("log_acquisition=True takes the exact EHVI (acquisition_func=None): the expected "
                             "decomposition has no log form")
        if self.batch_strategy == "thompson" and acquisition_func is not None:
            raise ValueError("batch_strategy='thompson' scores draws by hypervolume improvement: it supports the EHVI "
                             "acquisitions (acquisition_func=None), not a scalarised expected decomposition")
        problem = self.test_problem
        pof, k = self.constraints == "pof", problem.n_obj
        con = self.constraints is not None      # "pof" or "paths": constraint models, feasible rows, Constrained_Res
        cached_samples = self._get_cached_samples(self.n_obj, sample_exponent)
        if pof and acquisition_func is None and k == 2 and self.mode == "reference" and \
                pareto.cache_stats(np.asarray(cached_samples, np.float64))[1] <= 0:
            # with s01 <= 0 the reference-mode acquisition is <= 0 everywhere, and a weight in
            # [0, 1] on a non-positive value favours the infeasible points
            raise ValueError("constraints='pof' with reference-mode 2-D EHVI needs a sample cache whose s01 > 0 "
                             "(this seed / sample_exponent gives s01 <= 0); use mode='textbook'")
        Xsample, ysample = self._initial_samples(n_init_samples)
        gsample = self._constraint_values(Xsample)
        ref_dirs = get_reference_directions("das-dennis", self.n_obj, n_partitions=100)
        hypervolume_convergence = []
        done = 0
        while done < budget:
            b = min(self.batch_size, budget - done)
            self._update_bounds(ysample, acquisition_func)
            hypervolume_convergence.append(self._hypervolume(ysample[self._feasible(gsample)]))
            models = self._fit_many(Xsample, np.hstack((ysample[:, :k], gsample)))
            eng = engine_for(models, self.device)
            yfant, gfant, picks = ysample[:, :k], gsample, None
            if self.batch_strategy == "thompson" and self.constraints == "paths":
                # the draws' score is the improvement over the feasible front (empty: over the reference point's box)
                picks = self._thompson_picks(eng, b, pareto.calc_pf(yfant[self._feasible(gfant)]))
            elif self.batch_strategy == "thompson":
                picks = self._thompson_picks(eng, b, pareto.calc_pf(yfant))
            if picks is None:              # the believer batch (also a Thompson iteration's fallback)
                picks = []
                for p in range(b):
                    ref_dir = np.asarray(ref_dirs[np.random.randint(0, len(ref_dirs))])
                    yfeas = yfant[self._feasible(gfant)]
                    on = dict(eng=eng) if p else {}        # conditioned since the fit: search it as it stands
                    if len(yfeas) == 0 and not self._paths_plan():         # "paths": every draw has its own front
                        x = self._maximise_feasibility(models, eng)
                    elif acquisition_func is None:
                        x, _ = self._get_proposed_EHVI("EHVI" if k == 2 else "EHVI_3D", models, self.ideal_point,
                                                       self.max_point, pareto.calc_pf(yfeas), cached_samples, **on)
                    else:
                        min_scalar = np.min([acquisition_func(y, ref_dir) for y in yfeas])
                        x, _, _ = self._get_proposed_scalarisation("expected_decomposition", models, min_scalar,
                                                                   acquisition_func, ref_dir, cached_samples, **on)
                    picks.append(x)
                    if p + 1 < b:
                        m = eng.condition(x[None, :])
                        yfant, gfant = np.vstack((yfant, m[:, :k])), np.vstack((gfant, m[:, k:]))
            for x in picks:
                ysample = np.vstack((ysample, self._objective_function(problem, x)))
                Xsample = np.vstack((Xsample, x))
            gsample = np.vstack((gsample, self._constraint_values(picks)))
            done += b
        if con:
            res = self._constrained_result(ysample, Xsample, gsample, hypervolume_convergence, n_init_samples)
        else:
            res = self._result(ysample, Xsample, hypervolume_convergence, n_init_samples)
        return self._with_model_front(res, Xsample, np.hstack((ysample[:, :k], gsample)))


class MonoSurrogateOptimiser(BODriver):
    """One GP on scalarised objectives; EI as the acquisition (optimisers.py:283-527)."""

    _pof_objective_models = 1
    _batch_strategies = ("believer", "thompson")
    _log_acquisition_modes = ("reference", "textbook")     # EI either way
    _acquisitions = ("mes", "nei")                         # MES / the noisy EI on the scalarised surrogate, in place of EI

    def _plan_ei(self, eng, best):
        """EI against ``best`` on ``eng``; its logarithm with ``log_acquisition``.  acquisition="mes": max-value
        entropy search on the surrogate instead (``best`` is not used: the sampled minima take its place)."""
        if self.acquisition == "mes":
            self._plan_mes(eng, 1)
            return
        if self.acquisition == "nei":
            self._plan_nehvi(eng, 1)                   # the noisy EI: ``best`` is not used, every path brings its own
            return
        eng.plan_ei(best, 0.0)
        if self.log_acquisition:
            eng.plan_log()

    def _expected_improvement(self, X, model, opt_value, kappa=0.01):
        """optimisers.py:325-344 (σ = sqrt(σ²)); X (d,) → (1,), X (N, d) → (N,)."""
        Xb = np.atleast_2d(np.asarray(X, np.float64))
        out = engine_for([model], self.device).ei(Xb, opt_value, 0.0).cpu().numpy()
        return out[:1] if np.ndim(X) == 1 else out

    def _get_proposed(self, function, models, current_best, eng=None):
        """``models``: the surrogate, or under constraints="pof" the list with the constraint models behind it.
        ``eng``: as in ``_maximise``."""
        models = models if isinstance(models, list) else [models]
        self._plan_ei(engine_for(models, self.device) if eng is None else eng, current_best)
        x, v = self._maximise_plan(models, eng)
        return x, -v

    def _normalize_data(self, data):
        return (data - np.min(data)) / (np.max(data) - np.min(data))

    def solve(self, aggregation_func, budget=100, n_init_samples=5):
        """MultiSurrogateOptimiser.solve's loop on the single surrogate of the aggregated values.  Every believer
        pick's ``current_best`` is the minimum over the true and the fantasised aggregated values, and goes through
        ``_get_proposed``; a reference direction is drawn after each evaluation, to aggregate it.
        ``batch_strategy="thompson"``: every draw nominates the candidate with its smallest drawn value.
        ``constraints="pof"``: ``current_best`` over the feasible rows only, and the surrogate is fitted together
        with the constraint models (``_fit_many``; without the keyword it is ``_fit``'s one model, as before)."""
        problem = self.test_problem
        pof = self.constraints is not None      # "pof" or "paths": constraint models, feasible rows, Constrained_Res
        weights = np.asarray([1 / problem.n_obj] * problem.n_obj)
        Xsample, ysample = self._initial_samples(n_init_samples)
        gsample = self._constraint_values(Xsample)
        self._update_bounds(ysample, aggregation_func)
        aggregated_samples = np.asarray([aggregation_func(i, weights) for i in ysample]).flatten()
        ref_dirs = get_reference_directions("das-dennis", problem.n_obj, n_partitions=100)
        hypervolume_convergence = []
        done = 0
        while done < budget:
            b = min(self.batch_size, budget - done)
            self._update_bounds(ysample, aggregation_func)
            hypervolume_convergence.append(self._hypervolume(ysample[self._feasible(gsample)]))
            if pof:
                models = self._fit_many(Xsample, np.column_stack((aggregated_samples, gsample)))
            else:
                models = [self._fit(Xsample, aggregated_samples)]
            eng = engine_for(models, self.device)
            fant, gfant, picks = aggregated_samples, gsample, None
            if self.batch_strategy == "thompson" and self.constraints == "paths":
                ffeas = fant[self._feasible(gfant)]     # nothing feasible yet: any feasible candidate beats the worst
                picks = self._thompson_picks(eng, b, best=float(ffeas.min() if len(ffeas) else fant.max()))
            elif self.batch_strategy == "thompson":
                picks = self._thompson_picks(eng, b)
            if picks is None:              # the believer batch (also a Thompson iteration's fallback)
                picks = []
                for p in range(b):
                    ffeas = fant[self._feasible(gfant)]
                    if len(ffeas) == 0 and not self._paths_plan():         # "paths": every draw has its own best
                        x = self._maximise_feasibility(models, eng)
                    else:                  # eng: conditioned since the fit, so picks 2..b search it as it stands
                        x, _ = self._get_proposed(self._expected_improvement, models if pof else models[0],
                                                  ffeas[np.argmin(ffeas)] if len(ffeas) else None,
                                                  **(dict(eng=eng) if p else {}))
                    picks.append(x)
                    if p + 1 < b:
                        m = eng.condition(x[None, :])
                        fant, gfant = np.append(fant, m[0, 0]), np.vstack((gfant, m[:, 1:]))
            for x in picks:
                next_y = self._objective_function(problem, x)
                ysample = np.vstack((ysample, next_y))
                ref_dir = ref_dirs[np.random.randint(0, len(ref_dirs))]
                aggregated_samples = np.append(aggregated_samples, aggregation_func(next_y, ref_dir))
                Xsample = np.vstack((Xsample, x))
            gsample = np.vstack((gsample, self._constraint_values(picks)))
            done += b
        if pof:
            return self._constrained_result(ysample, Xsample, gsample, hypervolume_convergence, n_init_samples)
        return self._result(ysample, Xsample, hypervolume_convergence, n_init_samples)
