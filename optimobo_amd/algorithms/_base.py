"""Shared BO-driver plumbing of the drop-in optimisers.

The loop structure, bounds bookkeeping, hypervolume trace, surrogate fitting and result
assembly follow the reference drivers (optimisers.py:144-277, 373-527; emo.py:244-328;
parego.py:148-298).  What changes is the acquisition maximiser: the reference's per-candidate
``differential_evolution`` is replaced by the batched device arg-max
(optimobo_amd.acquisition.AcquisitionEngine.maximise).
"""
import warnings

import numpy as np

from .. import pareto
from .. import util_functions
from .._lib import OMB_ENOTPD, OMB_EUNSUP, OMBError
from ..acquisition import device_engine, engine_for
from ..gp import GPRegression, Matern52, apply_noise_option, check_noise_option, fit_concurrently
from ..parallel import agree_host_rng
from ..result import Constrained_Res, Res


class BODriver:
    # constraints="pof": surrogates in front of the constraint models (n_obj for MultiSurrogateOptimiser, 1 for
    # MonoSurrogateOptimiser); None: the driver does not take the keyword's "pof"
    _pof_objective_models = None
    pof_eps = 1e-5      # added to the constraint models' σ² inside the probability of feasibility (cParEGO's value)
    # batch_strategy values the driver takes: the drivers that ignore batch_size take the default alone
    _batch_strategies = ("believer",)
    thompson_candidates = None   # candidates of a Thompson batch (None: AcquisitionEngine.thompson_batch's default)
    # thompson_sampler="paths": random Fourier features per model and refinement rounds around every nominee
    thompson_features = 1024
    thompson_refine_rounds = 2
    path_gradients = False       # the keyword's default (an instance attribute only where it is True)
    model_front = False          # likewise; _model_front: whether the driver takes model_front=True
    model_front_candidates = 1 << 18
    _model_front = False
    # the keyword's default (instance attributes only under "device"); _device_hypervolume: whether the driver takes it
    hypervolume = "host"
    hypervolume_fallbacks = 0
    _device_hypervolume = True
    model_front_min_feasibility = 0.5    # constraints: the probability of feasibility a member of the model front needs
    # constraints="paths": the width of the sigmoid that stands for the feasibility indicator in the noisy EHVI / EI
    # (0.0: the indicator itself; a Thompson batch always takes the indicator)
    paths_eta = 0.0

    def __init__(self, test_problem, ideal_point=None, max_point=None, mode="reference", n_candidates=1 << 14,
                 refine_rounds=2, seed=None, device=None, polish=True, starts=None, noise=0.0, batch_size=1,
                 constraints=None, batch_strategy="believer", thompson_sampler="joint", log_acquisition=False,
                 acquisition=None, mes_samples=8, mes_candidates=1 << 16, path_gradients=False, model_front=False,
                 model_front_candidates=1 << 18, hypervolume="host"):
        self.test_problem = test_problem
        self.max_point = max_point
        self.ideal_point = ideal_point
        self.n_vars = test_problem.n_var
        self.n_obj = test_problem.n_obj
        self.upper = test_problem.xu
        self.lower = test_problem.xl
        self.is_ideal_known = ideal_point is not None
        self.is_max_known = max_point is not None
        # device-maximiser settings (not in the reference, which uses scipy DE)
        if mode not in ("reference", "textbook"):
            raise ValueError("mode must be 'reference' or 'textbook'")
        self.mode = mode
        self.n_candidates = int(n_candidates)
        self.refine_rounds = int(refine_rounds)
        # several ranks (torch.distributed initialised): one seed and one numpy state for all of them
        self.seed = agree_host_rng(seed)
        self.device = device
        # AcquisitionEngine.maximise's finish (True: the stencil L-BFGS-B; "analytic" / "auto": the batched one on
        # the device gradient) and its number of starts (None: maximise's default)
        self.polish = polish
        self.starts = starts
        # the surrogates' noise variance (not in the reference, which fixes it at 0): 0.0 or a positive float
        # fixes it there, "fit" leaves it free for the hyperparameter search (GPy's own default)
        self.noise = check_noise_option(noise)
        # points proposed per BO iteration (not in the reference, which proposes one).  MultiSurrogateOptimiser and
        # MonoSurrogateOptimiser build a batch greedily with the Kriging believer (AcquisitionEngine.condition);
        # the other drivers accept the keyword and ignore it.  1 is the reference's loop, call for call.
        if isinstance(batch_size, bool) or not isinstance(batch_size, (int, np.integer)) or batch_size < 1:
            raise ValueError(f"batch_size must be an integer >= 1, not {batch_size!r}")
        self.batch_size = int(batch_size)
        # inequality constraints of the problem (not in the reference, whose optimisers.py:22 says "Constraints not
        # supported"): None ignores them, as the reference does; "pof" fits one GP per constraint and weights the
        # acquisition by the probability of feasibility (g <= 0 feasible); "paths" fits the same GPs and reads them
        # through posterior sample paths — under every draw a row or a candidate is feasible when all constraint
        # paths are <= 0 there — which is what the sampled-front acquisitions and Thompson batches can use
        self.constraints = self._check_constraints_option(constraints)
        # how a batch is built (not in the reference): "believer" picks one point after another, conditioning the
        # surrogates on each pick's posterior mean; "thompson" takes q joint posterior draws over one candidate set
        # and lets every draw nominate its best candidate (AcquisitionEngine.thompson_batch)
        self.batch_strategy = self._check_batch_strategy(batch_strategy)
        # how a Thompson batch draws (not in the reference): "joint" draws jointly at the candidates (a covariance and
        # its Cholesky factor, TuRBO's way); "paths" draws posterior sample paths — functions, evaluated at many more
        # candidates and again around every nominee (AcquisitionEngine.sample_paths)
        if thompson_sampler not in ("joint", "paths"):
            raise ValueError(f"thompson_sampler must be 'joint' or 'paths', not {thompson_sampler!r}")
        if thompson_sampler == "paths" and self.batch_strategy != "thompson":
            raise ValueError("thompson_sampler='paths' needs batch_strategy='thompson'")
        self.thompson_sampler = thompson_sampler
        # maximise the logarithm of the acquisition (not in the reference): EI and the exact EHVI are exactly 0.0 in
        # fp64 over most of a late-run box, where their logarithms still rank the candidates and have a slope
        # (AcquisitionEngine.plan_log).  False is the linear path, call for call.
        self.log_acquisition = self._check_log_acquisition(log_acquisition)
        # the acquisition of every pick (not in the reference): None is the driver's own (EHVI / expected decomposition
        # / EI), call for call; "mes" is max-value entropy search — MESMO over MultiSurrogateOptimiser's objectives, MES
        # on MonoSurrogateOptimiser's scalarised surrogate — from ``mes_samples`` posterior sample paths per pick, each
        # minimised over ``mes_candidates`` Sobol' points and the training inputs (AcquisitionEngine.sample_minima);
        # "nehvi" (MultiSurrogateOptimiser) / "nei" (MonoSurrogateOptimiser) are the noisy EHVI / EI: the improvement
        # averaged over ``nehvi_samples`` fronts (best values) drawn from the posterior at the points already evaluated,
        # in place of the improvement over the observed — noisy — front (AcquisitionEngine.sample_fronts)
        self.acquisition = self._check_acquisition(acquisition, mes_samples, mes_candidates)
        # finish what a pick takes from posterior sample paths on the paths' own device gradient (not in the reference):
        # acquisition="mes" polishes every sampled minimum (sample_minima(polish=True)), thompson_sampler="paths" every
        # nominee under its own draw (thompson_batch(polish=True)), acquisition="nehvi" / "nei" finishes the search
        # with maximise(polish="paths").  False is the run without it, call for call.
        if not isinstance(path_gradients, (bool, np.bool_)):
            raise ValueError(f"path_gradients must be True or False, not {path_gradients!r}")
        if path_gradients and self.acquisition is None and self.thompson_sampler != "paths":
            raise ValueError("path_gradients=True needs something drawn from sample paths: acquisition='mes', 'nehvi' "
                             "or 'nei', or thompson_sampler='paths'")
        if self.constraints == "paths":
            if self.acquisition not in ("nehvi", "nei") and self.batch_strategy != "thompson":
                raise ValueError("constraints='paths' reads the constraint models through posterior sample paths: it "
                                 "needs acquisition='nehvi' (MultiSurrogateOptimiser) or 'nei' (MonoSurrogateOptimiser), "
                                 "or batch_strategy='thompson'; the other acquisitions take constraints='pof'")
            if path_gradients:
                raise ValueError("path_gradients=True does not support constraints='paths' (no gradient through the "
                                 "paths' feasibility weight)")
            if self.n_vars > 64:
                raise ValueError(f"constraints='paths' samples posterior paths, which need n_var <= 64 "
                                 f"(n_var={self.n_vars})")
        if path_gradients:      # False stays the class attribute: the instance is the one built without the keyword
            self.path_gradients = True
        # report the model's Pareto set next to the observed one (not in the reference): after its loop ``solve`` fits
        # the surrogates once more on everything evaluated and filters their posterior mean over the evaluated inputs
        # and ``model_front_candidates`` Sobol' points of the box (AcquisitionEngine.predicted_front) — under noise the
        # observed front is made of the luckiest draws.  False fits and draws nothing more: the run without it.
        if not isinstance(model_front, (bool, np.bool_)):
            raise ValueError(f"model_front must be True or False, not {model_front!r}")
        if model_front:
            if not self._model_front:
                raise ValueError(f"{type(self).__name__} does not support model_front=True (MultiSurrogateOptimiser "
                                 "does: its surrogates model the objectives themselves)")
            if isinstance(model_front_candidates, bool) or not isinstance(model_front_candidates, (int, np.integer)) \
                    or model_front_candidates < 1:
                raise ValueError(f"model_front_candidates must be an integer >= 1, not {model_front_candidates!r}")
            self.model_front = True
            self.model_front_candidates = int(model_front_candidates)
        # where the hypervolume trace is computed (not in the reference, which calls pygmo): "host" is
        # ``pareto.hypervolume``, the run without the keyword; "device" the exact sweep of
        # ``AcquisitionEngine.hypervolume`` — the same number to rounding — which falls back to the host function for
        # a front it refuses (more than 1024 rows, or above its work cap) and counts that in
        # ``hypervolume_fallbacks``.  Nothing a proposal is computed from reads it: the run picks the same points.
        if not isinstance(hypervolume, str) or hypervolume not in ("host", "device"):
            raise ValueError(f"hypervolume must be 'host' or 'device', not {hypervolume!r}")
        if hypervolume == "device":
            if not self._device_hypervolume:
                raise ValueError(f"{type(self).__name__} does not support hypervolume='device' (it computes its own "
                                 "trace; the drivers whose trace is BODriver's do)")
            self.hypervolume = "device"
            self.hypervolume_fallbacks = 0   # trace entries that the host function computed after all
        self.thompson_fallbacks = 0   # Thompson iterations that fell back to the believer batch
        self._iteration = 0
        self._mes_picks = 0

    def _check_batch_strategy(self, batch_strategy):
        if batch_strategy not in ("believer", "thompson"):
            raise ValueError(f"batch_strategy must be 'believer' or 'thompson', not {batch_strategy!r}")
        if batch_strategy not in self._batch_strategies:
            raise ValueError(f"{type(self).__name__} ignores batch_size and takes batch_strategy='believer' alone "
                             "(MultiSurrogateOptimiser with an EHVI acquisition and MonoSurrogateOptimiser support "
                             "'thompson')")
        if batch_strategy == "thompson" and self.constraints == "pof":
            raise ValueError("batch_strategy='thompson' does not support constraints='pof' (supported: "
                             "constraints=None; 'believer' batches take constraints='pof')")
        return batch_strategy

    # log_acquisition=True: MonoSurrogateOptimiser (EI) and MultiSurrogateOptimiser in textbook mode (exact EHVI)
    _log_acquisition_modes = None

    def _check_log_acquisition(self, log_acquisition):
        if not isinstance(log_acquisition, (bool, np.bool_)):
            raise ValueError(f"log_acquisition must be True or False, not {log_acquisition!r}")
        if not log_acquisition:
            return False
        modes = self._log_acquisition_modes
        if modes is None:
            raise ValueError(f"{type(self).__name__} does not support log_acquisition=True (MonoSurrogateOptimiser's "
                             "EI and MultiSurrogateOptimiser's exact EHVI in mode='textbook' have a log form)")
        if self.mode not in modes:
            raise ValueError(f"log_acquisition=True needs mode in {modes} on {type(self).__name__} (mode={self.mode!r} "
                             "plans an acquisition without a log form)")
        return True

    # acquisition="mes": MultiSurrogateOptimiser (acquisition_func=None) and MonoSurrogateOptimiser; "nehvi": the
    # former, "nei": the latter
    _acquisitions = ()
    mes_features = 1024          # random Fourier features per model of a pick's sample paths
    nehvi_samples = 16           # sampled fronts (paths per model) of a noisy-EHVI / noisy-EI pick: 1..16, one install
    nehvi_features = 1024        # random Fourier features per model of those paths

    def _check_acquisition(self, acquisition, mes_samples, mes_candidates):
        self.mes_samples, self.mes_candidates = mes_samples, mes_candidates
        if acquisition is None:
            return None
        if not isinstance(acquisition, str) or acquisition not in ("mes", "nehvi", "nei"):
            raise ValueError(f"acquisition must be None or 'mes', 'nehvi' or 'nei', not {acquisition!r}")
        if acquisition not in self._acquisitions:
            raise ValueError(f"{type(self).__name__} does not support acquisition={acquisition!r} ('mes' is "
                             "MultiSurrogateOptimiser's and MonoSurrogateOptimiser's, 'nehvi' the former's alone, "
                             "'nei' the latter's)")
        if acquisition != "mes" and self.constraints == "pof":
            raise ValueError(f"acquisition={acquisition!r} does not support constraints='pof' (the sampled-front plan "
                             "computes no posterior for the constraint models to weight it with)")
        # what the three share: every pick plans from fresh posterior sample paths
        if self.batch_strategy == "thompson":
            raise ValueError(f"acquisition={acquisition!r} does not support batch_strategy='thompson' (a Thompson "
                             "batch maximises no acquisition; 'believer' batches take it)")
        if self.log_acquisition:
            raise ValueError(f"acquisition={acquisition!r} does not support log_acquisition=True (neither max-value "
                             "entropy search nor the mean over sampled fronts has a log form)")
        if self.n_vars > 64:
            raise ValueError(f"acquisition={acquisition!r} samples posterior paths, which need n_var <= 64 "
                             f"(n_var={self.n_vars})")
        if acquisition != "mes":
            return acquisition
        if isinstance(mes_samples, bool) or not isinstance(mes_samples, (int, np.integer)) or not 1 <= mes_samples <= 16:
            raise ValueError(f"mes_samples must be an integer in [1, 16], not {mes_samples!r}")
        if isinstance(mes_candidates, bool) or not isinstance(mes_candidates, (int, np.integer)) or mes_candidates < 1:
            raise ValueError(f"mes_candidates must be an integer >= 1, not {mes_candidates!r}")
        self.mes_samples, self.mes_candidates = int(mes_samples), int(mes_candidates)
        return "mes"

    def _base_seed(self):
        return self.seed if self.seed is not None else np.random.randint(0, 2 ** 31 - 1)

    def _search_seed(self):
        """The seed of the next search or Thompson batch: one per call, so every rank computes the same one."""
        seed = self._base_seed() + 7919 * self._iteration
        self._iteration += 1
        return seed

    def _path_seed(self):
        """The seed of the next pick's sample paths (``_plan_mes`` and ``_plan_nehvi`` share the counter)."""
        base = self._base_seed()
        self._mes_picks += 1
        return base + 15485863 + 7919 * self._mes_picks

    def _plan_nehvi(self, eng, k):
        """The noisy-EHVI (k = 1: noisy-EI) plan of one pick on ``eng`` over its ``k`` models: ``nehvi_samples`` fresh
        sample paths, their fronts at the training inputs, the plan.  Under constraints="paths" the ``n_con`` models
        behind them are sampled too: every path's front is its own feasible one and the plan weights every candidate's
        path by its feasibility under the same draw (``paths_eta``).  ``eng.condition`` drops the paths, so a believer
        batch samples again for every pick, from the conditioned state.  ``pareto.BoxBudgetError`` (n_obj ≥ 4, a
        front past ``exact_max_boxes``) propagates."""
        eng.sample_fronts(self.nehvi_samples, self.max_point if k > 1 else None, self.test_problem.xl,
                          self.test_problem.xu, seed=self._path_seed(), n_features=self.nehvi_features,
                          max_boxes=getattr(self, "exact_max_boxes", 1 << 20),
                          **({"n_con": self.n_con} if self.constraints == "paths" else {}))
        eng.plan_nehvi(**({"eta": self.paths_eta} if self.constraints == "paths" else {}))

    def _plan_mes(self, eng, k):
        """The MES plan of one pick on ``eng`` over its first ``k`` models: fresh sample paths, their minima, the
        plan.  ``eng.condition`` drops the paths, so a believer batch samples again for every pick, from the
        conditioned state."""
        ystar = eng.sample_minima(self.mes_samples, self.test_problem.xl, self.test_problem.xu,
                                  n_candidates=self.mes_candidates, seed=self._path_seed(),
                                  n_features=self.mes_features, **({"polish": True} if self.path_gradients else {}))
        eng.plan_mes(ystar[:k])

    def _check_constraints_option(self, constraints):
        if constraints is None:
            return None
        if not isinstance(constraints, str) or constraints not in ("pof", "paths"):
            raise ValueError(f"constraints must be None or 'pof' (or 'paths', with the sampled-front acquisitions and "
                             f"Thompson batches), not {constraints!r}")
        k = self._pof_objective_models
        if k is None:
            raise ValueError(f"{type(self).__name__} does not support constraints={constraints!r} "
                             "(MultiSurrogateOptimiser and MonoSurrogateOptimiser do)")
        k = self.n_obj if k == "n_obj" else int(k)
        n_ieq = int(getattr(self.test_problem, "n_ieq_constr", 0) or 0)
        if n_ieq == 0:
            raise ValueError(f"constraints={constraints!r} needs a problem with n_ieq_constr > 0")
        if int(getattr(self.test_problem, "n_eq_constr", 0) or 0) > 0:
            raise ValueError(f"constraints={constraints!r} does not handle equality constraints (n_eq_constr > 0)")
        if k + n_ieq > 8:
            raise ValueError(f"constraints={constraints!r}: {k} objective model(s) + {n_ieq} constraints exceed the "
                             "device context's 8 models")
        self.n_con = n_ieq
        return constraints

    # -- constraints="pof"
    def _constraint_values(self, X):
        """G (len(X), n_ieq_constr) of the rows of X through ``problem.evaluate_constraints``.  Without
        constraints="pof" / "paths" nothing is evaluated and G has no columns, so that ``_feasible`` passes every
        row."""
        X = np.atleast_2d(X)
        if self.constraints is None:
            return np.empty((len(X), 0))
        return np.asarray([np.atleast_1d(self.test_problem.evaluate_constraints(x, return_values_of=["G"])) for x in X],
                          dtype=np.float64).reshape(len(X), -1)

    @staticmethod
    def _feasible(G):
        """cParEGO's rule: a row is feasible when every g <= 0."""
        return np.all(np.atleast_2d(G) <= 0, axis=1)

    def _constrained_result(self, ysample, Xsample, gsample, hypervolume_convergence, n_init_samples):
        feas = self._feasible(gsample)
        y_feasible, X_feasible = ysample[feas], Xsample[feas]
        pf_approx = util_functions.calc_pf(y_feasible)
        idx = [i for i, y in enumerate(y_feasible) if any(np.array_equal(y, p) for p in np.atleast_2d(pf_approx))]
        return Constrained_Res(ysample[~feas], y_feasible, Xsample[~feas], X_feasible, pf_approx, X_feasible[idx],
                               ysample, Xsample, hypervolume_convergence, self.n_obj, n_init_samples)

    def _objective_function(self, problem, x):
        return problem.evaluate(x)

    # -- optimisers.py:189-213 (the AttributeError for an unset acquisition_func is the reference's)
    def _update_bounds(self, ysample, scal):
        if not self.is_ideal_known and not self.is_max_known:
            self.max_point = ysample.max(axis=0).astype(float)
            self.ideal_point = ysample.min(axis=0).astype(float)
            self._set_bounds(scal, self.ideal_point, self.max_point)
        elif not self.is_ideal_known:
            self.ideal_point = ysample.min(axis=0).astype(float)
            self._set_bounds(scal, self.ideal_point, self.max_point)
        elif not self.is_max_known:
            self.max_point = ysample.max(axis=0).astype(float)
            self._set_bounds(scal, self.ideal_point, self.max_point)

    def _set_bounds(self, scal, lo, hi):
        if scal is None and self.mode == "textbook":
            return
        scal.set_bounds(lo, hi)       # reference mode: None raises AttributeError, as the reference does

    def _hypervolume(self, ysample):
        if self.hypervolume == "device" and np.size(ysample):
            try:
                hv = device_engine(self.device).hypervolume(np.ascontiguousarray(np.atleast_2d(ysample).T),
                                                            self.max_point)
                return float(hv[0])
            except OMBError as e:
                if e.code != OMB_EUNSUP:
                    raise
                self.hypervolume_fallbacks += 1
        return pareto.hypervolume(ysample, self.max_point)

    def _model(self, X, y):
        model = GPRegression(X, np.reshape(y, (-1, 1)), Matern52(self.n_vars, ARD=True))
        return apply_noise_option(model, self.noise)

    def _fit(self, X, y):
        model = self._model(X, y)
        model.optimize(messages=False, max_f_eval=1000)
        return model

    def _fit_many(self, X, ys):
        """One surrogate per column of ``ys`` on the same inputs, as the reference's per-objective
        loop does (optimisers.py:186, emo.py:297-301); the independent fits run concurrently on the
        GPU (gp.fit_concurrently), each taking the path it takes alone."""
        models = [self._model(X, ys[:, i]) for i in range(ys.shape[1])]
        fit_concurrently(models, device=self.device, messages=False, max_f_eval=1000)
        return models

    def _maximise(self, models, acq_fn, eng=None):
        """acq_fn None: the plan set on the engine (fused chain); else a batched callable.  ``eng``: the engine
        to search on as it stands (a batch's later picks, whose states carry fantasies that loading ``models``
        again would undo); None loads ``models``."""
        if eng is None:
            eng = engine_for(models, self.device)
        polish = self.polish
        if self.path_gradients and acq_fn is None and self.acquisition in ("nehvi", "nei"):
            polish = "paths"
        return eng.maximise(acq_fn, self.test_problem.xl, self.test_problem.xu, n_candidates=self.n_candidates,
                            seed=self._search_seed(), refine_rounds=self.refine_rounds, polish=polish,
                            starts=self.starts)

    def _maximise_plan(self, models, eng):
        """The search of a ``_get_proposed*`` hook once its plan is set.  Under constraints="pof" the plan is first
        weighted by the probability of feasibility of the ``n_con`` models behind it (AcquisitionEngine
        .plan_constraints, after the plan and its ``plan_log``: a log plan keeps its flag, log F is added).
        ``eng`` None — an iteration's first pick — is the reference loop's two-argument ``_maximise`` call.
        constraints="paths": the sampled-front plan carries its constraints itself; a Thompson iteration that fell
        back to the believer batch plans the driver's own acquisition and is weighted as under "pof"."""
        if self.constraints == "pof" or (self.constraints == "paths" and not self._paths_plan()):
            (engine_for(models, self.device) if eng is None else eng).plan_constraints(self.n_con, self.pof_eps)
        return self._maximise(models, None) if eng is None else self._maximise(models, None, eng=eng)

    def _paths_plan(self):
        """constraints="paths" with the sampled-front acquisition, whose plan reads the constraint paths itself."""
        return self.constraints == "paths" and self.acquisition in ("nehvi", "nei")

    def _maximise_feasibility(self, models, eng):
        """constraints="pof" while no row is feasible: the point most likely to be feasible (by log F with
        ``log_acquisition``)."""
        pof = eng.log_feasibility if self.log_acquisition else eng.feasibility
        return self._maximise(models, lambda Xd: pof(Xd, self.n_con, self.pof_eps), eng=eng)[0]

    def _thompson_picks(self, eng, b, PF=None, best=None):
        """``b`` proposals of one iteration by AcquisitionEngine.thompson_batch on ``eng`` as it stands (seeded as
        ``_maximise`` seeds a search, so every rank computes the same batch), or None when that iteration has to
        fall back to the believer batch: the draws' covariance could not be factorised within the jitter ladder
        (OMB_ENOTPD — near-singular fits can exhaust it) or the front needs more boxes than the budget
        (pareto.BoxBudgetError).  A fallback warns and is counted in ``thompson_fallbacks``; any other error of the
        call — a batch larger than the candidate set, say — is the caller's and is raised.  Under
        constraints="paths" the ``n_con`` models behind the objectives are drawn too and every draw nominates its best
        feasible candidate, else its least violating one; ``PF`` is then the feasible front and ``best`` (one
        surrogate) the best feasible value."""
        seed = self._search_seed()
        kw = {}
        if self.constraints == "paths":
            kw = dict(n_con=self.n_con, best=best)
        if self.thompson_sampler == "paths":
            kw.update(sampler="paths", n_features=self.thompson_features, refine_rounds=self.thompson_refine_rounds)
            if self.path_gradients:
                kw["polish"] = True
        try:
            X, _ = eng.thompson_batch(b, self.test_problem.xl, self.test_problem.xu, PF=PF,
                                      max_point=self.max_point if PF is not None else None,
                                      n_candidates=self.thompson_candidates, seed=seed,
                                      max_boxes=getattr(self, "exact_max_boxes", 1 << 20), **kw)
        except (OMBError, pareto.BoxBudgetError) as e:
            if isinstance(e, OMBError) and e.code != OMB_ENOTPD:
                raise
            self.thompson_fallbacks += 1
            warnings.warn(f"Thompson batch unavailable this iteration ({e}); using the Kriging-believer batch",
                          RuntimeWarning, stacklevel=3)
            return None
        return list(X)

    def _result(self, ysample, Xsample, hypervolume_convergence, n_init_samples):
        pf_approx = util_functions.calc_pf(ysample)
        # optimisers.py:269-273 (numpy `in`: any coordinate of the row appears in pf_approx)
        indicies = [i for i, item in enumerate(ysample) if item in pf_approx]
        return Res(pf_approx, Xsample[indicies], ysample, Xsample, hypervolume_convergence, self.n_obj,
                   n_init_samples)

    def _with_model_front(self, res, Xsample, Y):
        """model_front=True: one more fit of the surrogates on all evaluated data — the columns of ``Y``: the
        objectives, then the constraints under constraints="pof" / "paths" — and the model's Pareto set over the
        evaluated inputs and ``model_front_candidates`` Sobol' points (AcquisitionEngine.predicted_front), set on
        ``res`` as ``model_pf_inputs`` (P, n_var), ``model_pf_mean`` and ``model_pf_var`` (P, n_obj)."""
        if not self.model_front:
            return res
        eng = engine_for(self._fit_many(Xsample, Y), self.device)
        front = eng.predicted_front(self.test_problem.xl, self.test_problem.xu, n_candidates=self.model_front_candidates,
                                    seed=self._search_seed(), n_con=Y.shape[1] - self.n_obj,
                                    min_feasibility=self.model_front_min_feasibility, include=Xsample)
        res.model_pf_inputs, res.model_pf_mean, res.model_pf_var = front["X"], front["mean"], front["var"]
        return res

    def _initial_samples(self, n_init_samples):
        ranges = list(zip(self.test_problem.xl, self.test_problem.xu))
        Xsample = util_functions.generate_latin_hypercube_samples(n_init_samples, ranges)
        ysample = np.asarray([self._objective_function(self.test_problem, x) for x in Xsample])
        return Xsample, ysample
