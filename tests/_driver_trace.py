"""Call traces of MultiSurrogateOptimiser.solve / MonoSurrogateOptimiser.solve against a fake engine, without a device.

``run(name)`` points ``engine_for`` at a recording stand-in for AcquisitionEngine, replaces the instance's ``_fit`` and
``_fit_many`` with recorders that return opaque tokens, seeds ``np.random`` and runs ``solve``.  The trace is the
ordered list of what the driver asked of the fits and of the engine — every ``plan_*`` / ``sample_*`` call with its
arguments, ``maximise`` (whether ``acq_fn`` is None, and every keyword), ``condition``, ``thompson_batch``,
``feasibility`` / ``log_feasibility`` by name — closed by one record of the run's end state.  The fake answers from a
generator seeded by the call's own arguments, so a trace depends on the driver alone.

Loading the model list that is already resident, with no ``condition`` since, uploads nothing on the real engine
(AcquisitionEngine.load_models); such loads are left out of the trace, every other load is in it.

``python tests/_driver_trace.py`` records every configuration twice, requires the two to agree and the fixture's
conditions to hold (``check_fixture``), and writes tests/golden/driver_traces.json.  The committed file was written
that way while each driver still had three copies of its loop (plain, batched and constrained);
tests/test_driver_trace_host.py replays it.
"""
import json
import os
import sys
import warnings
import zlib

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
FIXTURE = os.path.join(REPO, "tests", "golden", "driver_traces.json")

BUDGET, N_INIT, SAMPLE_EXPONENT = 5, 6, 3
IDEAL, MAX_POINT = [0, 0], [700, 12]


def _problem(constrained):
    from optimobo_amd.problem import ElementwiseProblem

    class MyProblem(ElementwiseProblem):        # the 2-objective problem of tests/test_gpu_append.py
        def __init__(self):
            super().__init__(n_var=2, n_obj=2, n_ieq_constr=int(constrained), xl=np.array([-2, -2]),
                             xu=np.array([2, 2]))

        def _evaluate(self, x, out, *args, **kwargs):
            out["F"] = [100 * (x[0] ** 2 + x[1] ** 2), (x[0] - 1) ** 2 + x[1] ** 2]

        def _evaluate_constraints(self, x, out, *args, **kwargs):
            out["G"] = [2.0 - x[0] - x[1]]      # feasible: the corner x0 + x1 >= 2, an eighth of the box
    return MyProblem()


# name -> (driver, problem constrained, numpy seed, constructor keywords, Tchebicheff as the scalarisation)
# Multi takes the scalarisation as solve's acquisition_func (None: the EHVI); Mono always aggregates with it.
def _configs():
    pof = dict(constraints="pof", mode="textbook")
    th = dict(batch_strategy="thompson")
    return {
        "multi_ehvi_reference": ("multi", False, 41, dict(seed=3), False),
        "multi_textbook_log": ("multi", False, 41, dict(seed=3, mode="textbook", log_acquisition=True), False),
        "multi_tchebicheff": ("multi", False, 41, dict(seed=3), True),
        "multi_mes": ("multi", False, 41, dict(seed=3, acquisition="mes"), False),
        "multi_nehvi": ("multi", False, 41, dict(seed=3, acquisition="nehvi"), False),
        "multi_q3_believer": ("multi", False, 41, dict(seed=3, batch_size=3), False),
        "multi_q3_thompson": ("multi", False, 41, dict(seed=3, batch_size=3, **th), False),
        "multi_q2_thompson_paths": ("multi", False, 41, dict(seed=3, batch_size=2, thompson_sampler="paths", **th), False),
        "multi_q3_thompson_fallback": ("multi", False, 41, dict(seed=3, batch_size=3, **th), False),
        "multi_pof_textbook_q1": ("multi", True, 42, dict(seed=3, batch_size=1, **pof), False),
        "multi_pof_tchebicheff_q2": ("multi", True, 45, dict(seed=3, batch_size=2, **pof), True),
        "multi_pof_textbook_log_q2": ("multi", True, 45, dict(seed=3, batch_size=2, log_acquisition=True, **pof), False),
        "mono_ei": ("mono", False, 43, dict(seed=3), True),
        "mono_nei": ("mono", False, 43, dict(seed=3, acquisition="nei"), True),
        "mono_q3_believer": ("mono", False, 43, dict(seed=3, batch_size=3), True),
        "mono_q3_thompson": ("mono", False, 43, dict(seed=3, batch_size=3, **th), True),
        "mono_pof_q2": ("mono", True, 45, dict(seed=3, batch_size=2, **pof), True),
        "mono_pof_log_q2": ("mono", True, 45, dict(seed=3, batch_size=2, log_acquisition=True, **pof), True),
        # seed=None: every search, Thompson batch and sampled-path plan draws its seed from np.random, in call order
        "mono_ei_unseeded": ("mono", False, 43, dict(seed=None), True),
        "mono_pof_q2_unseeded": ("mono", True, 41, dict(seed=None, batch_size=2, **pof), True),
        "multi_mes_unseeded": ("multi", False, 41, dict(seed=None, acquisition="mes"), False),
    }


CONFIGS = _configs()
POF = [n for n in CONFIGS if "_pof_" in n]
BELIEVER_BATCHES = ["multi_q3_believer", "mono_q3_believer"] + [n for n in POF if not n.endswith("_q1")]
FALLBACK = "multi_q3_thompson_fallback"


def _plain(v):
    """Arguments and results as JSON values: arrays as nested lists, a callable by the name of its class."""
    if v is None or isinstance(v, (bool, str)):
        return v
    if isinstance(v, (np.bool_,)):
        return bool(v)
    if isinstance(v, (int, np.integer)):
        return int(v)
    if isinstance(v, (float, np.floating)):
        return float(v)
    if isinstance(v, Token):
        return v.name
    if isinstance(v, dict):
        return {str(k): _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    if isinstance(v, np.ndarray):
        return v.tolist()
    if callable(v):
        return type(v).__name__
    raise TypeError(f"no trace form for {type(v).__name__}")


def _rng(*what):
    """A generator seeded by the values of a call's arguments."""
    return np.random.default_rng(zlib.crc32(json.dumps(_plain(what)).encode()))


class Token:
    """What a recorded fit returns in place of a surrogate."""

    def __init__(self, name):
        self.name = name


class FakeEngine:
    def __init__(self, trace, fail_thompson_call=None):
        self.trace, self.fail_thompson_call = trace, fail_thompson_call
        self.models, self.conditioned, self.thompson_calls, self.n_obj = None, False, 0, 0

    def load(self, models):
        models = list(models)
        same = self.models is not None and len(models) == len(self.models) and \
            all(a is b for a, b in zip(models, self.models))
        if not same or self.conditioned:
            self.trace.append(["load_models", [m.name for m in models]])
        self.models, self.conditioned, self.n_obj = models, False, len(models)
        return self

    def __getattr__(self, name):
        if not name.startswith(("plan_", "sample_")):
            raise AttributeError(name)

        def call(*args, **kw):
            self.trace.append([name, _plain(args), _plain(kw)])
            if name == "sample_minima":                     # (n_obj, S) minima of the sampled paths
                return _rng(name, args, kw).normal(size=(self.n_obj, args[0]))
        return call

    def maximise(self, acq_fn, lower, upper, **kw):
        self.trace.append(["maximise", acq_fn is None, _plain([lower, upper]), _plain(kw)])
        if acq_fn is not None:
            acq_fn(np.zeros((1, len(lower))))               # names the callable's engine method in the trace
        r = _rng("maximise", acq_fn is None, kw)
        return lower + (upper - lower) * r.random(len(lower)), float(r.random())

    def condition(self, Xnew, Y=None):
        self.trace.append(["condition", _plain(Xnew), _plain(Y)])
        self.conditioned = True
        # means around 0, so that a fantasy is feasible (g <= 0) about every other time
        return _rng("condition", Xnew).normal(size=(len(Xnew), self.n_obj))

    def thompson_batch(self, q, lower, upper, **kw):
        from optimobo_amd._lib import OMB_ENOTPD, OMBError
        self.trace.append(["thompson_batch", q, _plain([lower, upper]), _plain(kw)])
        self.thompson_calls += 1
        if self.thompson_calls == self.fail_thompson_call:
            raise OMBError(OMB_ENOTPD, "the draws' covariance is not positive definite")
        r = _rng("thompson_batch", q, kw)
        return lower + (upper - lower) * r.random((q, len(lower))), dict(indices=np.arange(q), zero_draws=0)

    def feasibility(self, Xd, n_con, pof_eps=1e-5):
        self.trace.append(["feasibility", n_con, pof_eps])
        return np.ones(len(Xd))

    def log_feasibility(self, Xd, n_con, pof_eps=1e-5):
        self.trace.append(["log_feasibility", n_con, pof_eps])
        return np.zeros(len(Xd))


def run(name):
    """The trace of configuration ``name`` as JSON values."""
    import optimobo_amd.acquisition as acquisition
    import optimobo_amd.algorithms._base as base
    import optimobo_amd.algorithms.optimisers as opti
    import optimobo_amd.scalarisations as sc
    driver, constrained, np_seed, kw, scalarise = CONFIGS[name]
    trace = []
    eng = FakeEngine(trace, fail_thompson_call=2 if name == FALLBACK else None)
    modules = [m for m in (acquisition, base, opti) if hasattr(m, "engine_for")]
    saved = [m.engine_for for m in modules]
    for m in modules:
        m.engine_for = lambda models, device=None: eng.load(models)
    try:
        cls = opti.MultiSurrogateOptimiser if driver == "multi" else opti.MonoSurrogateOptimiser
        opt = cls(_problem(constrained), IDEAL, MAX_POINT, **kw)
        fits = []

        def fit(X, y):
            fits.append(Token(f"fit{len(fits)}"))
            trace.append(["_fit", fits[-1].name, _plain(np.asarray(X)), _plain(np.asarray(y))])
            return fits[-1]

        def fit_many(X, ys):
            new = [Token(f"fit{len(fits) + i}") for i in range(np.shape(ys)[1])]
            fits.extend(new)
            trace.append(["_fit_many", [t.name for t in new], _plain(np.asarray(X)), _plain(np.asarray(ys))])
            return new
        opt._fit, opt._fit_many = fit, fit_many
        tch = sc.Tchebicheff(IDEAL, MAX_POINT) if scalarise else None
        np.random.seed(np_seed)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)           # a Thompson fallback says so
            if driver == "multi":
                res = opt.solve(budget=BUDGET, n_init_samples=N_INIT, sample_exponent=SAMPLE_EXPONENT,
                                acquisition_func=tch)
            else:
                res = opt.solve(tch, budget=BUDGET, n_init_samples=N_INIT)
        state = np.random.get_state()
        trace.append(["end", dict(result=type(res).__name__, Xsample=res.Xsample, ysample=res.ysample,
                                  hypervolume_convergence=list(res.hypervolume_convergence),
                                  numpy_state=state[1], numpy_pos=state[2], _iteration=opt._iteration,
                                  _mes_picks=opt._mes_picks, thompson_fallbacks=opt.thompson_fallbacks)])
    finally:
        for m, f in zip(modules, saved):
            m.engine_for = f
    return _plain(trace)


def pof_pick_kinds(trace):
    """(picks that maximised the feasibility alone, picks that planned an acquisition and weighted it)."""
    alone = sum(r[0] == "maximise" and r[1] is False for r in trace)
    return alone, sum(r[0] == "plan_constraints" for r in trace)


def check_fixture(traces):
    """What keeps a degenerate fixture from passing: both kinds of pick under constraints="pof", conditioning in
    every believer batch, and the fallback taken once."""
    assert sorted(traces) == sorted(CONFIGS)
    alone, planned = map(sum, zip(*(pof_pick_kinds(traces[n]) for n in POF)))
    assert alone >= 1 and planned >= 1, (alone, planned)
    for n in POF:
        assert traces[n][-1][1]["result"] == "Constrained_Res"
    for n in BELIEVER_BATCHES:
        assert any(r[0] == "condition" for r in traces[n]), n
    assert traces[FALLBACK][-1][1]["thompson_fallbacks"] == 1
    assert any(r[0] == "condition" for r in traces[FALLBACK])         # the fallback built a believer batch


if __name__ == "__main__":
    traces = {n: run(n) for n in CONFIGS}
    for n in CONFIGS:
        assert run(n) == traces[n], f"{n}: two runs give two traces"
    check_fixture(traces)
    for n in POF:
        print(n, "picks (feasibility alone, planned):", pof_pick_kinds(traces[n]))
    with open(FIXTURE, "w") as fh:
        fh.write("{\n" + ",\n".join(
            json.dumps(n) + ": [\n" + ",\n".join(json.dumps(r) for r in t) + "\n]" for n, t in traces.items()) + "\n}\n")
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")
