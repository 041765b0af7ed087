"""Max-value entropy search on the device: per-launch times and the drivers' acquisition="mes".

    python tools/mes_timing.py [--drivers-only | --kernels-only] [--seeds 5] [--budget 40] > mes_timing.jsonl

Kernels — each group alternates in one process after a warm-up of all its variants, timed by device events around
back-to-back launches (tools/logacq_timing.py's ``alternate``: medians of 7):
  * omb_paths_min against the only other way to the same numbers, omb_paths_eval into an (n_obj·S, N) matrix and a
    torch row-min, at DESIGN §21's shapes: 16 paths, 2 objectives, d 6, m 1024, n 128 and 512, N = 2^16 / 2^18 / 2^20
    (the values and indices of the two are compared once per shape);
  * omb_mes, the posterior (every σ², as the plan asks) and the whole omb_eval chain of omb_plan_mes at 2^20
    candidates, n 512, d 6, for (k, S) = (1, 8), (2, 8), (2, 16).
Drivers — MultiSurrogateOptimiser.solve on the README problem, budget 40 from 20 initial samples, mode "textbook":
the default acquisition (exact 2-D EHVI) against acquisition="mes" (8 sampled minima per pick over 2^16 candidates),
alternating within every seed after one warm-up round: ms per true evaluation (median, min, max over the seeds), its
fit / proposal split and the last hypervolume entry of every seed, as tools/thompson_batch_timing.py reports them.
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from logacq_timing import alternate  # noqa: E402

from optimobo_amd import paths  # noqa: E402
from optimobo_amd.device import AcqContext  # noqa: E402
from optimobo_amd.gp import GPState  # noqa: E402


def emit(shape, res):
    base = None
    for name, (launches, us) in res.items():
        med = float(np.median(us))
        base = med if base is None else base
        print(json.dumps(dict(shape, variant=name, launches_per_repeat=launches, us_per_launch=[round(u, 2) for u in us],
                              median_us=round(med, 2), spread=round((max(us) - min(us)) / med, 4),
                              over_first=round(med / base, 3))), flush=True)


def states(ctx, n, d, k, rng):
    X = rng.uniform(0.0, 1.0, (n, d))
    out = []
    for o in range(k):
        y = np.sin(3.0 * X + o).sum(1)
        st = GPState(X, y, rng.uniform(0.3, 1.2, d) * np.sqrt(d), float(np.var(y) + 0.1), noise=1e-6)
        ctx.set_gp(o, st.X, st.lengthscale, st.variance, st.alpha, st.Linv)
        out.append(st)
    return out


def kernels():
    ctx = AcqContext(0)
    dev = ctx.device
    S, d, m, k = 16, 6, 1024, 2
    for n in (128, 512):
        rng = np.random.default_rng(n + d)
        for o, st in enumerate(states(ctx, n, d, k, rng)):
            ctx.paths_set(o, *paths.draw_path_inputs("matern52", n, d, S, m, rng, np.zeros(d), np.ones(d), st.lengthscale),
                          noise=1e-6)
        for N in (1 << 16, 1 << 18, 1 << 20):
            Xc = torch.as_tensor(np.random.default_rng(N).uniform(0.0, 1.0, (N, d)), device=dev)
            out = torch.empty((k, S, N), dtype=torch.float64, device=dev)

            def eval_then_min():
                return ctx.paths_eval(Xc, k, out=out).min(dim=-1)
            res = alternate([("paths_eval_then_torch_min", eval_then_min), ("omb_paths_min", lambda: ctx.paths_min(Xc, k))])
            v, i = ctx.paths_min(Xc, k)
            w = eval_then_min()
            emit({"kernel": "paths_min", "n": n, "d": d, "m": m, "k": k, "S": S, "N": N,
                  "matrix_MB": round(8e-6 * k * S * N, 1), "values_bitwise_equal": bool(torch.equal(v, w.values)),
                  "indices_equal": bool(torch.equal(i, w.indices))}, res)
            del out
    N, n = 1 << 20, 512
    rng = np.random.default_rng(7)
    states(ctx, n, d, 2, rng)
    Xc = torch.as_tensor(rng.uniform(0.0, 1.0, (N, d)), device=dev)
    vals = torch.empty(N, dtype=torch.float64, device=dev)
    for kk, SS in ((1, 8), (2, 8), (2, 16)):
        mu, var = ctx.posterior(Xc, kk)
        ys = mu.min(dim=1).values.cpu().numpy()[:, None] - 0.05 * rng.uniform(0.0, 1.0, (kk, SS))
        ctx.plan_mes(ys)
        pm, pv = torch.empty_like(mu), torch.empty_like(var)
        res = alternate([("omb_posterior", lambda: ctx.posterior(Xc, kk, out=(pm, pv))),
                         ("omb_mes", lambda: ctx.mes(mu, var, ys, out=vals)),
                         ("omb_eval(plan_mes)", lambda: ctx.eval(Xc, out=vals)),
                         ("omb_eval_argmax(plan_mes)", lambda: ctx.eval_argmax(Xc))])
        emit({"kernel": "mes", "n": n, "d": d, "k": kk, "S": SS, "N": N}, res)
    ctx.close()


def drivers(seeds, budget):
    import optimobo_amd.algorithms.optimisers as opti
    from optimobo_amd.problem import ElementwiseProblem

    class MyProblem(ElementwiseProblem):
        def __init__(self):
            super().__init__(n_var=2, n_obj=2, xl=np.array([-2, -2]), xu=np.array([2, 2]))

        def _evaluate(self, x, out, *a, **k):
            out["F"] = [100 * (x[0] ** 2 + x[1] ** 2), (x[0] - 1) ** 2 + x[1] ** 2]

    variants = {"ehvi_exact": dict(mode="textbook"), "mes": dict(mode="textbook", acquisition="mes")}

    def run(name, seed):
        np.random.seed(seed)
        opt = opti.MultiSurrogateOptimiser(MyProblem(), [0, 0], [700, 12], seed=seed + 1, **variants[name])
        split = {"fit": 0.0, "propose": 0.0}

        def timed(key, fn):
            def w(*a, **k):
                t = time.perf_counter()
                out = fn(*a, **k)
                torch.cuda.synchronize()
                split[key] += time.perf_counter() - t
                return out
            return w
        opt._fit_many = timed("fit", opt._fit_many)
        opt._get_proposed_EHVI = timed("propose", opt._get_proposed_EHVI)      # the plan (MES: its sample paths) and the search
        t0 = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res = opt.solve(budget=budget, n_init_samples=20)
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        return [el / budget, split["fit"] / budget, split["propose"] / budget, float(res.hypervolume_convergence[-1])]

    t = {k: [] for k in variants}
    for seed in range(-1, seeds):          # seed −1 is the warm-up round
        for name in variants:
            r = run(name, max(seed, 0))
            if seed >= 0:
                t[name].append(r)
    for name, v in t.items():
        a = np.array(v)
        print(json.dumps({"variant": name, "budget": budget, "n_init": 20, "seeds": seeds,
                          "ms_per_evaluation": {"median": float(np.median(a[:, 0]) * 1e3), "min": float(a[:, 0].min() * 1e3),
                                                "max": float(a[:, 0].max() * 1e3)},
                          "fit_ms_per_evaluation": float(np.median(a[:, 1]) * 1e3),
                          "propose_ms_per_evaluation": float(np.median(a[:, 2]) * 1e3),
                          "last_hypervolume_entry": [float(x) for x in a[:, 3]],
                          "median_last_hypervolume_entry": float(np.median(a[:, 3]))}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--drivers-only", action="store_true")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--seeds", type=int, default=5)
    ap.add_argument("--budget", type=int, default=40)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mes_timing needs the GPU: a CPU run measures nothing")
    if not args.drivers_only:
        kernels()
    if not args.kernels_only:
        drivers(args.seeds, args.budget)


if __name__ == "__main__":
    main()
