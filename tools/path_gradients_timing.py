"""The sample paths' gradient: kernel times, the cost of a polish, and the drivers with it switched on.

    python tools/path_gradients_timing.py [--kernels-only | --polish-only | --drivers-only] [--seeds 5] [--budget 40]

  kernels   omb_paths_grad against omb_paths_eval on the same points at N = 16, 1024, 2^16 for (n 128, d 6, m 1024,
            2 objectives) and (n 1024, d 30, m 2048, 1 objective), S = 16; omb_hvi_paths_grad (with the per-path
            outputs) against omb_hvi_paths at the same N for tools/nehvi_timing.py's k = 2 (S 16, 50-point fronts) and
            k = 3 (S 8) lists, d = 6.  Device events around back-to-back launches after a warm-up, the variants taking
            turns (tools/logacq_timing.py's ``alternate``).
  polish    one ``maximise`` under the noisy-EHVI plan (k = 2, S = 16, m = 1024, d = 6, 2^14 candidates, 4 starts) with
            polish="paths" against polish=True (the stencil) and polish=False: wall clock per call (median of 5 after
            a warm-up) and the value reached, at n_train 128 and 512.
  drivers   the README problem, budget 40 from 20 initial samples, five seeds alternated after a warm-up round, every
            variant with ``path_gradients`` off and on: acquisition="mes" and thompson_sampler="paths" (batch_size 4)
            on the noise-free problem (last hypervolume entry), acquisition="nehvi" under Gaussian noise of 1 % / 5 %
            of each objective's range with noise="fit" (hypervolume of the noise-free values of the evaluated points).
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
from mes_timing import emit, states  # noqa: E402

from optimobo_amd import pareto, paths  # noqa: E402
from optimobo_amd.device import AcqContext  # noqa: E402

NS = (16, 1024, 1 << 16)


def kernels():
    ctx = AcqContext(0)
    dev = ctx.device
    S = 16
    for n, d, m, k in [(128, 6, 1024, 2), (1024, 30, 2048, 1)]:
        rng = np.random.default_rng(n + d)
        for o, st in enumerate(states(ctx, n, d, k, rng)):
            ctx.paths_set(o, *paths.draw_path_inputs("matern52", n, d, S, m, rng, np.zeros(d), np.ones(d), st.lengthscale),
                          noise=1e-6)
        for N in NS:
            Xc = torch.as_tensor(np.random.default_rng(N).uniform(0.0, 1.0, (N, d)), device=dev)
            out = torch.empty((k, S, N), dtype=torch.float64, device=dev)
            res = alternate([("omb_paths_eval", lambda: ctx.paths_eval(Xc, k, out=out)),
                             ("omb_paths_grad", lambda: ctx.paths_grad(Xc, k))])
            v, _ = ctx.paths_grad(Xc, k)
            emit({"kernel": "paths_grad", "n": n, "d": d, "m": m, "k": k, "S": S, "N": N,
                  "values_bitwise_equal": bool(torch.equal(v, ctx.paths_eval(Xc, k)))}, res)
    d = 6
    for k, S, P in ((2, 16, 50), (3, 8, 50)):
        rng = np.random.default_rng(10 * k + S)
        lists = pareto.pack_box_lists([pareto.box_decomposition(rng.dirichlet(np.ones(k), size=P), np.full(k, 1.1))
                                       for _ in range(S)])
        for N in NS:
            y = torch.as_tensor(rng.uniform(-0.2, 1.3, (k, S, N)), device=dev)
            dy = torch.as_tensor(rng.normal(size=(k, S, d, N)), device=dev)
            out = torch.empty(N, dtype=torch.float64, device=dev)
            res = alternate([("omb_hvi_paths", lambda: ctx.hvi_paths(y, *lists, out=out)),
                             ("omb_hvi_paths_grad", lambda: ctx.hvi_paths_grad(y, dy, *lists)),
                             ("omb_hvi_paths_grad per_path", lambda: ctx.hvi_paths_grad(y, dy, *lists, per_path=True))])
            emit({"kernel": "hvi_paths_grad", "k": k, "S": S, "d": d, "front": P, "boxes": int(lists[1][-1]), "N": N,
                  "values_bitwise_equal": bool(torch.equal(ctx.hvi_paths_grad(y, dy, *lists)[0],
                                                           ctx.hvi_paths(y, *lists)))}, res)
    ctx.close()


def polish():
    from optimobo_amd.acquisition import AcquisitionEngine
    from optimobo_amd.gp import GPState
    d, k, S, m = 6, 2, 16, 1024
    eng = AcquisitionEngine(0)
    lo, hi = np.zeros(d), np.ones(d)
    for n in (128, 512):
        rng = np.random.default_rng(n + d)
        X = rng.uniform(0.0, 1.0, (n, d))
        Y = np.stack([np.sin(3.0 * X + o).sum(1) for o in range(k)], 1)
        models = [GPState(X, Y[:, o], rng.uniform(0.3, 1.2, d) * np.sqrt(d), float(np.var(Y[:, o]) + 0.1), noise=1e-6)
                  for o in range(k)]
        eng.load_models(models)
        eng.sample_fronts(S, Y.max(0) + 0.1, lo, hi, seed=1, n_features=m)
        eng.plan_nehvi()
        for name, p in (("polish=False", False), ("polish=True (stencil)", True), ("polish='paths'", "paths")):
            ms, val = [], None
            for rep in range(6):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _, val = eng.maximise(None, lo, hi, n_candidates=1 << 14, seed=3, refine_rounds=2, polish=p, starts=4)
                torch.cuda.synchronize()
                if rep:
                    ms.append((time.perf_counter() - t0) * 1e3)
            print(json.dumps({"maximise": "plan_nehvi", "n": n, "d": d, "k": k, "S": S, "m": m, "variant": name,
                              "ms_per_call": [round(x, 2) for x in ms], "median_ms": round(float(np.median(ms)), 2),
                              "value": float(val)}), flush=True)
    eng.ctx.close()


def drivers(seeds, budget):
    import optimobo_amd.algorithms.optimisers as opti
    from optimobo_amd.problem import ElementwiseProblem

    def clean(x):
        return np.array([100 * (x[0] ** 2 + x[1] ** 2), (x[0] - 1) ** 2 + x[1] ** 2])

    span = np.array([800.0, 13.0])      # the objectives' ranges over the box [-2, 2]^2

    class Problem(ElementwiseProblem):
        def __init__(self, rel, seed):
            super().__init__(n_var=2, n_obj=2, xl=np.array([-2, -2]), xu=np.array([2, 2]))
            self.sd = rel * span
            self.rng = np.random.default_rng(seed)

        def _evaluate(self, x, out, *a, **k):
            out["F"] = list(clean(x) + (self.sd * self.rng.standard_normal(2) if self.sd.any() else 0.0))

    groups = [("mes", 0.0, dict(acquisition="mes")),
              ("thompson_paths", 0.0, dict(batch_strategy="thompson", thompson_sampler="paths", batch_size=4)),
              ("nehvi", 0.01, dict(acquisition="nehvi", noise="fit")),
              ("nehvi", 0.05, dict(acquisition="nehvi", noise="fit"))]

    def run(kw, rel, seed, pg):
        np.random.seed(seed)
        opt = opti.MultiSurrogateOptimiser(Problem(rel, seed), [0, 0], [700, 12], seed=seed + 1, mode="textbook",
                                           path_gradients=pg, **kw)
        t0 = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res = opt.solve(budget=budget, n_init_samples=20)
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        hv = pareto.hypervolume(np.array([clean(x) for x in res.Xsample]), np.array([700.0, 12.0]))
        return [el / budget, float(res.hypervolume_convergence[-1]), float(hv)]

    for name, rel, kw in groups:
        t = {False: [], True: []}
        for seed in range(-1, seeds):          # seed −1 is the warm-up round
            for pg in (False, True):
                r = run(kw, rel, max(seed, 0), pg)
                if seed >= 0:
                    t[pg].append(r)
        for pg, v in t.items():
            a = np.array(v)
            print(json.dumps({"variant": name, "path_gradients": pg, "noise_sd_of_range": rel, "budget": budget,
                              "n_init": 20, "seeds": seeds,
                              "ms_per_evaluation": {"median": float(np.median(a[:, 0]) * 1e3),
                                                    "min": float(a[:, 0].min() * 1e3), "max": float(a[:, 0].max() * 1e3)},
                              "last_hypervolume_entry": [float(x) for x in a[:, 1]],
                              "median_last_hypervolume_entry": float(np.median(a[:, 1])),
                              "noise_free_hypervolume": [float(x) for x in a[:, 2]],
                              "median_noise_free_hypervolume": float(np.median(a[:, 2]))}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--polish-only", action="store_true")
    ap.add_argument("--drivers-only", action="store_true")
    ap.add_argument("--seeds", type=int, default=5)
    ap.add_argument("--budget", type=int, default=40)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("path_gradients_timing needs the GPU: a CPU run measures nothing")
    only = args.kernels_only or args.polish_only or args.drivers_only
    if args.kernels_only or not only:
        kernels()
    if args.polish_only or not only:
        polish()
    if args.drivers_only or not only:
        drivers(args.seeds, args.budget)


if __name__ == "__main__":
    main()
