"""The drivers' batch strategies on the README problem: wall time per true evaluation and the last hypervolume entry.

    python tools/thompson_batch_timing.py [--out FILE] [--seeds 5] [--budget 40]

``MultiSurrogateOptimiser.solve`` on the 2-objective README problem, budget 40 from 20 initial samples, batch_size 4:
  believer_tch      the Tchebicheff expected decomposition with the Kriging believer (tools/append_timing.py's
                    batch_size 4 row, measured again here);
  believer_ehvi     the exact 2-D EHVI (mode "textbook") with the Kriging believer;
  thompson_ehvi     batch_strategy="thompson" at the default candidate count (hypervolume improvement of joint
                    posterior draws; it takes the EHVI acquisitions only, so believer_ehvi is its counterpart);
  thompson_paths    the same with thompson_sampler="paths": posterior sample paths at 2^16 candidates and two
                    refinement rounds around every nominee (nothing factorised, so no fallback can arise).
The variants alternate within every seed after one warm-up round; wall clock around a solve that ends in a
synchronise.  One JSON line per variant: ms per true evaluation (median, min, max over the seeds), its fit /
proposal split, the last hypervolume entry of every seed, and the Thompson iterations that fell back.
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--seeds", type=int, default=5)
    ap.add_argument("--budget", type=int, default=40)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("thompson_batch_timing needs the GPU: a CPU run measures nothing")
    import optimobo_amd.algorithms.optimisers as opti
    import optimobo_amd.scalarisations as sc
    from optimobo_amd.problem import ElementwiseProblem

    class MyProblem(ElementwiseProblem):
        def __init__(self):
            super().__init__(n_var=2, n_obj=2, xl=np.array([-2, -2]), xu=np.array([2, 2]))

        def _evaluate(self, x, out, *a, **k):
            out["F"] = [100 * (x[0] ** 2 + x[1] ** 2), (x[0] - 1) ** 2 + x[1] ** 2]

    variants = {"believer_tch": dict(kw={}, tch=True),
                "believer_ehvi": dict(kw=dict(mode="textbook"), tch=False),
                "thompson_ehvi": dict(kw=dict(mode="textbook", batch_strategy="thompson"), tch=False),
                "thompson_paths": dict(kw=dict(mode="textbook", batch_strategy="thompson", thompson_sampler="paths"),
                                       tch=False)}

    def run(name, seed):
        v = variants[name]
        np.random.seed(seed)
        opt = opti.MultiSurrogateOptimiser(MyProblem(), [0, 0], [700, 12], seed=seed + 1, batch_size=4, **v["kw"])
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
        opt._maximise = timed("propose", opt._maximise)
        opt._thompson_picks = timed("propose", opt._thompson_picks)
        extra = dict(sample_exponent=3, acquisition_func=sc.Tchebicheff([0, 0], [700, 12])) if v["tch"] else {}
        t0 = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res = opt.solve(budget=args.budget, n_init_samples=20, **extra)
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        return [el / args.budget, split["fit"] / args.budget, split["propose"] / args.budget,
                float(res.hypervolume_convergence[-1]), opt.thompson_fallbacks]

    t = {k: [] for k in variants}
    for seed in range(-1, args.seeds):          # seed −1 is the warm-up round
        for name in variants:
            r = run(name, max(seed, 0))
            if seed >= 0:
                t[name].append(r)
    rows = []
    for name, v in t.items():
        a = np.array(v)
        row = {"variant": name, "batch_size": 4, "budget": args.budget, "n_init": 20, "seeds": args.seeds,
               "ms_per_evaluation": {"median": float(np.median(a[:, 0]) * 1e3), "min": float(a[:, 0].min() * 1e3),
                                     "max": float(a[:, 0].max() * 1e3)},
               "fit_ms_per_evaluation": float(np.median(a[:, 1]) * 1e3),
               "propose_ms_per_evaluation": float(np.median(a[:, 2]) * 1e3),
               "last_hypervolume_entry": [float(x) for x in a[:, 3]],
               "median_last_hypervolume_entry": float(np.median(a[:, 3])),
               "thompson_fallbacks": [int(x) for x in a[:, 4]]}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
