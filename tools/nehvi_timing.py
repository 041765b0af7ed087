"""The noisy EHVI / noisy EI on the device: per-launch times and the drivers' acquisition="nehvi".

    python tools/nehvi_timing.py [--kernels-only | --chain-only | --drivers-only] [--seeds 5] [--budget 40]

Kernels and chains — each group alternates in one process after a warm-up of all its variants, timed by device events
around back-to-back launches (tools/logacq_timing.py's ``alternate``: medians of 7):
  * omb_hvi_paths against the only other way to the same number, S calls of omb_hvi_boxes on the paths' row slices and
    their sum in path order, at N = 2^16 / 2^18 / 2^20 for (k, S, front size) = (1, 16, –), (2, 16, 50), (3, 8, 50)
    (k = 1 has no omb_hvi_boxes: its baseline is the torch expression mean_s (b_s − y)⁺); values compared once per shape;
  * the omb_eval chain of omb_plan_hvi_paths at n = 128 and 512, d 6, m 1024, k 2, S 16, in passes of
    2^16 / 2^17 / 2^18 candidates and in one pass (OMB_DEBUG_HVI_PATHS_CHUNK), against its two stages alone and the
    exact-EHVI chain (omb_plan_ehvi_boxes over the observed front) at the same N.
Drivers — MultiSurrogateOptimiser.solve on the README problem with Gaussian noise of standard deviation 1 % and 5 % of
each objective's range added to every evaluation, noise="fit", budget 40 from 20 initial samples, mode "textbook": the
default acquisition (exact EHVI over the observed front), acquisition="nehvi" and acquisition="mes", alternating
within every seed after one warm-up round: the hypervolume of the noise-free objective values at the evaluated points
(per seed and median), ms per true evaluation and its fit / proposal split.
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

from optimobo_amd import _lib, pareto, paths  # noqa: E402
from optimobo_amd.device import AcqContext  # noqa: E402


def simplex_front(k, P, rng):
    return rng.dirichlet(np.ones(k), size=P)


def kernels():
    ctx = AcqContext(0)
    dev = ctx.device
    for k, S, P in ((1, 16, None), (2, 16, 50), (3, 8, 50)):
        rng = np.random.default_rng(10 * k + S)
        if k == 1:
            b = rng.normal(size=S)
            lists = pareto.pack_box_lists(pareto.threshold_lists(b))
        else:
            lists = pareto.pack_box_lists([pareto.box_decomposition(simplex_front(k, P, rng), np.full(k, 1.1))
                                           for _ in range(S)])
        coords, off, boxes = lists
        cd = [torch.as_tensor(coords[s], device=dev) for s in range(S)]
        bd = [ctx._boxes_dev(boxes[off[s]:off[s + 1]]) for s in range(S)]
        for N in (1 << 16, 1 << 18, 1 << 20):
            y = torch.as_tensor(rng.uniform(-0.2, 1.3, (k, S, N)), device=dev)
            out = torch.empty(N, dtype=torch.float64, device=dev)
            ts = torch.empty((S, N), dtype=torch.float64, device=dev)
            if k == 1:
                bt = torch.as_tensor(b, device=dev)[:, None]

                def baseline():
                    return torch.clamp(bt - y[0], min=0.0).sum(0) / S
            else:
                def baseline():
                    for s in range(S):
                        ctx.hvi_boxes(y[:, s, :], cd[s], bd[s], out=ts[s])
                    total = ts[0].clone()
                    for s in range(1, S):
                        total += ts[s]
                    return total / S
            res = alternate([("S x omb_hvi_boxes + sum" if k > 1 else "torch clamp + sum", baseline),
                             ("omb_hvi_paths", lambda: ctx.hvi_paths(y, *lists, out=out))])
            got, want = ctx.hvi_paths(y, *lists), baseline()
            emit({"kernel": "hvi_paths", "k": k, "S": S, "front": P, "boxes": int(off[-1]), "C": int(coords.shape[2]),
                  "N": N, "values_bitwise_equal": bool(torch.equal(got, want)),
                  "max_abs_diff": float((got - want).abs().max())}, res)
            del y, out, ts
    ctx.close()


def chain():
    ctx = AcqContext(0)
    dev = ctx.device
    S, d, m, k = 16, 6, 1024, 2
    for n in (128, 512):
        rng = np.random.default_rng(n + d)
        sts = states(ctx, n, d, k, rng)
        for o, st in enumerate(sts):
            ctx.paths_set(o, *paths.draw_path_inputs("matern52", n, d, S, m, rng, np.zeros(d), np.ones(d), st.lengthscale),
                          noise=1e-6)
        Xt = torch.as_tensor(sts[0].X, device=dev)
        F = ctx.paths_eval(Xt, k).cpu().numpy()
        Y = np.stack([st.y.reshape(-1) for st in sts], 1)
        r = Y.max(0) + 0.1
        lists = pareto.pack_box_lists([pareto.box_decomposition(pareto.calc_pf(np.ascontiguousarray(F[:, s, :].T)), r)
                                       for s in range(S)])
        exact = pareto.box_decomposition(pareto.calc_pf(Y), r)
        for N in (1 << 16, 1 << 20):
            Xc = torch.as_tensor(np.random.default_rng(N).uniform(0.0, 1.0, (N, d)), device=dev)
            vals = torch.empty(N, dtype=torch.float64, device=dev)
            yb = torch.empty((k, S, N), dtype=torch.float64, device=dev)
            ctx.paths_eval(Xc, k, out=yb)

            # the plan and the chunk are set outside the timed launches: one group per plan
            ctx.plan_hvi_paths(*lists)
            # the pass size is context state, so every variant sets its own before it launches (a host-side store)
            def passes(c):
                def f():
                    ctx.debug_set("hvi_paths_chunk", c)
                    return ctx.eval(Xc, out=vals)
                return f
            a = passes(1 << 16)().clone()
            b = passes(0)().clone()
            res = alternate([("omb_eval(plan_hvi_paths), one pass", passes(0)),
                             ("omb_eval(plan_hvi_paths), passes of 2^16", passes(1 << 16)),
                             ("omb_eval(plan_hvi_paths), passes of 2^17", passes(1 << 17)),
                             ("omb_eval(plan_hvi_paths), passes of 2^18", passes(1 << 18)),
                             ("omb_paths_eval", lambda: ctx.paths_eval(Xc, k, out=yb)),
                             ("omb_hvi_paths", lambda: ctx.hvi_paths(yb, *lists, out=vals))])
            ctx.debug_set("hvi_paths_chunk", _lib.HVI_PATHS_CHUNK)
            ctx.plan_ehvi_boxes(exact[0], exact[2])
            res.update(alternate([("omb_eval(plan_ehvi_boxes)", lambda: ctx.eval(Xc, out=vals))]))
            emit({"chain": "nehvi", "n": n, "d": d, "m": m, "k": k, "S": S, "N": N, "boxes": int(lists[1][-1]),
                  "exact_boxes": int(len(exact[2])), "matrix_MB": round(8e-6 * k * S * N, 1),
                  "default_chunk": _lib.HVI_PATHS_CHUNK, "chunked_equals_one_pass": bool(torch.equal(a, b))}, res)
            del Xc, vals, yb
    ctx.close()


def drivers(seeds, budget):
    import optimobo_amd.algorithms.optimisers as opti
    from optimobo_amd.problem import ElementwiseProblem

    def clean(x):
        return np.array([100 * (x[0] ** 2 + x[1] ** 2), (x[0] - 1) ** 2 + x[1] ** 2])

    span = np.array([800.0, 13.0])      # the objectives' ranges over the box [-2, 2]^2

    class Noisy(ElementwiseProblem):
        def __init__(self, rel, seed):
            super().__init__(n_var=2, n_obj=2, xl=np.array([-2, -2]), xu=np.array([2, 2]))
            self.sd = rel * span
            self.rng = np.random.default_rng(seed)

        def _evaluate(self, x, out, *a, **k):
            out["F"] = list(clean(x) + self.sd * self.rng.standard_normal(2))

    variants = {"ehvi_exact": dict(), "nehvi": dict(acquisition="nehvi"), "mes": dict(acquisition="mes")}

    def run(name, rel, seed):
        np.random.seed(seed)
        opt = opti.MultiSurrogateOptimiser(Noisy(rel, seed), [0, 0], [700, 12], seed=seed + 1, mode="textbook",
                                           noise="fit", **variants[name])
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
        opt._get_proposed_EHVI = timed("propose", opt._get_proposed_EHVI)
        t0 = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res = opt.solve(budget=budget, n_init_samples=20)
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        hv = pareto.hypervolume(np.array([clean(x) for x in res.Xsample]), np.array([700.0, 12.0]))
        return [el / budget, split["fit"] / budget, split["propose"] / budget, float(hv)]

    for rel in (0.01, 0.05):
        t = {k: [] for k in variants}
        for seed in range(-1, seeds):          # seed −1 is the warm-up round
            for name in variants:
                r = run(name, rel, max(seed, 0))
                if seed >= 0:
                    t[name].append(r)
        for name, v in t.items():
            a = np.array(v)
            print(json.dumps({"variant": name, "noise_sd_of_range": rel, "budget": budget, "n_init": 20, "seeds": seeds,
                              "ms_per_evaluation": {"median": float(np.median(a[:, 0]) * 1e3),
                                                    "min": float(a[:, 0].min() * 1e3), "max": float(a[:, 0].max() * 1e3)},
                              "fit_ms_per_evaluation": float(np.median(a[:, 1]) * 1e3),
                              "propose_ms_per_evaluation": float(np.median(a[:, 2]) * 1e3),
                              "noise_free_hypervolume": [float(x) for x in a[:, 3]],
                              "median_noise_free_hypervolume": float(np.median(a[:, 3]))}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--chain-only", action="store_true")
    ap.add_argument("--drivers-only", action="store_true")
    ap.add_argument("--seeds", type=int, default=5)
    ap.add_argument("--budget", type=int, default=40)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("nehvi_timing needs the GPU: a CPU run measures nothing")
    only = args.kernels_only or args.chain_only or args.drivers_only
    if args.kernels_only or not only:
        kernels()
    if args.chain_only or not only:
        chain()
    if args.drivers_only or not only:
        drivers(args.seeds, args.budget)


if __name__ == "__main__":
    main()
