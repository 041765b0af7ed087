"""Constraints through sample paths on the device: per-launch times and the drivers' constraints="paths".

    python tools/nehvi_con_timing.py [--kernels-only | --chain-only | --skip-only | --drivers-only] [--seeds 5] [--budget 30]

Kernels and chains — each group alternates in one process after a warm-up of all its variants, timed by device events
around back-to-back launches (tools/logacq_timing.py's ``alternate``: medians of 7):
  * omb_hvi_paths_con (with and without the per-path output) against the other way to the same numbers — S calls of
    omb_hvi_boxes on the paths' row slices (k = 1: the torch expression (b_s − y)⁺), a torch indicator weight per path
    and the sum in path order — at
    N = 2^16 / 2^18 / 2^20 for (k, c, S, front size) = (1, 1, 16, –), (2, 1, 16, 50), (2, 2, 16, 50), with the
    indicator and with the sigmoid (eta = 0.05); omb_hvi_paths alone at the same N stands beside them;
  * the omb_eval chain of omb_plan_hvi_paths_con at n = 128 and 512, d 6, m 1024, k 2, S 16 with c = 0, 1 and 2
    constraint models, against its two stages alone: the expectation is one more slot of path evaluation per
    constraint, about 1/k of the posterior stage;
  * the skip: the kernel at k 2, c 1, S 16, N 2^20 with 1 %, 50 % and 100 % of the candidates feasible (under every
    path at once, in runs of whole wavefronts and scattered), against omb_hvi_paths on the same objectives.
Drivers — MultiSurrogateOptimiser.solve on the tests' constrained problem (two variables, g = 1.5 − x0 − x1 ≤ 0) with
Gaussian noise of standard deviation 1 % and 5 % of each objective's range on every objective evaluation (the
constraint is observed exactly), noise="fit", mode "textbook": constraints="pof" (exact EHVI over the observed
feasible front times the probability of feasibility) against acquisition="nehvi" with constraints="paths",
alternating within every seed after one warm-up round: the feasible proposals and the hypervolume of the noise-free
objective values at the feasible evaluated points.
"""
import argparse
import json
import os
import sys
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from logacq_timing import alternate  # noqa: E402
from mes_timing import emit, states  # noqa: E402
from nehvi_timing import simplex_front  # noqa: E402

from optimobo_amd import pareto, paths  # noqa: E402
from optimobo_amd.device import AcqContext  # noqa: E402


def lists_for(k, S, P, rng):
    if k == 1:
        return pareto.pack_box_lists(pareto.threshold_lists(rng.normal(size=S)))
    return pareto.pack_box_lists([pareto.box_decomposition(simplex_front(k, P, rng), np.full(k, 1.1)) for _ in range(S)])


def kernels():
    ctx = AcqContext(0)
    dev = ctx.device
    for k, c, S, P in ((1, 1, 16, None), (2, 1, 16, 50), (2, 2, 16, 50)):
        rng = np.random.default_rng(100 * k + 10 * c + S)
        lists = lists_for(k, S, P, rng)
        coords, off, boxes = lists
        cd = [torch.as_tensor(coords[s], device=dev) for s in range(S)]
        bd = [ctx._boxes_dev(boxes[off[s]:off[s + 1]]) for s in range(S)]
        bt = torch.as_tensor(coords[:, 0, 1].copy(), device=dev)[:, None]
        for N in (1 << 16, 1 << 18, 1 << 20):
            y = torch.as_tensor(np.concatenate([rng.uniform(-0.2, 1.3, (k, S, N)),
                                                rng.normal(size=(c, S, N)) - 0.3]), device=dev)
            out = torch.empty(N, dtype=torch.float64, device=dev)
            ts = torch.empty((S, N), dtype=torch.float64, device=dev)

            def baseline():
                if k == 1:
                    torch.clamp(bt - y[0], min=0.0, out=ts)
                else:
                    for s in range(S):
                        ctx.hvi_boxes(y[:k, s, :], cd[s], bd[s], out=ts[s])
                u = ts * (y[k:] <= 0).all(0)
                total = u[0].clone()
                for s in range(1, S):
                    total += u[s]
                return total / S, u
            res = alternate([("omb_hvi_boxes per path (k = 1: torch) + torch weight + sum", baseline),
                             ("omb_hvi_paths_con, indicator", lambda: ctx.hvi_paths_con(y, c, *lists, out=out)),
                             ("omb_hvi_paths_con, indicator, per-path output",
                              lambda: ctx.hvi_paths_con(y, c, *lists, out=out, per_path=True)),
                             ("omb_hvi_paths_con, sigmoid eta 0.05", lambda: ctx.hvi_paths_con(y, c, *lists, eta=0.05, out=out)),
                             ("omb_hvi_paths (objectives alone)", lambda: ctx.hvi_paths(y[:k], *lists, out=out))])
            got, gu = ctx.hvi_paths_con(y, c, *lists, per_path=True)
            want, wu = baseline()
            emit({"kernel": "hvi_paths_con", "k": k, "c": c, "S": S, "front": P, "boxes": int(off[-1]), "N": N,
                  "feasible_pairs": float((y[k:] <= 0).all(0).double().mean()),
                  "values_bitwise_equal": bool(torch.equal(got, want) and torch.equal(gu, wu))}, res)
            del y, out, ts
    ctx.close()


def chain():
    ctx = AcqContext(0)
    dev = ctx.device
    S, d, m, k = 16, 6, 1024, 2
    for n in (128, 512):
        rng = np.random.default_rng(n + d)
        sts = states(ctx, n, d, k + 2, rng)
        for o, st in enumerate(sts):
            ctx.paths_set(o, *paths.draw_path_inputs("matern52", n, d, S, m, rng, np.zeros(d), np.ones(d), st.lengthscale),
                          noise=1e-6)
        Xt = torch.as_tensor(sts[0].X, device=dev)
        F = ctx.paths_eval(Xt, k + 2).cpu().numpy()
        r = np.stack([st.y.reshape(-1) for st in sts[:k]], 1).max(0) + 0.1
        for N in (1 << 16, 1 << 20):
            Xc = torch.as_tensor(np.random.default_rng(N).uniform(0.0, 1.0, (N, d)), device=dev)
            vals = torch.empty(N, dtype=torch.float64, device=dev)
            res, shape = {}, {}
            for c in (0, 1, 2):
                G = F[k:k + c] - np.median(F[k:k + c]) if c else F[k:k]      # about half of the rows feasible per slot
                lists = pareto.pack_box_lists(pareto.feasible_fronts(F[:k], G, r)[1]) if c else pareto.pack_box_lists(
                    [pareto.box_decomposition(pareto.calc_pf(np.ascontiguousarray(F[:k, s, :].T)), r) for s in range(S)])
                yb = torch.empty((k + c, S, N), dtype=torch.float64, device=dev)
                ctx.paths_eval(Xc, k + c, out=yb)
                ctx.plan_hvi_paths_con(c, *lists)
                a = ctx.eval(Xc).clone()
                b = ctx.hvi_paths_con(yb, c, *lists)
                shape[f"c{c}_boxes"] = int(lists[1][-1])
                shape[f"c{c}_chain_equals_stages"] = bool(torch.equal(a, b))
                shape[f"c{c}_feasible_pairs"] = float((yb[k:] <= 0).all(0).double().mean())
                res.update(alternate([(f"omb_eval(plan_hvi_paths_con), c = {c}", lambda: ctx.eval(Xc, out=vals)),
                                      (f"omb_paths_eval, {k + c} slots", lambda: ctx.paths_eval(Xc, k + c, out=yb)),
                                      (f"omb_hvi_paths_con, c = {c}", lambda: ctx.hvi_paths_con(yb, c, *lists, out=vals))]))
                del yb
            emit(dict({"chain": "nehvi_con", "n": n, "d": d, "m": m, "k": k, "S": S, "N": N}, **shape), res)
            del Xc, vals
    ctx.close()


def skip():
    ctx = AcqContext(0)
    dev = ctx.device
    k, c, S, P, N = 2, 1, 16, 50, 1 << 20
    rng = np.random.default_rng(7)
    lists = lists_for(k, S, P, rng)
    f = rng.uniform(-0.2, 1.3, (k, S, N))
    out = torch.empty(N, dtype=torch.float64, device=dev)
    for frac in (0.01, 0.5, 1.0):
        for layout in ("runs of 64", "scattered"):
            if layout == "runs of 64":
                ok = np.repeat(rng.uniform(size=N // 64) < frac, 64)
            else:
                ok = rng.uniform(size=N) < frac
            g = np.where(ok, -1.0, 1.0)[None, None, :] * np.ones((1, S, 1))
            y = torch.as_tensor(np.concatenate([f, g]), device=dev)
            res = alternate([("omb_hvi_paths (objectives alone)", lambda: ctx.hvi_paths(y[:k], *lists, out=out)),
                             ("omb_hvi_paths_con", lambda: ctx.hvi_paths_con(y, c, *lists, out=out)),
                             ("omb_hvi_paths_con, violation score",
                              lambda: ctx.hvi_paths_con(y, c, *lists, violation=True, out=out))])
            waves = ok.reshape(-1, 64).any(1).mean()
            emit({"kernel": "hvi_paths_con skip", "k": k, "c": c, "S": S, "front": P, "boxes": int(lists[1][-1]), "N": N,
                  "feasible": float(ok.mean()), "layout": layout, "wavefronts_with_a_feasible_lane": float(waves)}, res)
            del y
    ctx.close()


def drivers(seeds, budget):
    import optimobo_amd.algorithms.optimisers as opti
    from optimobo_amd.problem import ElementwiseProblem

    def clean(x):
        return np.array([(x[0] - 0.2) ** 2 + 2.0 * (x[1] - 0.1) ** 2, 1.5 * (x[0] - 0.9) ** 2 + (x[1] - 0.9) ** 2])

    span = np.array([2.26, 1.62])       # the objectives' ranges over the box [0, 1]^2
    ref = np.array([2.5, 2.0])

    class Noisy(ElementwiseProblem):
        def __init__(self, rel, seed):
            super().__init__(n_var=2, n_obj=2, n_ieq_constr=1, xl=np.zeros(2), xu=np.ones(2))
            self.sd = rel * span
            self.rng = np.random.default_rng(seed)

        def _evaluate(self, x, out, *a, **k):
            out["F"] = list(clean(x) + self.sd * self.rng.standard_normal(2))

        def _evaluate_constraints(self, x, out, *a, **k):
            out["G"] = [1.5 - x[0] - x[1]]

    variants = {"pof + exact EHVI": dict(constraints="pof"),
                "paths + nehvi": dict(constraints="paths", acquisition="nehvi")}

    def run(name, rel, seed):
        np.random.seed(seed)
        opt = opti.MultiSurrogateOptimiser(Noisy(rel, seed), [0, 0], list(ref), seed=seed + 1, mode="textbook",
                                           noise="fit", **variants[name])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res = opt.solve(budget=budget, n_init_samples=12)
        X = res.Xsample
        feas = 1.5 - X[:, 0] - X[:, 1] <= 0
        hv = pareto.hypervolume(np.array([clean(x) for x in X[feas]]).reshape(-1, 2), ref) if feas.any() else 0.0
        return [int(feas[12:].sum()), float(hv)]

    for rel in (0.01, 0.05):
        t = {k: [] for k in variants}
        for seed in range(-1, seeds):          # seed −1 is the warm-up round
            for name in variants:
                r = run(name, rel, max(seed, 0))
                if seed >= 0:
                    t[name].append(r)
        for name, v in t.items():
            a = np.array(v)
            print(json.dumps({"variant": name, "noise_sd_of_range": rel, "budget": budget, "n_init": 12, "seeds": seeds,
                              "feasible_proposals": [int(x) for x in a[:, 0]],
                              "median_feasible_proposals": float(np.median(a[:, 0])),
                              "noise_free_feasible_hypervolume": [float(x) for x in a[:, 1]],
                              "median_noise_free_feasible_hypervolume": float(np.median(a[:, 1]))}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--chain-only", action="store_true")
    ap.add_argument("--skip-only", action="store_true")
    ap.add_argument("--drivers-only", action="store_true")
    ap.add_argument("--seeds", type=int, default=5)
    ap.add_argument("--budget", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("nehvi_con_timing needs the GPU: a CPU run measures nothing")
    only = args.kernels_only or args.chain_only or args.skip_only or args.drivers_only
    if args.kernels_only or not only:
        kernels()
    if args.chain_only or not only:
        chain()
    if args.skip_only or not only:
        skip()
    if args.drivers_only or not only:
        drivers(args.seeds, args.budget)


if __name__ == "__main__":
    main()
