"""The arg-max chain's two-phase path at the bench's config 3: n_train 512, n_var 6, 2^20 Sobol candidates,
reference-mode EHVI-2D.

    python tools/argmax_prune_timing.py [--log2-cand 20]

One JSON line per plan, the dense chain ("argmax_prune" = 0) and the two-phase path (2) alternated in one process
(tools/logacq_timing.py's ``alternate``: device events around back-to-back calls, medians of its repeats), with the
seed and survivor counts of omb_argmax_prune_stats and whether the two pairs are bitwise equal:
  * "bench": the bench's own plan (its front, reference point and cache statistics);
  * "no-prune": a one-point front and reference point far below every posterior mean, so every value is 0, the
    seed's best value is 0 and the bound may drop nothing — the path's worst case, every candidate evaluated in full
    on top of the means, the bound and the compaction.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))

import bench  # noqa: E402
from logacq_timing import alternate  # noqa: E402
from optimobo_amd import pareto  # noqa: E402
from optimobo_amd.device import AcqContext  # noqa: E402
from optimobo_amd.gp import GPState  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-cand", type=int, default=20)
    args = ap.parse_args()
    cfg = bench.CONFIGS[3]
    n, d, N = cfg["n"], cfg["d"], 1 << args.log2_cand
    X, Y, ls, variances = bench.setup_problem(n, d, problem=cfg["problem"], tail_hi=cfg["tail_hi"])
    ctx = AcqContext(0)
    for o in range(2):
        ctx.set_gp_state(o, GPState(X, Y[:, o], ls, variances[o]))
    pf = pareto.calc_pf(Y)
    r = Y.max(axis=0) + 0.1 * (Y.max(axis=0) - Y.min(axis=0))
    s00, s01 = pareto.cache_stats(pareto.cached_samples(2, 5, seed=1))
    Xc = torch.as_tensor(bench.candidates(d, 0, N), device="cuda:0")
    out = torch.empty(2, dtype=torch.float64, device="cuda:0")
    plans = {"bench": (pareto.stripes_2d(pf), r),
             "no-prune": (np.array([[-101.0, -101.0]]), np.array([-100.0, -100.0]))}
    for name, (stripes, ref) in plans.items():
        ctx.plan_ehvi2d(stripes, ref, s00, s01, mode="reference")
        pairs, stats = {}, {}
        for mode in (0, 2):
            ctx.debug_set("argmax_prune", mode)
            pairs[mode] = ctx.eval_argmax(Xc).cpu().numpy()
            ctx.synchronize()
            stats[mode] = ctx.argmax_prune_stats()

        def run(mode):
            def fn():
                ctx.debug_set("argmax_prune", mode)
                ctx.eval_argmax(Xc, out=out)
            return fn

        res = alternate([("dense", run(0)), ("two-phase", run(2))])
        ctx.debug_set("argmax_prune", 1)
        row = {"plan": name, "n_train": n, "n_var": d, "N": N, "seed": stats[2][1], "survivors": stats[2][2],
               "survivor_share": stats[2][2] / N, "pair": [float(pairs[0][0]), int(pairs[0][1])],
               "pair_bitwise_equal": bool(np.array_equal(pairs[0].view(np.int64), pairs[2].view(np.int64)))}
        for k, (launches, us) in res.items():
            row[k + "_ms_median"] = float(np.median(us)) / 1e3
            row[k + "_ms"] = [round(u / 1e3, 4) for u in us]
            row[k + "_calls_per_repeat"] = launches
        print(json.dumps(row), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
