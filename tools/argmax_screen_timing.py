"""The arg-max chain's fp32 screen at the bench's config 3: n_train 512, n_var 6, 2^20 Sobol candidates,
reference-mode EHVI-2D.

    python tools/argmax_screen_timing.py [--log2-cand 20]

One JSON line per plan: the dense chain ("argmax_prune" 0), the two-phase path on fp64 means ("argmax_screen" 0) and
on the screen (1) alternated in one process (tools/logacq_timing.py's ``alternate``: device events around
back-to-back calls, medians of its repeats), with the survivor counts of both paths and whether the three pairs are
bitwise equal; then one line for omb_posterior_screen over the same batch: its time and its largest |μ̃ − μ| / ε
against omb_posterior's μ.
  * "bench": the bench's own plan;
  * "no-prune": a one-point front and reference point far below every posterior mean — τ = 0, nothing is dropped, the
    worst case of either path.
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

MODES = {"dense": (0, 1), "fp64-means": (2, 0), "screen": (2, 1)}


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

    def switch(mode):
        ctx.debug_set("argmax_prune", MODES[mode][0])
        ctx.debug_set("argmax_screen", MODES[mode][1])

    plans = {"bench": (pareto.stripes_2d(pf), r),
             "no-prune": (np.array([[-101.0, -101.0]]), np.array([-100.0, -100.0]))}
    for name, (stripes, ref) in plans.items():
        ctx.plan_ehvi2d(stripes, ref, s00, s01, mode="reference")
        pairs, stats = {}, {}
        for mode in MODES:
            switch(mode)
            pairs[mode] = ctx.eval_argmax(Xc).cpu().numpy()
            ctx.synchronize()
            stats[mode] = ctx.argmax_prune_stats()

        def run(mode):
            def fn():
                switch(mode)
                ctx.eval_argmax(Xc, out=out)
            return fn

        res = alternate([(mode, run(mode)) for mode in MODES])
        switch("dense")
        ctx.debug_set("argmax_prune", 1)
        bits = [pairs[m].view(np.int64) for m in MODES]
        row = {"plan": name, "n_train": n, "n_var": d, "N": N, "seed": stats["screen"][1],
               "survivors_fp64_means": stats["fp64-means"][2], "survivors_screen": stats["screen"][2],
               "pair": [float(pairs["dense"][0]), int(pairs["dense"][1])],
               "pairs_bitwise_equal": bool(np.array_equal(bits[0], bits[1]) and np.array_equal(bits[0], bits[2]))}
        for k, (launches, us) in res.items():
            row[k + "_ms_median"] = float(np.median(us)) / 1e3
            row[k + "_ms"] = [round(u / 1e3, 4) for u in us]
            row[k + "_calls_per_repeat"] = launches
        print(json.dumps(row), flush=True)

    mu, var = ctx.posterior(Xc, n_obj=2)
    mt, eps = ctx.posterior_screen(Xc, n_obj=2)
    ctx.synchronize()
    ratio = ((mt - mu).abs() / eps).max().item()
    scr = torch.empty_like(mt), torch.empty_like(eps)
    res = alternate([("posterior_screen", lambda: ctx.posterior_screen(Xc, n_obj=2, out=scr))])
    row = {"entry": "omb_posterior_screen", "N": N, "max_err_over_eps": ratio,
           "max_eps": [float(v) for v in eps.max(1).values.cpu().numpy()],
           "max_err": [float(v) for v in (mt - mu).abs().max(1).values.cpu().numpy()]}
    for k, (launches, us) in res.items():
        row[k + "_ms_median"] = float(np.median(us)) / 1e3
        row[k + "_ms"] = [round(u / 1e3, 4) for u in us]
    print(json.dumps(row), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
