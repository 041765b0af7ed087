"""Objective 1's bound as one cut at the bench's config 3: n_train 512, n_var 6, 2^20 Sobol candidates,
reference-mode EHVI-2D.

    python tools/argmax_cut_timing.py [--log2-cand 20] [--out profiles/argmax_cut_timing_mi355x.jsonl]

One JSON line per plan, printed and written to --out: the dense chain ("argmax_prune" 0), §31's order
("argmax_staged" 0), the staged order with the bound per candidate ("argmax_cut" 0) and with the cut ("argmax_cut" 1)
alternated in one process (tools/logacq_timing.py's ``alternate``: device events around back-to-back calls, medians of
its 7 repeats), with the list sizes of omb_argmax_stage_stats under both forms, the cut of omb_argmax_cut_stats and
whether the four pairs are bitwise equal.  The plans are tools/argmax_staged_timing.py's: "bench", "no-prune" (τ₀ = 0:
no cut, everything kept) and "swapped" (list A keeps most of the batch).
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

# ("argmax_prune", "argmax_staged", "argmax_cut")
MODES = {"dense": (0, 1, 1), "staged0": (1, 0, 1), "cut0": (1, 1, 0), "cut1": (1, 1, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-cand", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "argmax_cut_timing_mi355x.jsonl"))
    args = ap.parse_args()
    cfg = bench.CONFIGS[3]
    n, d, N = cfg["n"], cfg["d"], 1 << args.log2_cand
    X, Y, ls, variances = bench.setup_problem(n, d, problem=cfg["problem"], tail_hi=cfg["tail_hi"])
    ctx = AcqContext(0)
    states = [GPState(X, Y[:, o], ls, variances[o]) for o in range(2)]
    s00, s01 = pareto.cache_stats(pareto.cached_samples(2, 5, seed=1))
    Xc = torch.as_tensor(bench.candidates(d, 0, N), device="cuda:0")
    out = torch.empty(2, dtype=torch.float64, device="cuda:0")

    def front(Yv):
        return pareto.stripes_2d(pareto.calc_pf(Yv)), Yv.max(axis=0) + 0.1 * (Yv.max(axis=0) - Yv.min(axis=0))

    plans = {"bench": (states,) + front(Y),
             "no-prune": (states, np.array([[-101.0, -101.0]]), np.array([-100.0, -100.0])),
             "swapped": (states[::-1],) + front(np.ascontiguousarray(Y[:, ::-1]))}
    rows = []
    for name, (sts, stripes, ref) in plans.items():
        for o, st in enumerate(sts):
            ctx.set_gp_state(o, st)
        ctx.plan_ehvi2d(stripes, ref, s00, s01, mode="reference")

        def select(v):
            ctx.debug_set("argmax_prune", v[0])
            ctx.debug_set("argmax_staged", v[1])
            ctx.debug_set("argmax_cut", v[2])

        pairs, stages, cuts = {}, {}, {}
        for mode, v in MODES.items():
            select(v)
            pairs[mode] = ctx.eval_argmax(Xc).cpu().numpy()
            ctx.synchronize()
            stages[mode] = ctx.argmax_stage_stats()
            cuts[mode] = ctx.argmax_cut_stats()

        def run(v):
            def fn():
                select(v)
                ctx.eval_argmax(Xc, out=out)
            return fn

        res = alternate([(mode, run(v)) for mode, v in MODES.items()])
        select(MODES["cut1"])
        bits = [pairs[m].view(np.int64) for m in MODES]
        c = cuts["cut1"]
        row = {"plan": name, "n_train": n, "n_var": d, "N": N,
               "cut_taken": [bool(cuts[m][0]) for m in MODES],
               "list_a_cut0": stages["cut0"][1], "list_b_cut0": stages["cut0"][2],
               "list_a_cut1": stages["cut1"][1], "list_b_cut1": stages["cut1"][2],
               "m_star": c[1] if np.isfinite(c[1]) else "inf", "tau0": c[2], "ubm1_at_m_star": None if np.isnan(c[3]) else c[3],
               "pair": [float(pairs["dense"][0]), int(pairs["dense"][1])],
               "pairs_bitwise_equal": bool(all(np.array_equal(bits[0], b) for b in bits[1:]))}
        for k, (launches, us) in res.items():
            row[k + "_ms_median"] = float(np.median(us)) / 1e3
            row[k + "_ms"] = [round(u / 1e3, 4) for u in us]
            row[k + "_calls_per_repeat"] = launches
        print(json.dumps(row), flush=True)
        rows.append(row)
    ctx.close()
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
