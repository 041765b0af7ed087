"""Times what inequality constraints add to the fused chain (omb_plan_constraints) and omb_feasibility alone.

    python tools/constraint_timing.py [--out FILE] [--log2-cand 20] [--repeats R]

The shape is bench.py's config 3: n_train 512, n_var 6, two ZDT1 objectives, 2^20 unscrambled Sobol candidates,
reference EHVI-2D, cache seed 1.  The constraint models are GPs of g₁ = x₀ + x₁ − 1 and g₂ = 0.3 − x₁ on the same
inputs and lengthscales.
  chain_c0/1/2      one ctx.eval_argmax (posterior → EHVI → [weight] → arg-max) with 0, 1, 2 constraints;
  feasibility_c1/2  ctx.feasibility on resident moments, in place on a resident acquisition vector.
The variants alternate within every repeat after two warm-up rounds; each is timed with device events around the one
call.  One JSON line per variant: the median and the min-max spread in milliseconds; for the chain also the stage
split of omb_timing (posterior / acquisition, the weight's launch inside the latter) and for omb_feasibility the
bytes it must move, (2c + 2)·8·N, over the median.
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--log2-cand", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=20)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("constraint_timing needs the GPU: a CPU run measures nothing")
    import bench
    from optimobo_amd import pareto
    from optimobo_amd.device import AcqContext
    from optimobo_amd.gp import GPState

    cfg = bench.CONFIGS[3]
    n, d, N = cfg["n"], cfg["d"], 1 << args.log2_cand
    X, Y, ls, variances = bench.setup_problem(n, d, problem=cfg["problem"], tail_hi=cfg["tail_hi"])
    G = np.column_stack([X[:, 0] + X[:, 1] - 1.0, 0.3 - X[:, 1]])
    pf = pareto.calc_pf(Y)
    r = Y.max(axis=0) + 0.1 * (Y.max(axis=0) - Y.min(axis=0))
    s00, s01 = pareto.cache_stats(pareto.cached_samples(2, 5, seed=1))
    ctx = AcqContext(0)
    for o in range(2):
        ctx.set_gp_state(o, GPState(X, Y[:, o], ls, variances[o]))
    for j in range(2):
        ctx.set_gp_state(2 + j, GPState(X, G[:, j], ls, float(np.var(G[:, j]))))
    Xc = torch.as_tensor(bench.candidates(d, 0, N), device=ctx.device)
    pair = torch.empty(2, dtype=torch.float64, device=ctx.device)
    mu, var = ctx.posterior(Xc, 4)
    acq = torch.rand(N, dtype=torch.float64, device=ctx.device)
    out = torch.empty_like(acq)

    def plan(c):
        ctx.plan_ehvi2d(pareto.stripes_2d(pf), r, s00, s01, mode="reference")
        if c:
            ctx.plan_constraints(c, 1e-5)

    def chain(c):
        return lambda: ctx.eval_argmax(Xc, offset=0, out=pair)

    def feas(c):
        return lambda: ctx.feasibility(mu[2:2 + c], var[2:2 + c], 1e-5, acq=acq, out=out)

    variants = [(f"chain_c{c}", c, chain(c)) for c in (0, 1, 2)] + [(f"feasibility_c{c}", c, feas(c)) for c in (1, 2)]
    t = {name: [] for name, _, _ in variants}
    stages = {name: [] for name, _, _ in variants if name.startswith("chain")}
    pairs = {}
    for rep in range(2 + args.repeats):
        for name, c, fn in variants:
            is_chain = name.startswith("chain")
            if is_chain:
                plan(c)
                ctx.timing(2)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if is_chain:
                st = ctx.timing_read()
                ctx.timing(0)
                pairs[name] = pair.cpu().numpy().tolist()
            if rep >= 2:
                t[name].append(e0.elapsed_time(e1))
                if is_chain:
                    stages[name].append([st[0][k] for k in ("sobol", "posterior", "acquisition", "argmax")])
    rows = []
    for name, c, _ in variants:
        v = np.array(t[name])
        row = {"variant": name, "constraints": c, "n_train": n, "n_var": d, "candidates": N, "repeats": args.repeats,
               "ms": {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max())}}
        if name in stages:
            s = np.median(np.array(stages[name], dtype=np.float64), axis=0)
            row["stage_ms_median"] = {"sobol": float(s[0]), "posterior": float(s[1]), "acquisition": float(s[2]),
                                      "argmax": float(s[3])}
            row["pair"] = pairs[name]
        else:
            nbytes = (2 * c + 2) * 8 * N
            row["bytes"] = nbytes
            row["gb_per_s_at_median"] = nbytes / (np.median(v) * 1e-3) / 1e9
        rows.append(row)
        print(json.dumps(row), flush=True)
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
