"""Per-launch time of the log-space acquisition kernels beside the linear kernels they stand in for.

Run on the GPU box: python tools/logacq_timing.py > logacq_timing.jsonl
Each pair alternates in one process — linear, log, linear, log, … — after a warm-up of both, timed by device events
around back-to-back launches (about 30 ms per timed repeat, at least one launch):
  * omb_ei against omb_log_ei at 2^20 candidates (moments: γ uniform over [−60, 5], σ² log-uniform over 1e-12 … 1);
  * omb_ehvi_boxes_k against omb_log_ehvi_boxes on the fronts of tools/hvi_timing.py — (k 2, 60 points),
    (k 4, 60 points), (k 6, 30 points): 61, 6,808 and 99,484 boxes — at N = 64·3000 = 192,000 candidates, front
    points plus 0.15·N(0, 1) with σ log-uniform over 1e-3 … 0.3.
Each line: the shape, the variant, µs per launch of every repeat, their median and spread, the share of candidates
whose linear value is exactly 0, and for the log variant its median over the linear one's.
"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from ehvi_boxes_timing import sphere_front  # noqa: E402

from optimobo_amd import pareto  # noqa: E402
from optimobo_amd.device import AcqContext  # noqa: E402

REPEATS = 7


def alternate(runs):
    """runs: [(name, fn)] → {name: (launches, [µs per launch] · REPEATS)}, the variants taking turns."""
    launches = {}
    for name, fn in runs:
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        one = max(time.perf_counter() - t0, 1e-5)
        for _ in range(max(1, min(200, int(0.1 / one)))):      # warm-up
            fn()
        torch.cuda.synchronize()
        launches[name] = max(1, min(200, int(0.03 / one)))
    us = {name: [] for name, _ in runs}
    for _ in range(REPEATS):
        for name, fn in runs:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(launches[name]):
                fn()
            b.record()
            b.synchronize()
            us[name].append(a.elapsed_time(b) * 1e3 / launches[name])
    return {name: (launches[name], us[name]) for name, _ in runs}


def report(shape, res, zero_share):
    base = None
    for name, (launches, us) in res.items():
        med = float(np.median(us))
        base = med if base is None else base
        row = dict(shape, variant=name, launches_per_repeat=launches, us_per_launch=[round(u, 2) for u in us],
                   median_us=round(med, 2), spread=round((max(us) - min(us)) / med, 4),
                   linear_exactly_zero=round(zero_share, 4), over_linear=round(med / base, 2))
        print(json.dumps(row), flush=True)


def main():
    ctx = AcqContext(0)
    dev = ctx.device
    rng = np.random.default_rng(0)
    N = 1 << 20
    sd = 10.0 ** rng.uniform(-6, 0, N)
    mu = torch.as_tensor(0.3 - rng.uniform(-60, 5, N) * sd, device=dev)
    var = torch.as_tensor(sd * sd, device=dev)
    out = torch.empty(N, dtype=torch.float64, device=dev)
    res = alternate([("omb_ei", lambda: ctx.ei(mu, var, 0.3, out=out)),
                     ("omb_log_ei", lambda: ctx.log_ei(mu, var, 0.3, out=out))])
    report({"kernel": "ei", "N": N}, res, float((ctx.ei(mu, var, 0.3) == 0).double().mean()))
    N = 64 * 3000
    for k, P in [(2, 60), (4, 60), (6, 30)]:
        rng, pf = sphere_front(k, P, 10 * k + P, 40 * P)
        coords, _, boxes = pareto.box_decomposition(pf, np.full(k, 1.2))
        cd = torch.as_tensor(coords, device=dev)
        bd = torch.as_tensor(boxes.view(np.int16), device=dev)
        m = torch.as_tensor((pf[rng.integers(0, len(pf), N)] + 0.15 * rng.standard_normal((N, k))).T.copy(), device=dev)
        v = torch.as_tensor((10.0 ** rng.uniform(-3, -0.5, (k, N))) ** 2, device=dev)
        out = torch.empty(N, dtype=torch.float64, device=dev)
        res = alternate([("omb_ehvi_boxes_k", lambda: ctx.ehvi_boxes(m, v, cd, bd, out=out, kd=True)),
                         ("omb_log_ehvi_boxes", lambda: ctx.log_ehvi_boxes(m, v, cd, bd, out=out))])
        lin = ctx.ehvi_boxes(m, v, cd, bd, kd=True)
        report({"kernel": "ehvi_boxes", "k": k, "P": len(pf), "N": N, "B": len(boxes), "C": coords.shape[1]}, res,
               float((lin == 0).double().mean()))
    ctx.close()


if __name__ == "__main__":
    main()
