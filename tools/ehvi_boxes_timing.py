"""Per-launch time of the exact-EHVI kernels at k ≥ 4 (and k = 3): omb_ehvi_boxes_k candidate-blocked
(ehvi_boxes_kd_kernel) against its one-wavefront-per-candidate baseline (OMB_DEBUG_BOXES_KD = 1), and at k = 3
against omb_ehvi_boxes.

Run on the GPU box: python tools/ehvi_boxes_timing.py > ehvi_boxes_timing.jsonl (or as a `py` step of tools/gpu.sh)
The acquisition kernel alone (moments already on the device), timed by device events around a run of back-to-back
launches; each variant is warmed up for ≥ 0.2 s first (the clocks need that long to settle), then
timed REPEATS times.  Each line: the shape, B, C, the variant, µs per launch of every repeat, their median and
spread (max − min) / median, and the largest difference from the first variant's values over their maximum.
"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from optimobo_amd import pareto  # noqa: E402
from optimobo_amd.device import AcqContext  # noqa: E402

REPEATS = 7


def sphere_front(k, P, seed, oversample):
    rng = np.random.default_rng(seed)
    pts = rng.uniform(0.05, 1, (oversample, k))
    pts /= np.linalg.norm(pts, axis=1, keepdims=True)
    return rng, pareto.calc_pf(pts)[:P]


def time_variant(ctx, run):
    run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run()
    torch.cuda.synchronize()
    one = max(time.perf_counter() - t0, 1e-5)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.25:                 # warm-up by time
        for _ in range(max(1, int(0.02 / one))):
            run()
        torch.cuda.synchronize()
    launches = max(3, min(200, int(0.03 / one)))           # ≈ 30 ms per timed repeat
    us = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            run()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / launches)
    return launches, us


def main():
    ctx = AcqContext(0)
    dev = ctx.device
    shapes = [(4, 60, 1 << 16), (5, 50, 1 << 14), (6, 30, 1 << 14), (3, 250, 1 << 16)]
    for k, P, N in shapes:
        if k == 3:      # the 250-point front of test_exact_ehvi_large_box_list_from_global
            rng, pf = sphere_front(3, 250, 5, 3000)
        else:
            rng, pf = sphere_front(k, P, 10 * k + P, 40 * P)
        r = np.full(k, 1.2)
        t0 = time.perf_counter()
        coords, _, boxes = pareto.box_decomposition(pf, r)
        host_s = time.perf_counter() - t0
        mu = torch.as_tensor(rng.uniform(0.0, 1.3, (k, N)), device=dev)
        var = torch.as_tensor(10 ** rng.uniform(-5, -0.5, (k, N)), device=dev)
        cd = torch.as_tensor(coords, device=dev)
        bd = torch.as_tensor(boxes.view(np.int16), device=dev)
        out = torch.empty(N, dtype=torch.float64, device=dev)
        variants = [("wave_per_candidate", 1, True), ("candidate_blocked", 0, True)]
        if k == 3:
            variants.append(("omb_ehvi_boxes", 0, False))
        first = None
        for name, wave, kd in variants:
            ctx.debug_set("boxes_kd", wave)
            run = lambda: ctx.ehvi_boxes(mu, var, cd, bd, out=out, kd=kd)  # noqa: E731
            launches, us = time_variant(ctx, run)
            vals = out.cpu().numpy().copy()
            first = vals if first is None else first
            med = float(np.median(us))
            print(json.dumps({"k": k, "P": len(pf), "N": N, "B": len(boxes), "C": coords.shape[1],
                              "decomposition_s": round(host_s, 3), "variant": name, "launches_per_repeat": launches,
                              "us_per_launch": [round(u, 2) for u in us], "median_us": round(med, 2),
                              "spread": round((max(us) - min(us)) / med, 4),
                              "max_diff_vs_first_over_max": float(np.abs(vals - first).max() / np.abs(first).max())}),
                  flush=True)
        ctx.debug_set("boxes_kd", 0)
    ctx.close()


if __name__ == "__main__":
    main()
