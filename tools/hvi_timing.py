"""Per-launch time of omb_hvi_boxes (hvi_boxes_kernel) and of the closest thing the library had before it: the same
values from omb_ehvi_boxes_k with a vanishing variance.

Run on the GPU box: python tools/hvi_timing.py > hvi_timing.jsonl
Fronts as tools/ehvi_boxes_timing.py builds them (points on the unit sphere, r = 1.2): (k 2, 60 points), (k 4, 60
points), (k 6, 30 points), each at N = 64·3000 (a Thompson batch's q·N_c) and N = 2^20; the points are front points
plus 0.15·N(0, 1).  Timed as there (device events around back-to-back launches after a warm-up by time).  Each line:
the shape, B, C, the variant, µs per launch of every repeat, their median and spread, for omb_hvi_boxes the implied
fp64 rate at 4k flops per box and point (k subtractions, 2k maxima, k − 1 products and the accumulation), and for
the EHVI variant (N = 64·3000 only) its largest difference from the HVI values over their maximum.
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from ehvi_boxes_timing import sphere_front, time_variant  # noqa: E402

from optimobo_amd import pareto  # noqa: E402
from optimobo_amd.device import AcqContext  # noqa: E402


def main():
    ctx = AcqContext(0)
    dev = ctx.device
    for k, P in [(2, 60), (4, 60), (6, 30)]:
        rng, pf = sphere_front(k, P, 10 * k + P, 40 * P)
        coords, _, boxes = pareto.box_decomposition(pf, np.full(k, 1.2))
        cd = torch.as_tensor(coords, device=dev)
        bd = torch.as_tensor(boxes.view(np.int16), device=dev)
        for N in (64 * 3000, 1 << 20):
            y = torch.as_tensor((pf[rng.integers(0, len(pf), N)] + 0.15 * rng.standard_normal((N, k))).T.copy(),
                                device=dev)
            out = torch.empty(N, dtype=torch.float64, device=dev)
            variants = [("omb_hvi_boxes", lambda: ctx.hvi_boxes(y, cd, bd, out=out))]
            if N == 64 * 3000:
                var = torch.full_like(y, 1e-30)
                variants.append(("omb_ehvi_boxes_k_sigma_1e-15",
                                 lambda: ctx.ehvi_boxes(y, var, cd, bd, out=out, kd=True)))
            first = None
            for name, run in variants:
                launches, us = time_variant(ctx, run)
                vals = out.cpu().numpy().copy()
                first = vals if first is None else first
                med = float(np.median(us))
                row = {"k": k, "P": len(pf), "N": N, "B": len(boxes), "C": coords.shape[1], "variant": name,
                       "launches_per_repeat": launches, "us_per_launch": [round(u, 2) for u in us],
                       "median_us": round(med, 2), "spread": round((max(us) - min(us)) / med, 4),
                       "share_positive": float(np.mean(vals > 0)),
                       "max_diff_vs_first_over_max": float(np.abs(vals - first).max() / np.abs(first).max())}
                if name == "omb_hvi_boxes":
                    row["tflops_at_4k_per_box"] = round(4.0 * k * len(boxes) * N / med * 1e-6, 3)
                print(json.dumps(row), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
