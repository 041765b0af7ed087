"""Per-launch time of omb_paths_eval (paths_eval_kernel) and of omb_paths_set, with the kernel's own cosine and with
the device library's.

Run on the GPU box: python tools/paths_timing.py > profiles/paths_timing_mi355x.jsonl
States (n, d, m, k) = (128, 6, 1024, 2), (512, 6, 1024, 2), (1024, 30, 2048, 1), S = 16 paths, Matern-5/2, at
N = 2^16, 2^18, 2^20 candidates.  Timed as tools/hvi_timing.py times (device events around back-to-back launches after
a warm-up by time).  Each line: the shape, the variant, µs per launch of every repeat, their median and spread, and the
implied instruction rates against DESIGN §4's figures, which share one pipe:
  valu_tflops   2 flops × (27 fp64 VALU instructions per feature and candidate — the cosine — plus 22 per training row
                and candidate — the Matern transform) per second, against 60 TFLOP/s;
  mfma_tflops   2048 flops per v_mfma_f64_16x16x4_f64: per 16 × 16 tile ⌈(d+1)/4⌉ + 4 for features,
                ⌈(d+2)/4⌉ (n_var ≤ 8) or ⌈d/4⌉ + 4 for training rows, against 70.3 TFLOP/s;
  pipe_share    valu_tflops / 60 + mfma_tflops / 70.3.
omb_paths_set is timed by wall clock around the call and a synchronise (it packs on the host and uploads).
"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from ehvi_boxes_timing import time_variant  # noqa: E402

from optimobo_amd import paths  # noqa: E402
from optimobo_amd.device import AcqContext  # noqa: E402
from optimobo_amd.gp import GPState  # noqa: E402

COS_INSTR, MATERN_INSTR = 27, 22


def pad_dim(d):
    return next(p for p in (2, 4, 6, 8, 16, 32, 64) if d <= p)


def main():
    ctx = AcqContext(0)
    dev = ctx.device
    S = 16
    for n, d, m, k in [(128, 6, 1024, 2), (512, 6, 1024, 2), (1024, 30, 2048, 1)]:
        rng = np.random.default_rng(n + d)
        X = rng.uniform(0.0, 1.0, (n, d))
        draws = []
        for o in range(k):
            y = np.sin(3.0 * X + o).sum(1)
            st = GPState(X, y, rng.uniform(0.3, 1.2, d) * np.sqrt(d), float(np.var(y) + 0.1), noise=1e-6)
            ctx.set_gp(o, st.X, st.lengthscale, st.variance, st.alpha, st.Linv)
            draws.append(paths.draw_path_inputs("matern52", n, d, S, m, rng, np.zeros(d), np.ones(d), st.lengthscale))
        DP = pad_dim(d)
        ft, rt = (m + 15) // 16, (n + 15) // 16
        mf_feat = (DP + 4) // 4 + 4
        mf_row = ((DP + 5) // 4 if DP <= 8 else (DP + 3) // 4) + 4
        first = None
        for libcos in (0, 1):
            ctx.debug_set("paths_libcos", libcos)
            set_ms = []
            for _ in range(5):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for o, (omega, phase, w, z) in enumerate(draws):
                    ctx.paths_set(o, omega, phase, w, z, noise=1e-6)
                torch.cuda.synchronize()
                set_ms.append((time.perf_counter() - t0) * 1e3 / k)
            for N in (1 << 16, 1 << 18, 1 << 20):
                Xc = torch.as_tensor(np.random.default_rng(N).uniform(0.0, 1.0, (N, d)), device=dev)
                out = torch.empty((k, S, N), dtype=torch.float64, device=dev)
                launches, us = time_variant(ctx, lambda: ctx.paths_eval(Xc, k, out=out))
                med = float(np.median(us))
                tiles = k * (N / 16)
                valu = 2.0 * k * N * (16 * ft * COS_INSTR + 16 * rt * MATERN_INSTR) / med * 1e-6
                mfma = 2048.0 * tiles * (ft * mf_feat + rt * mf_row) / med * 1e-6
                row = {"n": n, "d": d, "m": m, "k": k, "S": S, "N": N,
                       "variant": "library_cos" if libcos else "kernel_cos", "launches_per_repeat": launches,
                       "us_per_launch": [round(u, 2) for u in us], "median_us": round(med, 2),
                       "spread": round((max(us) - min(us)) / med, 4), "valu_tflops": round(valu, 2),
                       "mfma_tflops": round(mfma, 2), "pipe_share": round(valu / 60.0 + mfma / 70.3, 3),
                       "paths_set_ms_per_objective": round(float(np.median(set_ms)), 3)}
                if N == 1 << 16:
                    vals = out.cpu().numpy()
                    first = vals if first is None else first
                    row["max_diff_vs_kernel_cos"] = float(np.abs(vals - first).max())
                print(json.dumps(row), flush=True)
        ctx.debug_set("paths_libcos", 0)
    ctx.close()


if __name__ == "__main__":
    main()
