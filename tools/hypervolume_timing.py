"""The exact hypervolume on the device: omb_hypervolume and omb_hypervolume_contrib against
``pareto.hypervolume`` on the same host and inputs, and one call just under the work cap.

    python tools/hypervolume_timing.py [--no-cap] [--cap-points 30]

Speed — unit-sphere fronts below the reference point 1.1 at (k, n) = (4, 60), (5, 50), (6, 30), (3, 1000): the device
entry (a synchronising call: device events around repeated calls after a warm-up by time, five repeats, median and
spread) and the host function (wall clock, one run where it takes longer than a second, else the median of three);
``omb_hypervolume_contrib`` at (5, 50) against n + 1 host calls.  Every row carries the values of both sides.

Cap — k = 8 with ``--cap-points`` rows in general position is n^6 cells × n point tests (30: 2.2e10, under
OMB_HV_MAX_WORK = 2^38 = 2.7e11), S sets of it the largest multiple under the cap: one call, wall clock with a
synchronise, after a warm-up call of one set.  One JSON row per line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))

from logacq_timing import alternate  # noqa: E402

import _hypervolume_reference as R  # noqa: E402
from optimobo_amd import _lib, pareto  # noqa: E402
from optimobo_amd.device import AcqContext  # noqa: E402


def emit(row):
    print(json.dumps(row), flush=True)


def wall(fn, budget_s=1.0):
    t = time.perf_counter()
    out = fn()
    first = time.perf_counter() - t
    if first > budget_s:
        return first, 1, out
    ts = [first]
    for _ in range(2):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)), 3, out


def speed(ctx):
    for k, n in ((4, 60), (5, 50), (6, 30), (3, 1000)):
        P = R.sphere(np.random.default_rng(100 * k + n), n, k)
        r = np.full(k, 1.1)
        Y = torch.as_tensor(np.ascontiguousarray(P.T), device=ctx.device)
        res = alternate([("omb_hypervolume", lambda: ctx.hypervolume(Y, r))])
        calls, us = res["omb_hypervolume"]
        host_s, host_runs, host = wall(lambda: pareto.hypervolume(P, r))
        dev = float(ctx.hypervolume(Y, r)[0])
        med = float(np.median(us))
        emit({"entry": "omb_hypervolume", "k": k, "n": n, "median_us": round(med, 1),
              "us_per_call": [round(u, 1) for u in us], "calls_per_repeat": calls,
              "spread": round((max(us) - min(us)) / med, 4), "host_s": round(host_s, 4), "host_runs": host_runs,
              "host_over_device": round(host_s * 1e6 / med, 1), "device_value": dev, "host_value": host,
              "relative_difference": abs(dev - host) / host})
    k, n = 5, 50
    P = R.sphere(np.random.default_rng(100 * k + n), n, k)
    r = np.full(k, 1.1)
    Y = torch.as_tensor(np.ascontiguousarray(P.T), device=ctx.device)
    res = alternate([("omb_hypervolume_contrib", lambda: ctx.hypervolume_contributions(Y, r))])
    calls, us = res["omb_hypervolume_contrib"]

    def host_contrib():
        full = pareto.hypervolume(P, r)
        return np.array([full - pareto.hypervolume(np.delete(P, i, axis=0), r) for i in range(n)])
    t = time.perf_counter()
    host = host_contrib()
    host_s = time.perf_counter() - t
    c = ctx.hypervolume_contributions(Y, r)[1].cpu().numpy()
    med = float(np.median(us))
    emit({"entry": "omb_hypervolume_contrib", "k": k, "n": n, "median_us": round(med, 1),
          "us_per_call": [round(u, 1) for u in us], "calls_per_repeat": calls,
          "spread": round((max(us) - min(us)) / med, 4), "host_s": round(host_s, 3), "host_runs": 1,
          "host_over_device": round(host_s * 1e6 / med, 1),
          "largest_difference_over_hv": float(np.max(np.abs(c - host)) / pareto.hypervolume(P, r)),
          "least_contributor": [int(np.argmin(c)), int(np.argmin(host))]})


def cap(ctx, n):
    k = 8
    per_set = n ** 7
    S = int(min(16, _lib.HV_MAX_WORK // per_set))
    if S < 1:
        sys.exit(f"{n} rows at k = 8 are above the cap on their own")
    P = R.sphere(np.random.default_rng(8), n, k)
    r = np.full(k, 1.1)
    one = torch.as_tensor(np.ascontiguousarray(P.T), device=ctx.device)
    Y = one[:, None, :].expand(k, S, n).contiguous()
    t = time.perf_counter()
    ctx.hypervolume(one, r)
    torch.cuda.synchronize()
    one_s = time.perf_counter() - t
    emit({"entry": "omb_hypervolume", "what": "one set, first call", "k": k, "n": n, "point_tests": per_set,
          "wall_s": round(one_s, 4)})
    for rep in range(2):
        t = time.perf_counter()
        hv = ctx.hypervolume(Y, r, S)
        torch.cuda.synchronize()
        s = time.perf_counter() - t
        emit({"entry": "omb_hypervolume", "what": "under the cap", "k": k, "n": n, "S": S, "point_tests": S * per_set,
              "cap": _lib.HV_MAX_WORK, "share_of_cap": round(S * per_set / _lib.HV_MAX_WORK, 3), "wall_s": round(s, 4),
              "point_tests_per_s": round(S * per_set / s, 0), "repeat": rep,
              "values_agree": bool((hv == hv[0]).all()), "value": float(hv[0])})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-cap", action="store_true")
    ap.add_argument("--cap-points", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("hypervolume_timing needs the GPU: a CPU run measures nothing")
    ctx = AcqContext(0)
    speed(ctx)
    if not args.no_cap:
        cap(ctx, args.cap_points)


if __name__ == "__main__":
    main()
