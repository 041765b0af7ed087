"""Times one Kriging-believer append (omb_gp_append) against what the library had to do before for the same
effect, and the drivers' batch_size on the README run.

    python tools/append_timing.py [--out FILE] [--sizes 128,512,1024,4096] [--repeats R] [--skip-solve]

Per n (d = 6, 2 objectives, Matern-5/2), the state of n points installed, one more point conditioned on:
  append        ctx.gp_append(o, x) for both objectives (synchronises);
  host_refit    a host GPState on the n + 1 points (Cholesky, explicit inverse: O(n³)) and set_gp_state (n² upload),
                for both objectives, then a synchronise — the only route before omb_gp_append for a host state;
  device_refit  ctx.gp_fit_state on the n + 1 points for both objectives (device O(n³)).
The three variants alternate within every repeat after two warm-up rounds; the installed state is put back (not
timed) before each.  Wall clock around work that ends in a synchronise.  One JSON line per n: the median and the
min-max spread in milliseconds.
Then ``MultiSurrogateOptimiser.solve`` on the README run (Tchebicheff expected decomposition, n_init 20) at
batch_size 1 and 4: wall seconds per true evaluation, alternating, with the fit / maximise split.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def case(n, d, seed=0):
    rng = np.random.default_rng(seed + n)
    X = rng.uniform(0.0, 1.0, (n + 1, d))
    ls = rng.uniform(0.3, 1.0, d) * np.sqrt(d)
    Y = np.column_stack([np.sin(3.0 * X).sum(1), np.cos(2.0 * X).prod(1)])
    return X, Y, ls, [1.7, 0.9]


def time_appends(sizes, repeats, d=6):
    import torch
    from optimobo_amd.device import AcqContext
    from optimobo_amd.gp import GPState
    ctx = AcqContext(0)
    rows = []
    for n in sizes:
        X, Y, ls, var = case(n, d)
        base = [GPState(X[:n], Y[:n, o], ls, var[o]) for o in range(2)]
        Xd, xnew = torch.as_tensor(X, device=ctx.device), torch.as_tensor(X[n:], device=ctx.device)
        Yd = [torch.as_tensor(np.ascontiguousarray(Y[:, o]), device=ctx.device) for o in range(2)]

        def restore():
            for o in range(2):
                ctx.set_gp_state(o, base[o])
            ctx.synchronize()

        def append():
            for o in range(2):
                ctx.gp_append(o, xnew, None, 0.0)

        def host_refit():
            for o in range(2):
                ctx.set_gp_state(o, GPState(X, Y[:, o], ls, var[o]))
            ctx.synchronize()

        def device_refit():
            for o in range(2):
                ctx.gp_fit_state(o, Xd, Yd[o], ls, var[o], 0.0)
            ctx.synchronize()

        variants = [("append", append), ("host_refit", host_refit), ("device_refit", device_refit)]
        t = {k: [] for k, _ in variants}
        r = repeats if n <= 1024 else max(3, repeats // 4)
        for rep in range(2 + r):
            for name, fn in variants:
                restore()
                t0 = time.perf_counter()
                fn()
                el = (time.perf_counter() - t0) * 1e3
                if rep >= 2:
                    t[name].append(el)
        row = {"n": n, "d": d, "n_obj": 2, "repeats": r}
        for k, v in t.items():
            row[k + "_ms"] = {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
        row["host_refit_over_append"] = row["host_refit_ms"]["median"] / row["append_ms"]["median"]
        row["device_refit_over_append"] = row["device_refit_ms"]["median"] / row["append_ms"]["median"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    ctx.close()
    return rows


def time_solve(budget=40, rounds=3):
    import torch
    import optimobo_amd.algorithms.optimisers as opti
    import optimobo_amd.scalarisations as sc
    from optimobo_amd.problem import ElementwiseProblem

    class MyProblem(ElementwiseProblem):
        def __init__(self):
            super().__init__(n_var=2, n_obj=2, xl=np.array([-2, -2]), xu=np.array([2, 2]))

        def _evaluate(self, x, out, *a, **k):
            out["F"] = [100 * (x[0] ** 2 + x[1] ** 2), (x[0] - 1) ** 2 + x[1] ** 2]

    def run(q):
        np.random.seed(0)
        opt = opti.MultiSurrogateOptimiser(MyProblem(), [0, 0], [700, 12], seed=1, batch_size=q)
        split = {"fit": 0.0, "maximise": 0.0}

        def timed(name, fn):
            def w(*a, **k):
                t = time.perf_counter()
                out = fn(*a, **k)
                torch.cuda.synchronize()
                split[name] += time.perf_counter() - t
                return out
            return w
        opt._fit_many = timed("fit", opt._fit_many)
        opt._maximise = timed("maximise", opt._maximise)
        t0 = time.perf_counter()
        res = opt.solve(budget=budget, n_init_samples=20, sample_exponent=3,
                        acquisition_func=sc.Tchebicheff([0, 0], [700, 12]))
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        return el / budget, split["fit"] / budget, split["maximise"] / budget, float(res.hypervolume_convergence[-1])

    t = {1: [], 4: []}
    for rnd in range(1 + rounds):            # round 0 warms up both
        for q in (1, 4):
            r = run(q)
            if rnd:
                t[q].append(r)
    rows = []
    for q, v in t.items():
        a = np.array(v)
        row = {"solve_batch_size": q, "budget": budget, "rounds": rounds,
               "ms_per_evaluation": {"median": float(np.median(a[:, 0]) * 1e3), "min": float(a[:, 0].min() * 1e3),
                                     "max": float(a[:, 0].max() * 1e3)},
               "fit_ms_per_evaluation": float(np.median(a[:, 1]) * 1e3),
               "maximise_ms_per_evaluation": float(np.median(a[:, 2]) * 1e3),
               "last_hypervolume_entry": float(a[-1, 3])}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="128,512,1024,4096")
    ap.add_argument("--repeats", type=int, default=12)
    ap.add_argument("--skip-solve", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("append_timing needs the GPU: a CPU run measures nothing")
    rows = time_appends([int(s) for s in args.sizes.split(",")], args.repeats)
    if not args.skip_solve:
        rows += time_solve()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
