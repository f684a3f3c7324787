"""Weighted synchronous CFR (k_cfr_sync_weighted) against the unweighted kernel, and what the weights buy: one process, one JSON line.

  per_iteration_us   seed-42 deal, `--iters` iterations per launch, `--repeats` launches each, the two kernels interleaved:
                     scopa_cfr_sync_iterate against scopa_cfr_sync_iterate_weighted at (1, 1, 1); median, min and max of the launches
  variants_us        the weighted kernel per variant, simultaneous and alternating (an alternating iteration is two sweeps)
  to_eps             per variant and form: iterations (checked every `--check-every`) and solver / wall seconds until the average policy's
                     exploitability is below 1e-3 and 1e-5 on the seed-42 deal, null where `--cap` iterations did not reach it
  multi              the same through MultiDeal.solve on `--deals` deals (py seeds 0 ..): mean / max iterations, deals at the cap, wall seconds

Usage: python benchmarks/cfr_variants_bench.py [--iters 200] [--repeats 7] [--cap 3000] [--deals 1024] [--multi-cap 1000]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scopa_amd import _lib as sl                                   # noqa: E402
from scopa_amd.algorithms.cfr_variants import VARIANTS, schedule   # noqa: E402


def _timed(fn):
    t = time.perf_counter()
    fn()
    return time.perf_counter() - t


def _stats(seconds, iters):
    us = [s / iters * 1e6 for s in seconds]
    return {"median": round(statistics.median(us), 3), "min": round(min(us), 3), "max": round(max(us), 3), "launches": len(us)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--check-every", type=int, default=10)
    ap.add_argument("--cap", type=int, default=3000)
    ap.add_argument("--deals", type=int, default=1024)
    ap.add_argument("--multi-cap", type=int, default=1000)
    a = ap.parse_args()
    ctx = sl.Context(0)
    n_inf = ctx.set_deal(sl.deal_py_seed(42))
    out = {"bench": "cfr_variants", "deal": 42, "n_infosets": n_inf, "iters_per_launch": a.iters}
    ones = np.ones((a.iters, 3))

    # -- the two kernels at the same arithmetic, interleaved (both are synchronous calls: the launch, the sweep and the wait)
    ctx.tables_reset()
    ctx.cfr_sync_iterate(a.iters); ctx.cfr_sync_iterate_weighted(ones)      # warm-up: code objects, LDS attributes, the weights' scratch
    plain, weighted = [], []
    for _ in range(max(a.repeats, 5)):
        plain.append(_timed(lambda: ctx.cfr_sync_iterate(a.iters)))
        weighted.append(_timed(lambda: ctx.cfr_sync_iterate_weighted(ones)))
    out["per_iteration_us"] = {"cfr_sync_iterate": _stats(plain, a.iters), "weighted_unit_weights": _stats(weighted, a.iters)}

    out["variants_us"] = {}
    for variant in VARIANTS:
        for alternating in (False, True):
            ctx.tables_reset()
            ts = [_timed(lambda: ctx.cfr_sync_iterate_weighted(schedule(variant, k * a.iters, a.iters), alternating)) for k in range(max(a.repeats, 5))]
            out["variants_us"][f"{variant}{'/alternating' if alternating else ''}"] = _stats(ts, a.iters)

    # -- iterations and time to a target exploitability
    out["to_eps"] = {}
    for variant in VARIANTS:
        for alternating in (False, True):
            ctx.tables_reset()
            t, solver, wall0, hit = 0, 0.0, time.perf_counter(), {}
            targets = [1e-3, 1e-5]
            while t < a.cap and targets:
                w = schedule(variant, t, a.check_every)
                solver += _timed(lambda: ctx.cfr_sync_iterate_weighted(w, alternating))
                t += a.check_every
                e = ctx.exploitability()["exploitability"]
                while targets and e < targets[0]:
                    hit[f"{targets.pop(0):.0e}"] = {"iterations": t, "solver_s": round(solver, 6), "wall_s": round(time.perf_counter() - wall0, 6)}
            for eps in targets:
                hit[f"{eps:.0e}"] = None
            hit["last"] = {"iterations": t, "exploitability": e}
            out["to_eps"][f"{variant}{'/alternating' if alternating else ''}"] = hit

    # -- many deals: MultiDeal.solve drops a deal from the active mask once it is below eps
    out["multi"] = {"deals": a.deals, "check_every": a.check_every, "cap": a.multi_cap}
    for eps in (1e-3, 1e-5):
        for variant in VARIANTS:
            m = sl.MultiDeal(ctx, a.deals)
            m.deal_py_seeds(np.arange(a.deals))
            m.build()
            wall = time.perf_counter()
            used = m.solve(variant, eps, a.multi_cap, check_every=a.check_every)
            wall = time.perf_counter() - wall
            out["multi"][f"{variant}@{eps:.0e}"] = {"mean_iterations": round(float(used.mean()), 2), "max_iterations": int(used.max()),
                                                   "at_cap": int((used >= a.multi_cap).sum()), "wall_s": round(wall, 4)}
            m.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
