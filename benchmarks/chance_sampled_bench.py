"""Deal-sampled iterations of the chance game (scopa_chance_cfr_iterate_sampled) against the full sweep on the same game: one process, one JSON
line, also written to `--out` (default profiles/chance_sampled.json).

  game               the 495 hidden-hand deals of the seed-42 seat-0 hand
  modes              "full": scopa_chance_cfr_iterate_weighted (every deal); "m16", "m64": scopa_chance_cfr_iterate_sampled with 16 / 64 deals
                     per iteration drawn by algorithms.chance.sample_deals
  us_per_iteration   `--iters` iterations per call, `--repeats` calls after `--warmup`, the modes interleaved, timed with HIP events on the
                     context's stream around the call (which includes the upload of the lists and weights and its final synchronise);
                     median, min, max.  Host-side drawing of the samples is outside the timed call
  equal_time         the budget is the median time of `--budget-iters` full iterations; each mode runs, from zero tables and with the `--variant`
                     schedule, the whole number of its iterations that fit that budget (by its median time per iteration), in ONE timed call;
                     recorded: iterations, the call's measured milliseconds and the exact exploitability over all 495 deals afterwards

Usage: python benchmarks/chance_sampled_bench.py [--iters 20] [--warmup 2] [--repeats 7] [--budget-iters 50] [--variant cfr+] [--seed 0] [--out path]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch                                                       # noqa: E402

from scopa_amd import _lib as sl                                   # noqa: E402
from scopa_amd.algorithms.cfr_variants import schedule             # noqa: E402
from scopa_amd.algorithms.chance import hidden_hand_deals, sample_deals   # noqa: E402

SAMPLES = (16, 64)


def _event_ms(stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def _stats(us):
    return {"median": round(statistics.median(us), 3), "min": round(min(us), 3), "max": round(max(us), 3), "calls": len(us)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--budget-iters", type=int, default=50)
    ap.add_argument("--variant", type=str, default="cfr+")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "chance_sampled.json"))
    a = ap.parse_args()
    stream = torch.cuda.Stream()
    ctx = sl.Context(0, stream=stream.cuda_stream)
    hand0 = sl.deal_py_seed(42)[:4]
    m = sl.MultiDeal(ctx, 495)
    m.set_perms(hidden_hand_deals(hand0))
    m.build()
    g = sl.ChanceGame(m)
    modes = ["full"] + [f"m{k}" for k in SAMPLES]

    def run(mode, t0, n):
        """n iterations of `mode` continuing the schedule and the samples from iteration t0"""
        w = schedule(a.variant, t0, n)
        if mode == "full":
            return lambda: g.cfr_iterate_weighted(w)
        lists = sample_deals(g.n, int(mode[1:]), t0, n, a.seed)
        return lambda: g.cfr_iterate_sampled(lists, w)

    for mode in modes:
        for _ in range(a.warmup):
            run(mode, 0, a.iters)()
    us = {mode: [] for mode in modes}
    for _ in range(a.repeats):                                     # interleaved: every mode sees the same clocks
        for mode in modes:
            us[mode].append(_event_ms(stream, run(mode, 0, a.iters)) * 1e3 / a.iters)
    out = {"bench": "chance_sampled", "game": "hidden_hand_495", "seat0_hand": [int(c) for c in hand0], "deals": g.n, "global_infosets": g.G,
           "occurrences": g.n_occurrences, "iters_per_call": a.iters, "variant": a.variant, "seed": a.seed,
           "us_per_iteration": {mode: _stats(us[mode]) for mode in modes}}
    g.tables_reset()
    uniform = float(g.exploitability()[0])
    budget_us = statistics.median(us["full"]) * a.budget_iters
    out["equal_time"] = {"budget_ms": round(budget_us * 1e-3, 3), "budget_full_iterations": a.budget_iters, "uniform_exploitability": uniform, "modes": {}}
    for mode in modes:
        n = a.budget_iters if mode == "full" else max(1, min(1 << 20, int(budget_us / statistics.median(us[mode]))))
        g.tables_reset()
        ms = _event_ms(stream, run(mode, 0, n))
        out["equal_time"]["modes"][mode] = {"iterations": n, "measured_ms": round(ms, 3), "exploitability": float(g.exploitability()[0])}
    g.close(); m.close(); ctx.close()
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
