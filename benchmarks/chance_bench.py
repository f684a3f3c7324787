"""The chance game over a set of deals (k_chance_sweep + k_chance_reduce) against the per-deal solver on the same deals: one process, one JSON line.

  games              the 495 hidden-hand deals of the seed-42 seat-0 hand, and `--random-deals` py-seeded deals (skipped if memory does not allow)
  chance_us          per iteration of scopa_chance_cfr_iterate_weighted, `--iters` iterations per call, `--repeats` calls after `--warmup`, timed with
                     HIP events on the context's stream; median, min, max
  per_deal_us        the baseline: scopa_multi_cfr_sync_iterate_weighted on the same deals -- the per-deal work without the exchange
  ratio              chance median / per-deal median
  reduce_traffic     k_chance_reduce's algorithmic bytes per launch: 64 B per occurrence in, 96 B per global row in and out; with `--reduce-us`
                     (the kernel's mean time from a kernel trace of this benchmark) the achieved bytes/s against the 8 TB/s HBM peak
  curves             exploitability of the 495-deal game every `--check-every` iterations up to `--curve-iters`, plain and DCFR(1.5, 0, 2)

Usage: python benchmarks/chance_bench.py [--iters 20] [--warmup 2] [--repeats 7] [--random-deals 16384] [--curve-iters 200] [--reduce-us t495,tRandom]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch                                                       # noqa: E402

from scopa_amd import _lib as sl                                   # noqa: E402
from scopa_amd.algorithms.cfr_variants import schedule             # noqa: E402
from scopa_amd.algorithms.chance import hidden_hand_deals          # noqa: E402

HBM_PEAK = 8.0e12


def _event_us(stream, fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def _stats(us):
    return {"median": round(statistics.median(us), 3), "min": round(min(us), 3), "max": round(max(us), 3), "calls": len(us)}


def _game(ctx, stream, name, deals_fn, a, reduce_us):
    try:
        m = deals_fn()
        g = sl.ChanceGame(m)
    except sl.ScopaError as e:
        if e.status in (sl.SCOPA_ENOMEM, sl.SCOPA_ELIMIT):
            return {"game": name, "skipped": str(e)}, None, None
        raise
    ones = np.ones((a.iters, 3))
    for _ in range(a.warmup):
        g.cfr_iterate_weighted(ones)
        m.cfr_sync_iterate_weighted(ones)
    chance, per_deal = [], []
    for _ in range(a.repeats):                                     # interleaved: both see the same clocks
        chance.append(_event_us(stream, lambda: g.cfr_iterate_weighted(ones), a.iters))
        per_deal.append(_event_us(stream, lambda: m.cfr_sync_iterate_weighted(ones), a.iters))
    traffic = 64 * g.n_occurrences + 96 * g.G
    rec = {"game": name, "deals": g.n, "global_infosets": g.G, "occurrences": g.n_occurrences, "chance_us": _stats(chance), "per_deal_us": _stats(per_deal),
           "ratio": round(statistics.median(chance) / statistics.median(per_deal), 4),
           "reduce_traffic": {"bytes_per_launch": traffic, "kernel_us": reduce_us,
                              "bytes_per_s": None if reduce_us is None else round(traffic / (reduce_us * 1e-6), 1),
                              "fraction_of_hbm_peak": None if reduce_us is None else round(traffic / (reduce_us * 1e-6) / HBM_PEAK, 5)}}
    return rec, m, g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--random-deals", type=int, default=16384)
    ap.add_argument("--curve-iters", type=int, default=200)
    ap.add_argument("--check-every", type=int, default=10)
    ap.add_argument("--reduce-us", type=str, default="")
    a = ap.parse_args()
    reduce_us = [float(x) for x in a.reduce_us.split(",")] if a.reduce_us else [None, None]
    stream = torch.cuda.Stream()
    ctx = sl.Context(0, stream=stream.cuda_stream)
    hand0 = sl.deal_py_seed(42)[:4]
    out = {"bench": "chance", "iters_per_call": a.iters, "seat0_hand": [int(c) for c in hand0], "games": []}

    def hidden():
        m = sl.MultiDeal(ctx, 495)
        m.set_perms(hidden_hand_deals(hand0))
        m.build()
        return m

    def random_deals():
        m = sl.MultiDeal(ctx, a.random_deals)
        m.deal_py_seeds(np.arange(a.random_deals))
        m.build()
        return m

    rec, m, g = _game(ctx, stream, "hidden_hand_495", hidden, a, reduce_us[0])
    out["games"].append(rec)
    out["curves"] = {}
    for variant in ("vanilla", "dcfr"):
        g.tables_reset()
        curve = []
        for t in range(0, a.curve_iters, a.check_every):
            g.cfr_iterate_weighted(schedule(variant, t, a.check_every))
            curve.append([t + a.check_every, float(g.exploitability()[0])])
        out["curves"][variant] = curve
    g.close(); m.close()
    if a.random_deals > 0:
        rec, m, g = _game(ctx, stream, f"random_{a.random_deals}", random_deals, a, reduce_us[1])
        out["games"].append(rec)
        if g is not None:
            g.close(); m.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
