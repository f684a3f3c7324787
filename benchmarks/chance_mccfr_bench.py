"""Chance-sampled MCCFR on the chance game (scopa_chance_mccfr_iterate) against the same walks without the exchange across deals
(scopa_multi_mccfr_iterate), and against the sweeping solvers in equal time: one process, one JSON line, also written to `--out` (default
profiles/chance_mccfr.json).

  game               the 495 hidden-hand deals of the seed-42 seat-0 hand
  visits             per batch (64, 1024) and deal set ("full": all 495 deals; "m64": 64 deals per iteration drawn by algorithms.chance.sample_deals):
                     `--iters` iterations per call, `--repeats` calls after `--warmup`, timed with HIP events on the context's stream around the call
                     (which includes the upload of the lists and the final synchronise); median, min, max of the time per iteration, and decision
                     visits per second from the handle's exact counters.  "baseline": scopa_multi_mccfr_iterate with the same batch on the same
                     number of deals (all 495; the 64 deals of the first list) -- one persistent launch per call, no shared rows, no reduce.
                     ratio = chance visits/s over baseline visits/s.  Host-side drawing of the samples is outside the timed call
  equal_time         the budget is the median time of `--budget-iters` full CFR+ iterations.  chance.solve_mccfr (batch `--solve-batch`, all deals),
                     chance.solve(variant="cfr+") and chance.solve(variant="cfr+", sample=64) each run, from zero tables, the whole number of their
                     iterations that fits that budget (by their median time per iteration) as ONE chunk; recorded: iterations, the call's measured
                     milliseconds (iterations + one exploitability pass) and the exact exploitability over all 495 deals

Usage: python benchmarks/chance_mccfr_bench.py [--iters 20] [--warmup 2] [--repeats 7] [--budget-iters 50] [--solve-batch 64] [--seed 0] [--out path]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch                                                       # noqa: E402

from scopa_amd import _lib as sl                                   # noqa: E402
from scopa_amd.algorithms import chance                            # noqa: E402
from scopa_amd.algorithms.cfr_variants import schedule             # noqa: E402

BATCHES = (64, 1024)
SAMPLE = 64
PAIR_DECISION_VISITS = 463


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
    ap.add_argument("--solve-batch", type=int, default=64)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "chance_mccfr.json"))
    a = ap.parse_args()
    stream = torch.cuda.Stream()
    ctx = sl.Context(0, stream=stream.cuda_stream)
    hand0 = sl.deal_py_seed(42)[:4]
    perms = chance.hidden_hand_deals(hand0)
    m = sl.MultiDeal(ctx, len(perms))
    m.set_perms(perms)
    m.build()
    g = sl.ChanceGame(m)
    lists = chance.sample_deals(g.n, SAMPLE, 0, a.iters, a.seed)
    sub = sl.MultiDeal(ctx, SAMPLE)                                # the baseline of the sampled mode: the first list's deals on their own
    sub.set_perms(perms[lists[0]])
    sub.build()

    legs = {}
    for batch in BATCHES:
        legs[f"b{batch}_full"] = (lambda b=batch: g.mccfr_iterate(b, a.iters, a.seed), g.n * batch)
        legs[f"b{batch}_full_baseline"] = (lambda b=batch: m.mccfr_iterate(b, a.iters, a.seed), g.n * batch)
        legs[f"b{batch}_m{SAMPLE}"] = (lambda b=batch: g.mccfr_iterate(b, a.iters, a.seed, lists), SAMPLE * batch)
        legs[f"b{batch}_m{SAMPLE}_baseline"] = (lambda b=batch: sub.mccfr_iterate(b, a.iters, a.seed), SAMPLE * batch)
    w = schedule("cfr+", 0, a.iters)
    legs["cfr+_full"] = (lambda: g.cfr_iterate_weighted(w), None)
    legs[f"cfr+_m{SAMPLE}"] = (lambda: g.cfr_iterate_sampled(lists, w), None)
    for fn, _ in legs.values():
        for _ in range(a.warmup):
            fn()
    us = {k: [] for k in legs}
    for _ in range(a.repeats):                                     # interleaved: every leg sees the same clocks
        for k, (fn, _) in legs.items():
            us[k].append(_event_ms(stream, fn) * 1e3 / a.iters)
    out = {"bench": "chance_mccfr", "game": "hidden_hand_495", "seat0_hand": [int(c) for c in hand0], "deals": g.n, "global_infosets": g.G,
           "occurrences": g.n_occurrences, "iters_per_call": a.iters, "seed": a.seed, "us_per_iteration": {k: _stats(v) for k, v in us.items()}, "visits": {}}
    for k, (_, pairs) in legs.items():
        if pairs is not None:
            out["visits"][k] = {"pairs_per_iteration": pairs, "decision_visits_per_s": pairs * PAIR_DECISION_VISITS / (statistics.median(us[k]) * 1e-6)}
    for batch in BATCHES:
        for mode in ("full", f"m{SAMPLE}"):
            k = f"b{batch}_{mode}"
            out["visits"][k]["ratio_to_baseline"] = out["visits"][k]["decision_visits_per_s"] / out["visits"][k + "_baseline"]["decision_visits_per_s"]
    d, _, iters = g.mccfr_counters()
    out["counters"] = {"decision_visits": d, "mccfr_iterations": iters}
    g.close()

    budget_us = statistics.median(us["cfr+_full"]) * a.budget_iters
    solvers = {f"mccfr_b{a.solve_batch}": (us.get(f"b{a.solve_batch}_full"), lambda n: chance.solve_mccfr(m, a.solve_batch, eps=0.0, max_iters=n, check_every=n, seed=a.seed)),
               "cfr+_full": (us["cfr+_full"], lambda n: chance.solve(m, "cfr+", eps=0.0, max_iters=n, check_every=n)),
               f"cfr+_m{SAMPLE}": (us[f"cfr+_m{SAMPLE}"], lambda n: chance.solve(m, "cfr+", eps=0.0, max_iters=n, check_every=n, sample=SAMPLE, seed=a.seed))}
    out["equal_time"] = {"budget_ms": round(budget_us * 1e-3, 3), "budget_full_cfr+_iterations": a.budget_iters, "solvers": {}}
    for name, (t_us, solve) in solvers.items():
        if t_us is None:                                           # a --solve-batch that was not timed above: time it now
            fn = lambda: chance.solve_mccfr(m, a.solve_batch, eps=0.0, max_iters=a.iters, check_every=a.iters, seed=a.seed)[0].close()
            fn()
            t_us = [_event_ms(stream, fn) * 1e3 / a.iters]
        n = max(1, min(1 << 20, int(budget_us / statistics.median(t_us))))
        res = {}
        ms = _event_ms(stream, lambda: res.update(zip(("game", "t", "curve"), solve(n))))
        out["equal_time"]["solvers"][name] = {"iterations": res["t"], "measured_ms": round(ms, 3), "exploitability": res["curve"][-1][1]}
        res["game"].close()
    sub.close(); m.close(); ctx.close()
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
