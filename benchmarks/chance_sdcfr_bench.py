"""Deep CFR traversals over a set of deals (scopa_chance_sdcfr_traverse) against the only earlier route -- a host loop of scopa_set_deal +
scopa_sdcfr_traverse_fused per deal -- and the exploitability ChanceDeepCFR reaches: one process, one JSON line, also written to `--out` (default
profiles/chance_sdcfr.json).

  game        the 495 hidden-hand deals of the seed-42 seat-0 hand (chance.hidden_hand_deals)
  traverse    per shape (m, batch) = (495, 8), (64, 64), (1, 4096) and per player: ONE scopa_chance_sdcfr_traverse call over the shape's deals (all 495;
              the 64 of chance.sample_deals' first row; deal 0) into a ring of 41 * m * batch rows, timed with HIP events on the context's stream,
              median / min / max of `--repeats` calls after `--warmup`.  "loop": m x (set_deal + scopa_sdcfr_traverse_fused) on one single-deal context
              on the same stream, the same deals, ids and ring rows -- a tree build and two launches per deal; for (1, 4096) scopa_sdcfr_traverse_fused
              itself on a context that already holds the deal.  ratio = loop / chance (> 1: the one-call form is faster).  rows_bytes_per_s = 41 * m * batch
              * DeviceMemory.row_bytes over the chance call's median, and its fraction of the HBM peak (8.0 TB/s)
  training    ChanceDeepCFR(batch `--train-batch`, deals_per_iteration `--train-deals`) for `--train-iters` iterations of `--epochs` epochs from
              torch.manual_seed(0): the exact exploitability across all 495 deals at the start (no snapshot: uniform) and at the end, and the wall time

Usage: python benchmarks/chance_sdcfr_bench.py [--repeats 30] [--warmup 3] [--train-iters 20] [--train-batch 8] [--train-deals 64] [--epochs 10] [--out path]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np                                                 # noqa: E402
import torch                                                       # noqa: E402

from scopa_amd import _lib as sl                                   # noqa: E402
from scopa_amd.algorithms import chance                            # noqa: E402
from scopa_amd.algorithms.deep_cfr import ChanceDeepCFR, DeviceMemory   # noqa: E402

SHAPES = ((495, 8), (64, 64), (1, 4096))
HBM_PEAK = 8.0e12
SEED = 0x5C09A


def _event_us(stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def _stats(us):
    return {"median": round(statistics.median(us), 3), "min": round(min(us), 3), "max": round(max(us), 3), "calls": len(us)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--train-iters", type=int, default=20)
    ap.add_argument("--train-batch", type=int, default=8)
    ap.add_argument("--train-deals", type=int, default=64)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "chance_sdcfr.json"))
    a = ap.parse_args()
    stream = torch.cuda.Stream()
    ctx = sl.Context(0, stream=stream.cuda_stream)
    ctx.mccfr_seed(SEED)
    hand0 = sl.deal_py_seed(42)[:4]
    perms = chance.hidden_hand_deals(hand0)
    multi = sl.MultiDeal(ctx, len(perms))
    multi.set_perms(perms)
    multi.build()
    g = sl.ChanceGame(multi)
    single = sl.Context(0, stream=stream.cuda_stream)             # the earlier route: one deal at a time, on the same stream
    single.mccfr_seed(SEED)

    torch.manual_seed(0)
    with torch.cuda.stream(stream):
        d = ChanceDeepCFR(g, batch=a.train_batch, deals_per_iteration=a.train_deals, seed=SEED)
        image = d._packed_weights()
        row_bytes = DeviceMemory(1, 34, "cuda:0").row_bytes
        out = {"bench": "chance_sdcfr", "game": "hidden_hand_495", "seat0_hand": [int(c) for c in hand0], "deals": g.n, "global_infosets": g.G,
               "row_bytes": row_bytes, "hbm_peak_bytes_per_s": HBM_PEAK, "traverse": {}}
        for m, batch in SHAPES:
            deals = None if m == g.n else (chance.sample_deals(g.n, m, 0, 1, SEED)[0] if m > 1 else np.zeros(1, np.int32))
            ids = np.arange(g.n) if deals is None else deals
            rows = 41 * m * batch
            feat = torch.zeros((rows, 34), dtype=torch.float32, device="cuda:0")
            regret = torch.zeros((rows, 16), dtype=torch.float32, device="cuda:0")
            vals = torch.zeros(m * batch, dtype=torch.float32, device="cuda:0")
            if m == 1:
                single.set_deal(perms[0])
            for player in range(2):
                def call(player=player):
                    g.sdcfr_traverse(player, batch, image.data_ptr(), feat.data_ptr(), regret.data_ptr(), 0, rows, 0, vals.data_ptr(), 0, 0, deals)

                def loop(player=player):
                    for s, deal in enumerate(ids):
                        if m > 1:
                            single.set_deal(perms[deal])
                        single.sdcfr_traverse_fused(player, batch, image.data_ptr(), feat.data_ptr(), regret.data_ptr(), 0, rows, 41 * s * batch,
                                                    vals.data_ptr() + 4 * s * batch, 0, 0, int(deal) * batch)
                for fn in (call, loop):
                    for _ in range(a.warmup):
                        fn()
                us = {"chance": [], "loop": []}
                for _ in range(a.repeats):                         # interleaved: both legs see the same clocks
                    us["chance"].append(_event_us(stream, call))
                    us["loop"].append(_event_us(stream, loop))
                med = statistics.median(us["chance"])
                out["traverse"][f"m{m}_b{batch}_p{player}"] = {
                    "chance_us": _stats(us["chance"]), "loop_us": _stats(us["loop"]), "ratio_loop_over_chance": round(statistics.median(us["loop"]) / med, 3),
                    "difference_us": round(med - statistics.median(us["loop"]), 3), "rows": rows, "rows_bytes_per_s": rows * row_bytes / (med * 1e-6),
                    "fraction_of_hbm_peak": round(rows * row_bytes / (med * 1e-6) / HBM_PEAK, 4)}
            del feat, regret, vals
    stream.synchronize()
    e0 = d.exploitability()["exploitability"]
    t0 = time.perf_counter()
    d.train(iterations=a.train_iters, advantage_epochs=a.epochs)
    stream.synchronize()
    seconds = time.perf_counter() - t0
    out["training"] = {"batch": a.train_batch, "deals_per_iteration": a.train_deals, "iterations": a.train_iters, "advantage_epochs": a.epochs,
                       "exploitability_start": e0, "exploitability_end": d.exploitability()["exploitability"], "train_seconds": round(seconds, 3),
                       "decision_visits": g.sdcfr_visits()}
    single.close(); g.close(); multi.close(); ctx.close()
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
