#!/usr/bin/env python3
"""The frontier form of Deep CFR's traversal on FullScopa over decks (scopa_full_chance_sdcfr_traverse_frontier,
FullChanceDeepCFR(traversal="frontier")): what a call costs beside the forest form, what it costs where the forest form cannot go, and the experiment
the form exists for -- whether nets trained on many decks carry to decks they have not seen.  Prints one JSON line and writes it to --out
(rewritten after every stage, so a run that is cut short leaves what it measured).

    python benchmarks/full_chance_frontier_bench.py [--seed 42] [--repeats 5] [--budget-s 40] [--epochs 10] [--many 1024]
                                                    [--out profiles/full_chance_frontier_bench.json]

Every figure is from ONE run of this script, one process.  No threshold is set on any of them.
decks        packet_decks(deck --seed, 4, 72 + --many, 1): its first 72 decks are full_chance_sdcfr_bench.py's packet (training decks 0..7, held-out
             decks 64..71); every deck fits the round-2 root of the random play (RandomState(0)) on deck 0 and the round-3 root below it.
call_ms      per (R, decks, batch) in R = 2, 3 x 8, 64 decks x batch 8, 64, traverser 0, freshly initialised nets: HIP events on the context's stream
             around ONE traverse call of each form (the median of --repeats calls after a first call that builds the forest or the scratch);
             `ratio` = frontier / forest; `forest_nodes` = the choice nodes the forest's policy launch evaluates whatever the batch, `visits` = the
             nodes the call's traversals visit, which is what the frontier form evaluates.
beyond_ms    the frontier form alone at R = 5 and R = 6 (the deal) on 8 decks at batch 8 and 64, traverser 0: time, visits / s, TFLOP/s by the
             46 080 flop / node model (`of_peak` against the 157 TFLOP/s float32 matrix peak), and the ring's bytes / s (544 a row).
generalisation  (BR0 + BR1) / 2 of the average policy on the round-3 root after --budget-s seconds of wall time in train() calls (chunks of 10
             iterations with resume=True), train_backend="hip", batch 64: on the 8 training decks with the forest form (the protocol of
             full_chance_sdcfr_bench.py), on the same 8 with the frontier form, and on --many decks with the frontier form and
             decks_per_iteration=8.  `held_out`: on decks 64..71 of the packet, none of which any run trains on; `train`: on the training decks (on
             the first 8 of them where the set is beyond the exact sweeps' cap).  With R = 3 the response has imperfect recall across rounds: the
             figures are lower bounds on the exploitability."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FLOP_PER_NODE = 46080
PEAK_TFLOPS = 157.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--budget-s", type=float, default=40.0)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--many", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from scopa_amd import _lib
    from scopa_amd.algorithms import FullChanceMCCFRTrainer, packet_decks
    from scopa_amd.algorithms.deep_cfr import AdvantageNetwork, FullChanceDeepCFR
    from scopa_amd.algorithms.deep_cfr.full_chance_deep_cfr import rows_per_traversal
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import full_mccfr_ref as F
    stream = torch.cuda.Stream()
    ctx = _lib.Context(0, stream=stream.cuda_stream)
    ctx.mccfr_seed(0x5C09A)
    deck = _lib.full_deal_py_seed(a.seed)
    _, acts = F.random_root(deck, 4, np.random.RandomState(0))
    decks = packet_decks(deck, 4, 72 + a.many, 1)

    def state_after(n_rounds):
        s = _lib.FullState(deck=deck)
        for x in acts[:6 * n_rounds]:
            s.step(x)
        return s.s

    rec = dict(bench="full_chance_frontier", runs=1, seed=a.seed, device=torch.cuda.get_device_name(0), repeats=a.repeats, budget_s=a.budget_s, epochs=a.epochs,
               call_ms={}, beyond_ms={}, generalisation={})

    def flush():
        line = json.dumps(rec)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return line

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        stream.synchronize()
        return e0.elapsed_time(e1)

    def ring_of(rows, n_vals):
        with torch.cuda.stream(stream):
            return (torch.zeros((rows, 96), dtype=torch.float32, device="cuda:0"), torch.zeros((rows, 40), dtype=torch.float32, device="cuda:0"),
                    torch.zeros(n_vals, dtype=torch.float32, device="cuda:0"))

    with torch.cuda.stream(stream):
        nets = [AdvantageNetwork(96, 40, "cuda:0", memory_size=1) for _ in range(2)]
        w = [torch.stack([nets[0].param_list()[k].detach(), nets[1].param_list()[k].detach()]).contiguous() for k in range(6)]
    wp = [t.data_ptr() for t in w]
    visits_of = lambda R, n, batch: n * batch * 13 * (6 ** R - 1) // 5

    # ---- forest against frontier, one call ----
    for R in (2, 3):
        for n in (8, 64):
            h = _lib.FullChanceMCCFR(ctx, decks[:n], state_after(6 - R), 4)
            for batch in (8, 64):
                rows = rows_per_traversal(R) * n * batch
                feat, regret, vals = ring_of(rows, n * batch)
                entry = dict(forest_nodes=n * 31 * (36 ** R - 1) // 35, visits=visits_of(R, n, batch), rows=rows)
                for name, call in (("forest", h.sdcfr_traverse), ("frontier", h.sdcfr_traverse_frontier)):
                    run = lambda: call(0, batch, wp, feat.data_ptr(), regret.data_ptr(), rows, 0, vals.data_ptr(), 1, 0)
                    entry[name + "_first_call_ms"] = timed(run)
                    entry[name + "_ms"] = float(np.median([timed(run) for _ in range(a.repeats)]))
                entry["ratio"] = entry["frontier_ms"] / entry["forest_ms"]
                rec["call_ms"][f"R{R}_decks{n}_batch{batch}"] = entry
                flush()
                del feat, regret, vals
            h.close()

    # ---- the frontier form where the forest cannot go ----
    for R in (5, 6):
        h = _lib.FullChanceMCCFR(ctx, decks[:8], state_after(6 - R), 4)
        for batch in (8, 64):
            rows = rows_per_traversal(R) * 8 * batch
            feat, regret, vals = ring_of(rows, 8 * batch)
            run = lambda: h.sdcfr_traverse_frontier(0, batch, wp, feat.data_ptr(), regret.data_ptr(), rows, 0, vals.data_ptr(), 1, 0)
            first = timed(run)
            ms = float(np.median([timed(run) for _ in range(a.repeats)]))
            v = visits_of(R, 8, batch)
            tflops = v * FLOP_PER_NODE / (ms * 1e-3) / 1e12
            rec["beyond_ms"][f"R{R}_decks8_batch{batch}"] = dict(first_call_ms=first, ms=ms, visits=v, visits_per_s=v / (ms * 1e-3), tflops=tflops, of_peak=tflops / PEAK_TFLOPS,
                                                                rows=rows, ring_bytes_per_s=rows * 544 / (ms * 1e-3))
            flush()
            del feat, regret, vals
        h.close()
    torch.cuda.empty_cache()

    # ---- generalisation ----
    held, acts3 = decks[64:72], tuple(acts[:18])
    for name, train, kw in (("forest_8", decks[:8], dict(traversal="forest")), ("frontier_8", decks[:8], dict(traversal="frontier")),
                            (f"frontier_{a.many}", decks[72:], dict(traversal="frontier", decks_per_iteration=8))):
        t = FullChanceMCCFRTrainer(decks=train, root_actions=acts3, capacity_log2=4, batch=1, ctx=ctx)
        d = FullChanceDeepCFR(t, batch=64, train_backend="hip", **kw)
        wall, its = 0.0, 0
        while wall < a.budget_s:
            t0 = time.perf_counter()
            d.train(10, advantage_epochs=a.epochs, resume=True)
            stream.synchronize()
            wall += time.perf_counter() - t0
            its += 10
        rec["generalisation"][name] = dict(decks=len(train), decks_per_iteration=kw.get("decks_per_iteration"), iterations=its, wall_s=wall,
                                           train=d.exploitability(decks=train[:8])["exploitability"], held_out=d.exploitability(decks=held)["exploitability"],
                                           snapshots=[len(b._slots) for b in d.strategy_buffers], losses=[x[-1] for x in d.training_history["losses"]])
        t.close()
        flush()
    t = FullChanceMCCFRTrainer(decks=decks[:8], root_actions=acts3, capacity_log2=4, batch=1, ctx=ctx)
    rec["generalisation"]["uniform"] = dict(train=t.exploitability()["exploitability"], held_out=t.exploitability(decks=held)["exploitability"])
    t.close()
    print(flush())
    ctx.close()


if __name__ == "__main__":
    main()
