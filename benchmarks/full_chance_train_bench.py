#!/usr/bin/env python3
"""The optimiser step of FullScopa's 96-128-64-40 advantage net: the hand-written step (scopa_full_sdcfr_train_steps, FullChanceDeepCFR(train_backend=
"hip")) beside the PyTorch paths, in one process.  Prints one JSON line and writes it to --out (rewritten after every stage, so a run that is cut
short leaves what it measured).

    python benchmarks/full_chance_train_bench.py [--seed 42] [--batch 64] [--repeats 9] [--budget-s 40] [--epochs 10]
                                                 [--out profiles/full_chance_train_bench.json]

Every figure is from ONE run of this script.  No threshold is set on any of them.  The game is full_chance_sdcfr_bench.py's: the round-3 root (R = 3)
of the random play on deck --seed, 8 decks of the packet to train on and 8 held out, --batch traversals a deck.
train_call_ms  one train() call of --epochs epochs on player 0's memory after two iterations (176 128 rows), at train batch 128, 1 024 and 8 192: HIP
               events on the solver's stream around the call, the median of --repeats calls after three warm-up calls (the first captures the graph).
               torch_eager: AdvantageNetwork's default; torch_graph: its graph-replayed lean step (graph_training=True); hip: the hand-written step.
iteration_ms   a whole FullChanceDeepCFR iteration (two traversal calls, 2 x --epochs optimiser steps, the snapshots) at train batch 128 per backend:
               HIP events around a 5-iteration train() after a 2-iteration warm-up, divided by 5.
budget         iterations completed in --budget-s seconds of wall time in the solver's own calls (train(10, resume=True) chunks, train batch 128) by
               each backend from scratch, and (BR0 + BR1) / 2 of the average policy at the end on the training decks and on the held-out decks."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TRAIN_BATCHES = (128, 1024, 8192)
BACKENDS = (("torch_eager", dict(train_backend="torch")), ("torch_graph", dict(train_backend="torch", graph_training=True)), ("hip", dict(train_backend="hip")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--budget-s", type=float, default=40.0)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from scopa_amd import _lib
    from scopa_amd.algorithms import FullChanceMCCFRTrainer, packet_decks
    from scopa_amd.algorithms.deep_cfr import AdvantageNetwork, FullChanceDeepCFR
    from scopa_amd.algorithms.deep_cfr.full_chance_deep_cfr import FullAdvantageNetwork, rows_per_traversal
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import full_mccfr_ref as F
    stream = torch.cuda.Stream()
    ctx = _lib.Context(0, stream=stream.cuda_stream)
    ctx.mccfr_seed(0x5C09A)
    deck = _lib.full_deal_py_seed(a.seed)
    _, acts = F.random_root(deck, 4, np.random.RandomState(0))
    decks = packet_decks(deck, 4, 72, 1)
    train, held, acts3 = decks[:8], decks[64:72], tuple(acts[:18])
    rec = dict(bench="full_chance_train", runs=1, seed=a.seed, device=torch.cuda.get_device_name(0), batch=a.batch, repeats=a.repeats, budget_s=a.budget_s,
               epochs=a.epochs, R=3, decks=8, rows_per_iteration=2 * rows_per_traversal(3) * 8 * a.batch, train_call_ms={}, iteration_ms={}, budget={})

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

    def deep(**kw):
        t = FullChanceMCCFRTrainer(decks=train, root_actions=acts3, capacity_log2=4, batch=1, ctx=ctx)
        return FullChanceDeepCFR(t, batch=a.batch, **kw), t

    # ---- one train() call ----
    d, t = deep()
    d.train(2, advantage_epochs=1)
    stream.synchronize()
    mem = d.advantage_nets[0].buffer
    rec["memory_rows"] = len(mem)
    with torch.cuda.stream(stream):
        for name, kw in BACKENDS:
            net = (FullAdvantageNetwork("cuda:0", memory_size=1) if kw["train_backend"] == "hip" else
                   AdvantageNetwork(96, 40, "cuda:0", memory_size=1, use_graph=kw.get("graph_training", False)))
            net._ctx, net._ctx_stream, net.buffer = ctx, d._stream, mem      # every path trains on the same rows
            for tb in TRAIN_BATCHES:
                call = lambda: net.train(batch_size=tb, epochs=a.epochs, defer=True)
                for _ in range(3):
                    timed(call)
                ms = [timed(call) for _ in range(a.repeats)]
                rec["train_call_ms"].setdefault(f"batch{tb}", {})[name] = dict(median=float(np.median(ms)), min=float(np.min(ms)))
            flush()
            del net
    t.close()

    # ---- a whole iteration, the budget ----
    for name, kw in BACKENDS:
        d, t = deep(**kw)
        d.train(2, advantage_epochs=a.epochs)
        stream.synchronize()
        rec["iteration_ms"][name] = timed(lambda: d.train(5, advantage_epochs=a.epochs, resume=True)) / 5
        t.close()
        flush()
    for name, kw in BACKENDS:
        d, t = deep(**kw)
        wall, its = 0.0, 0
        while wall < a.budget_s:
            t0 = time.perf_counter()
            d.train(10, advantage_epochs=a.epochs, resume=True)       # the loop index goes on across the calls: a snapshot an iteration from the second on
            stream.synchronize()
            wall += time.perf_counter() - t0
            its += 10
        s = d.policy_store()
        h = d.policy_store(decks=held)
        rec["budget"][name] = dict(iterations=its, wall_s=wall, iterations_per_s=its / wall, train=s.exploitability()["exploitability"],
                                   held_out=h.exploitability(decks=held)["exploitability"], snapshots=[len(b._slots) for b in d.strategy_buffers],
                                   losses=[x[-1] for x in d.training_history["losses"]])
        s.close(), h.close(), t.close()
        flush()
    print(flush())
    ctx.close()


if __name__ == "__main__":
    main()
