#!/usr/bin/env python3
"""Deep CFR on FullScopa over a set of decks (scopa_full_chance_sdcfr_*, algorithms.deep_cfr.FullChanceDeepCFR): what its launches cost, and the
figure the feature exists for -- how the policy carries to decks it has not seen -- beside the tabular solvers in the same run.  Prints one JSON
line and writes it to --out (rewritten after every stage, so a run that is cut short leaves what it measured).

    python benchmarks/full_chance_sdcfr_bench.py [--seed 42] [--batch 64] [--repeats 5] [--budget-s 40] [--epochs 10] [--snapshots 100]
                                                 [--out profiles/full_chance_sdcfr_bench.json]

Every figure is from ONE run of this script, one process.  No threshold is set on any of them.
decks        packet_decks(deck --seed, 4, 72, 1): decks that share their first four rounds, so every one of them fits the round-2 root of the random
             play (RandomState(0)) on deck 0 and the round-3 root one round further down (the exploitability bench's packet).
launch_ms    per (R, decks) in (2, 8), (2, 64), (3, 8), (3, 64) at --batch, traverser 0, freshly initialised nets: HIP events on the context's stream
             around a traverse call that makes the policy launch alone, the walk launch alone, and both (the median of --repeats calls after a first
             call that builds the forest); `nodes` = the choice nodes the policy launch evaluates, `rows` = the memory rows the walk writes.
iteration_ms FullChanceDeepCFR on the round-3 root, 8 decks, --batch, --epochs optimiser epochs: wall time per iteration of a 5-iteration train()
             after a 2-iteration warm-up.
average_ms   the average policy of --snapshots snapshots at every choice node of both players on those 8 decks (wall time of the two synchronous
             calls), and policy_rows() on top of it (the host's deduplication).
generalisation  (BR0 + BR1) / 2 of the average policy on the round-3 root on the 8 training decks and on 8 held-out decks of the packet, after
             --budget-s seconds of wall time in the solver's own calls: Deep CFR (train(10, resume=True) chunks, so that the snapshots are those
             of one long call: `snapshots` = the nets each player's buffer holds at the end, at most 100, `snapshot_weights` the first and the
             last weight), tabular MCCFR at --batch (chunks of 10 iterations) and exact DCFR(1.5, 0, 2) (chunks of 5 iterations), each from
             scratch; `uniform` is the empty store.  With R = 3 the response has imperfect recall across rounds: the figures are lower bounds on
             the exploitability."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((2, 8), (2, 64), (3, 8), (3, 64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--budget-s", type=float, default=40.0)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--snapshots", type=int, default=100)
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
    decks = packet_decks(deck, 4, 72, 1)

    def state_after(n_rounds):
        s = _lib.FullState(deck=deck)
        for x in acts[:6 * n_rounds]:
            s.step(x)
        return s.s

    rec = dict(bench="full_chance_sdcfr", runs=1, seed=a.seed, device=torch.cuda.get_device_name(0), batch=a.batch, repeats=a.repeats, budget_s=a.budget_s,
               epochs=a.epochs, launch_ms={}, generalisation={})

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

    # ---- the launches ----
    with torch.cuda.stream(stream):
        nets = [AdvantageNetwork(96, 40, "cuda:0", memory_size=1) for _ in range(2)]
        w = [torch.stack([nets[0].param_list()[k].detach(), nets[1].param_list()[k].detach()]).contiguous() for k in range(6)]
    for R, n in SHAPES:
        h = _lib.FullChanceMCCFR(ctx, decks[:n], state_after(6 - R), 4)
        rows = rows_per_traversal(R) * n * a.batch
        with torch.cuda.stream(stream):
            feat = torch.zeros((rows, 96), dtype=torch.float32, device="cuda:0")
            regret = torch.zeros((rows, 40), dtype=torch.float32, device="cuda:0")
            vals = torch.zeros(n * a.batch, dtype=torch.float32, device="cuda:0")
        call = lambda: h.sdcfr_traverse(0, a.batch, [t.data_ptr() for t in w], feat.data_ptr(), regret.data_ptr(), rows, 0, vals.data_ptr(), 1, 0)
        first_ms = timed(call)
        entry = dict(nodes=n * 31 * (36 ** R - 1) // 35, rows=rows, first_call_ms=first_ms)
        for name, launches in (("policy_ms", 1), ("walk_ms", 2), ("both_ms", 0)):
            h.debug_sdcfr(launches)
            entry[name] = float(np.median([timed(call) for _ in range(a.repeats)]))
        h.debug_sdcfr(0)
        rec["launch_ms"][f"R{R}_decks{n}"] = entry
        flush()
        h.close()

    # ---- an iteration, the average policy ----
    train, held, acts3 = decks[:8], decks[64:72], tuple(acts[:18])

    def deep():
        t = FullChanceMCCFRTrainer(decks=train, root_actions=acts3, capacity_log2=4, batch=1, ctx=ctx)
        return FullChanceDeepCFR(t, batch=a.batch), t

    d, t = deep()
    d.train(2, advantage_epochs=a.epochs)
    stream.synchronize()
    t0 = time.perf_counter()
    d.train(5, advantage_epochs=a.epochs)
    stream.synchronize()
    rec["iteration_ms"] = dict(decks=8, R=3, per_iteration=(time.perf_counter() - t0) / 5 * 1e3, rows_per_iteration=2 * rows_per_traversal(3) * 8 * a.batch)
    with torch.cuda.stream(stream):
        for p in range(2):
            while len(d.strategy_buffers[p]._slots) < a.snapshots:
                d.strategy_buffers[p].add_strategy(d.advantage_nets[p].net, len(d.strategy_buffers[p]._slots), d.advantage_nets[p].param_list())
    stream.synchronize()
    d._average_nodes(0)
    t0 = time.perf_counter()
    n_nodes = sum(len(d._average_nodes(p)[0]) for p in range(2))
    t1 = time.perf_counter()
    keys, _, _ = d.policy_rows()
    rec["average_ms"] = dict(snapshots=a.snapshots, nodes=n_nodes, both_players=(t1 - t0) * 1e3, policy_rows=(time.perf_counter() - t1) * 1e3, distinct_pairs=len(keys))
    flush()
    t.close()

    # ---- generalisation ----
    def measure(trainer):
        return dict(train=trainer.exploitability()["exploitability"], held_out=trainer.exploitability(decks=held)["exploitability"])

    t = FullChanceMCCFRTrainer(decks=train, root_actions=acts3, capacity_log2=4, batch=1, ctx=ctx)
    rec["generalisation"]["uniform"] = measure(t)
    t.close()

    d, t = deep()
    wall, its = 0.0, 0
    while wall < a.budget_s:
        t0 = time.perf_counter()
        d.train(10, advantage_epochs=a.epochs, resume=True)       # the loop index goes on across the calls: a snapshot an iteration from the second on
        stream.synchronize()
        wall += time.perf_counter() - t0
        its += 10
    s = d.policy_store()
    h = d.policy_store(decks=held)
    rec["generalisation"]["deep_cfr"] = dict(iterations=its, wall_s=wall, train=s.exploitability()["exploitability"],
                                             held_out=h.exploitability(decks=held)["exploitability"], rows_train=int(s.counters()["rows"]),
                                             rows_held_out=int(h.counters()["rows"]), snapshots=[len(b._slots) for b in d.strategy_buffers],
                                             snapshot_weights=[[b.weights[0], b.weights[-1]] for b in d.strategy_buffers], losses=[x[-1] for x in d.training_history["losses"]])
    s.close(), h.close(), t.close()
    flush()

    for name, step in (("mccfr", lambda tr: tr.train(10)), ("dcfr", lambda tr: tr.solve_cfr(5, variant="dcfr", alpha=1.5, beta=0.0, gamma=2.0))):
        tr = FullChanceMCCFRTrainer(decks=train, root_actions=acts3, capacity_log2=22, batch=a.batch, ctx=ctx)
        wall, chunks = 0.0, 0
        while wall < a.budget_s:
            t0 = time.perf_counter()
            step(tr)
            ctx.synchronize()
            wall += time.perf_counter() - t0
            chunks += 1
        rec["generalisation"][name] = dict(iterations=chunks * (10 if name == "mccfr" else 5), wall_s=wall, rows=int(tr.counters()["rows"]), **measure(tr))
        tr.close()
        flush()
    print(flush())
    ctx.close()


if __name__ == "__main__":
    main()
