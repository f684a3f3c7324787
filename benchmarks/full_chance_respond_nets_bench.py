#!/usr/bin/env python3
"""The sampled best response to the Deep CFR nets on FullScopa over decks (scopa_full_chance_respond_nets_iterate; FullChanceDeepCFR.sampled_response /
.sampled_lower_bound): what an iteration costs beside the store route where a store of the nets' policy fits, what it costs where none does, and the
figure it exists for -- a lower bound on the exploitability of nets trained from the deal, measured from the deal.  Prints one JSON line and writes
it to --out (rewritten after every stage).

    python benchmarks/full_chance_respond_nets_bench.py [--seed 42] [--repeats 5] [--stages both,only,bound] [--budget-s 40] [--many 1024]
                                                        [--respond 10,100,200] [--episodes 32768] [--out profiles/full_chance_respond_nets_bench.json]

Every figure is from ONE run of this script, one process, timed with HIP events on the context's stream; medians of --repeats.  No threshold anywhere.
both    R = 3 on 8 decks (18 plies of random play on the deck of --seed, packet_decks(deck, 3, 8, 1)), batch 64, 10 random snapshots a player:
        `nets_ms` = one respond_nets_iterate iteration, `store_ms` = one respond_iterate iteration against policy_store() in the same process,
        both stores warm; `store_build_ms` = policy_store() itself, stated apart.  Both routes walk the same number of nodes.
only    R = 5 (6 plies played, batch 8) and the deal (batch 1) on 8 decks at 1, 10 and 100 random snapshots: `iteration_ms` = one
        respond_nets_iterate iteration (two launches' worth of levels and two applies); `rest_ms` = the same iteration WITHOUT snapshots, where
        average_at is not launched (uniform play: other paths, the same node counts); `average_at_ms` = their difference; `opponent_nodes` the
        pairs average_at evaluated; `tflops` = opponent_nodes x snapshots x 46 080 flop over average_at_ms, to set beside the 64 - 84 TFLOP/s
        average_at has shown on long lists; `frontier_ms` = sdcfr_traverse_frontier for both players at the same batch and decks (one net a
        player, whatever the snapshot count, and float32 rows instead of float64 atomics).
bound   nets trained as profiles/full_chance_net_match_bench.json's `use` trained them (traversal="frontier" from the deal on --many decks,
        decks_per_iteration=8, batch 1, train_backend="hip", --budget-s seconds of train() calls); ONE responder on the first 8 training decks at
        batch 1, trained on and hardened at each count of --respond, per count the responder's reward over --episodes episodes
        (response_report), beside the same nets' match against uniform play on those decks.  Then the same bound at a round-3 root (8 decks of
        the packet, batch 64, 100 response iterations) beside the exact br0, br1 and (br0 + br1) / 2 of exploitability(root_actions=...)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(128, 96), (128,), (64, 128), (64,), (40, 64), (40,)]
FLOP_PER_PAIR = 2 * (96 * 128 + 128 * 64 + 64 * 40)          # 46 080: the three layers of one snapshot on one pair


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--stages", default="both,only,bound")
    ap.add_argument("--budget-s", type=float, default=40.0)
    ap.add_argument("--many", type=int, default=1024)
    ap.add_argument("--respond", default="10,100,200")
    ap.add_argument("--response-capacity-log2", type=int, default=28)
    ap.add_argument("--episodes", type=int, default=1 << 15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    stages = set(a.stages.split(","))
    import torch
    from scopa_amd import _lib
    from scopa_amd.algorithms import FullChanceMCCFRTrainer, packet_decks
    from scopa_amd.algorithms.deep_cfr import FullChanceDeepCFR
    stream = torch.cuda.Stream()
    ctx = _lib.Context(0, stream=stream.cuda_stream)
    ctx.mccfr_seed(0x5C09A)
    deck = _lib.full_deal_py_seed(a.seed)
    rng = np.random.RandomState(0)
    late, prefix = _lib.FullState(deck=deck), []
    for _ in range(18):
        legal = late.legal()
        prefix.append(int(legal[rng.randint(len(legal))]))
        late.step(prefix[-1])
    prefix = tuple(prefix)
    rec = dict(bench="full_chance_respond_nets", runs=1, seed=a.seed, device=torch.cuda.get_device_name(0), repeats=a.repeats, budget_s=a.budget_s, both={}, only={},
               bound={})
    if a.out and os.path.exists(a.out):                                     # a run of some stages keeps what an earlier run of the others wrote
        try:
            with open(a.out) as f:
                old = json.loads(f.read())
            for k in ("both", "only", "bound"):
                if k not in stages and old.get(k):
                    rec[k] = old[k]
        except ValueError:
            pass

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

    def median_ms(fn):
        return float(np.median([timed(fn) for _ in range(a.repeats)]))

    def deep_with_snapshots(t, n_snap, batch):
        d = FullChanceDeepCFR(t, batch=batch, traversal="frontier")
        g = torch.Generator(device="cuda:0").manual_seed(7)
        with torch.cuda.stream(stream):
            store = []
            for sh in SHAPES:
                bound = float(np.sqrt(6.0 / (sh[0] + sh[1]))) if len(sh) == 2 else 0.1
                store.append((torch.rand((n_snap,) + sh, generator=g, device="cuda:0", dtype=torch.float32) * 2 - 1) * bound)
            for p in (0, 1):
                for i in range(n_snap):
                    d.strategy_buffers[p].add_strategy(None, i + 1, params=[x[(i + p) % n_snap] for x in store])
        stream.synchronize()
        return d

    # ---- where both routes exist: R = 3 on 8 decks ----
    if "both" in stages:
        decks, batch = packet_decks(deck, 3, 8, 1), 64
        t = FullChanceMCCFRTrainer(decks=decks, root_actions=prefix, capacity_log2=4, batch=1, ctx=ctx)
        d = deep_with_snapshots(t, 10, batch)
        sets = [d._snapshot_set(p) for p in (0, 1)]
        made = []
        build_ms = median_ms(lambda: made.append(d.policy_store()))
        store = made[-1]
        rn = FullChanceMCCFRTrainer(decks=decks, root_actions=prefix, capacity_log2=20, batch=batch, ctx=ctx)
        rs = FullChanceMCCFRTrainer(decks=decks, root_actions=prefix, capacity_log2=20, batch=batch, ctx=ctx)
        rs.solver.cut(0)
        rn.solver.respond_nets_iterate([s[0] for s in sets], batch, 2)      # warm-up: code objects, first touches, most rows claimed
        rs.solver.respond_iterate(store.solver, 0, batch, 2)
        nets, stor = [], []
        for _ in range(a.repeats):                                          # interleaved
            nets.append(timed(lambda: rn.solver.respond_nets_iterate([s[0] for s in sets], batch, 1)))
            stor.append(timed(lambda: rs.solver.respond_iterate(store.solver, 0, batch, 1)))
        rs.solver.cut(-1)
        cut = median_ms(lambda: rs.solver.respond_iterate(store.solver, 0, batch, 1))
        rec["both"] = dict(R=3, decks=8, batch=batch, snapshots=10, nets_runs_ms=nets, store_runs_ms=stor, nets_ms=float(np.median(nets)),
                           store_ms=float(np.median(stor)), store_default_cut_ms=cut, ratio=float(np.median(nets) / np.median(stor)), store_build_ms=build_ms,
                           store_rows=int(store.counters()["rows"]), response_rows=[int(rn.counters()["rows"]), int(rs.counters()["rows"])],
                           dropped=int(rn.counters()["dropped"] + rs.counters()["dropped"]))
        for x in made + [rn, rs, t]:
            x.close()
        del sets
        flush()

    # ---- where only this exists: R = 5 and the deal on 8 decks ----
    if "only" in stages:
        none = [([], [0] * 6, 0, 0)] * 2
        for R, decks, acts, batch in ((5, packet_decks(deck, 1, 8, 1), prefix[:6], 8), (6, packet_decks(deck, 0, 8, 1), (), 1)):
            S = (6 ** R - 1) // 5
            nodes = 8 * batch * 13 * S                                     # the other player's choice nodes of an iteration: 9 S as responder 0, 4 S as responder 1
            t = FullChanceMCCFRTrainer(decks=decks, root_actions=acts, capacity_log2=4, batch=1, ctx=ctx)
            r = FullChanceMCCFRTrainer(decks=decks, root_actions=acts, capacity_log2=26, batch=batch, ctx=ctx)
            r.solver.respond_nets_iterate(none, batch, 2)
            rest = median_ms(lambda: r.solver.respond_nets_iterate(none, batch, 1))
            for n_snap in (1, 10, 100):
                d = deep_with_snapshots(t, n_snap, batch)
                sets = [d._snapshot_set(p) for p in (0, 1)]
                r.solver.respond_nets_iterate([s[0] for s in sets], batch, 1)
                ms = median_ms(lambda: r.solver.respond_nets_iterate([s[0] for s in sets], batch, 1))
                front = median_ms(lambda: [d._traverse_batch_fused(p, batch, sync=False) for p in (0, 1)])
                avg = ms - rest
                rec["only"][f"R{R}_decks8_batch{batch}_snap{n_snap}"] = dict(
                    iteration_ms=ms, rest_ms=rest, average_at_ms=avg, opponent_nodes=nodes, model_flop=nodes * n_snap * FLOP_PER_PAIR,
                    tflops=nodes * n_snap * FLOP_PER_PAIR / (avg * 1e-3) / 1e12 if avg > 0 else None, frontier_ms=front,
                    response_rows=int(r.counters()["rows"]), dropped=int(r.counters()["dropped"]))
                del sets, d
                flush()
            r.close()
            t.close()
            torch.cuda.empty_cache()

    # ---- the figure the feature exists for ----
    if "bound" in stages:
        train = packet_decks(deck, 0, a.many, 1)                             # train[0] is the deck of --seed: the round-3 prefix is played on it
        t = FullChanceMCCFRTrainer(decks=train, root_actions=(), capacity_log2=4, batch=1, ctx=ctx)
        d = FullChanceDeepCFR(t, batch=1, train_backend="hip", traversal="frontier", decks_per_iteration=8)
        wall, its = 0.0, 0
        while wall < a.budget_s:
            t0 = time.perf_counter()
            d.train(5, advantage_epochs=10, resume=True)
            stream.synchronize()
            wall += time.perf_counter() - t0
            its += 5
        bound = dict(decks=len(train), decks_per_iteration=8, batch=1, iterations=its, train_wall_s=wall, snapshots=[len(b._slots) for b in d.strategy_buffers],
                     episodes=a.episodes, response_decks=8, response_batch=1, deal=[])
        on = train[:8]
        ctx.mccfr_seed(0x5C09A)
        m = d.match(a.episodes, decks=on, stream_id=3)
        bound["nets_vs_uniform"] = dict(reward=m["reward"], std_error=m["std_error"], by_seat=[s["reward"] for s in m["by_seat"]])
        rec["bound"] = bound
        flush()
        r, done, spent = None, 0, 0.0
        sets = [d._snapshot_set(p) for p in (0, 1)]
        for target in (int(x) for x in a.respond.split(",")):
            t0 = time.perf_counter()
            if r is None:
                r = d.sampled_response(target, batch=1, capacity_log2=a.response_capacity_log2, decks=on)
            else:
                r._checked(r.solver.respond_nets_iterate, [s[0] for s in sets], 1, target - done)
                r.solver.harden()
            stream.synchronize()
            spent += time.perf_counter() - t0
            done = target
            rep = d.response_report(r, a.episodes, decks=on, stream_id=3)
            bound["deal"].append(dict(response_iterations=done, response_wall_s=spent, reward=rep["reward"], std_error=rep["std_error"],
                                      reward_by_seat=[s["reward"] for s in rep["by_seat"]], response_rows=int(r.counters()["rows"]),
                                      dropped=int(r.counters()["dropped"])))
            flush()
        r.close()
        del sets
        torch.cuda.empty_cache()
        sub = packet_decks(deck, 3, 8, 1)
        t0 = time.perf_counter()
        rep = d.sampled_lower_bound(100, a.episodes, batch=64, capacity_log2=22, decks=sub, root_actions=prefix, stream_id=3)
        e = d.exploitability(decks=sub, root_actions=prefix)
        bound["round3"] = dict(decks=8, response_iterations=100, response_batch=64, wall_s=time.perf_counter() - t0, reward=rep["reward"], std_error=rep["std_error"],
                               reward_by_seat=[s["reward"] for s in rep["by_seat"]], exact_reward=rep["exact_reward"], exact_by_seat=rep["exact_by_seat"],
                               br0=e["br0"], br1=e["br1"], exact_exploitability=e["exploitability"], value=e["value"])
        t.close()
        flush()
    print(flush())
    ctx.close()


if __name__ == "__main__":
    main()
