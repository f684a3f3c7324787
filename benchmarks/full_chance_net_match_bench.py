#!/usr/bin/env python3
"""The Deep CFR nets of FullScopa over decks in sampled matches (scopa_full_chance_sdcfr_average_at, scopa_full_chance_sdcfr_match;
FullChanceDeepCFR.average_policy_at / .match): what the average policy on a list costs beside the route that existed, what a match costs beside
policy_store() + match where a store fits, what it costs where none does, and one use -- nets trained from the deal, measured from the deal.  Prints
one JSON line and writes it to --out (rewritten after every stage, so a run that is cut short leaves what it measured).

    python benchmarks/full_chance_net_match_bench.py [--seed 42] [--repeats 5] [--stages average,grid,match,beyond,use] [--match-snapshots 10]
                                                     [--budget-s 60] [--many 1024] [--use-episodes 32768] [--mccfr-capacity-log2 28] [--out profiles/full_chance_net_match_bench.json]

Every figure is from ONE run of this script, one process, timed with HIP events on the context's stream (the median of --repeats calls after a first
call that allocates).  No threshold is set on any of them.
decks        packet_decks(deck --seed, 0, 72 + --many, 1): decks that share the deal's table; 0..7 the match stages' decks, 64..71 held out, 72.. the
             training decks of the use.  The sub-game roots are the random play (RandomState(0)) on deck 0, which every deck of
             packet_decks(deck, 4, 8, 1) -- the R = 3 and R = 5 stages' decks -- shares for four rounds.
average      lists of 1 << 10, 1 << 14, 1 << 17 key pairs of player 0 (the distinct pairs of the R = 2 sub-game on 8 decks, repeated to length) at 1, 10
             and 100 snapshots of random nets: `average_at_ms` the one launch; `route_ms` what existed: per snapshot one policy_at launch and a torch
             accumulate (acc += coef * p in float32, the product and the sum rounded separately as the library rounds them), then a torch
             normalisation in float64; `ratio` = average_at / route; `tflops` by the 46 080 flop / pair / snapshot model (`of_peak` against the
             157 TFLOP/s float32 matrix peak); `rows_equal`: the two routes' rows compared bit for bit (the run stops where they differ).
grid         the sweep behind the library's grid rule: average_at at 100 snapshots on lists of 1 << 10, 14, 17, 20 pairs under forced workgroup counts
             (scopa_full_chance_debug_sdcfr_average_grid; median of 3): `rule` the library's own choice, `wgN` N workgroups.
match        R = 3 on 8 decks, --match-snapshots snapshots a player, uniform opponent, 1 << 16 and 1 << 20 episodes: `match_ms` the nets' match;
             `store_build_ms` policy_store() (the forest's average policy, the rows to the host and into a store), `store_match_ms` match on it,
             `store_route_ms` their sum, `ratio` = match / store route.  A match evaluates 2 R pairs an episode (the agent's choice levels: two a
             round), so 46 080 x snapshots x 2 R flop an episode.
beyond       the same match at R = 5 and from the deal (R = 6), where no store fits: time, episodes / s, TFLOP/s by that model.
use          nets trained traversal="frontier" from the deal on --many decks, decks_per_iteration=8, batch 1, train_backend="hip", for --budget-s
             seconds of wall time in train() calls; their reward over --use-episodes episodes from the deal against uniform play and against an
             MCCFR store of 100 iterations (8 sampled decks an iteration, batch 1) on the same decks, on the first 64 training decks and on the 8
             held-out decks, with the sampled standard errors."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FLOP_PER_PAIR = 46080
PEAK_TFLOPS = 157.0
SHAPES = ((128, 96), (128,), (64, 128), (64,), (40, 64), (40,))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--stages", default="average,grid,match,beyond,use")
    ap.add_argument("--match-snapshots", type=int, default=10)
    ap.add_argument("--budget-s", type=float, default=60.0)
    ap.add_argument("--many", type=int, default=1024)
    ap.add_argument("--use-episodes", type=int, default=32768)
    ap.add_argument("--mccfr-capacity-log2", type=int, default=28)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    stages = set(a.stages.split(","))
    import torch
    from scopa_amd import _lib
    from scopa_amd.algorithms import FullChanceMCCFRTrainer, packet_decks
    from scopa_amd.algorithms.deep_cfr import FullChanceDeepCFR
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import full_chance_ref as W
    import full_mccfr_ref as F
    stream = torch.cuda.Stream()
    ctx = _lib.Context(0, stream=stream.cuda_stream)
    ctx.mccfr_seed(0x5C09A)
    deck = _lib.full_deal_py_seed(a.seed)
    _, acts = F.random_root(deck, 4, np.random.RandomState(0))
    decks = packet_decks(deck, 0, 72 + a.many, 1)
    sub_decks = packet_decks(deck, 4, 8, 1)

    rec = dict(bench="full_chance_net_match", runs=1, seed=a.seed, device=torch.cuda.get_device_name(0), repeats=a.repeats, match_snapshots=a.match_snapshots,
               budget_s=a.budget_s, average={}, grid={}, match={}, beyond={}, use={})
    if a.out and os.path.exists(a.out):                                     # a run of some stages keeps what an earlier run of the others wrote
        try:
            with open(a.out) as f:
                old = json.loads(f.read())
            for k in ("average", "grid", "match", "beyond", "use"):
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
        first = timed(fn)
        return first, float(np.median([timed(fn) for _ in range(a.repeats)]))

    def random_store(n_snap, seed):
        g = torch.Generator(device="cuda:0").manual_seed(seed)
        with torch.cuda.stream(stream):
            store = []
            for sh in SHAPES:
                bound = float(np.sqrt(6.0 / (sh[0] + sh[1]))) if len(sh) == 2 else 0.1
                store.append((torch.rand((n_snap,) + sh, generator=g, device="cuda:0", dtype=torch.float32) * 2 - 1) * bound)
            w = np.arange(1, n_snap + 1, dtype=np.float64)
            coef = torch.tensor((w / w.sum()).astype(np.float32), device="cuda:0")
        stream.synchronize()
        return store, coef

    # ---- average_at against n_snap policy_at launches + a torch accumulate + a torch normalisation ----
    if "average" in stages:
        pairs = W.subgame_keys(F.root_of(deck, acts), sub_decks)
        pairs = pairs[((pairs[:, 0] >> np.uint64(62)) & np.uint64(1)) == 0]
        for n_snap in (1, 10, 100):
            store, coef = random_store(n_snap, 100 + n_snap)
            ptrs = [t.data_ptr() for t in store]
            coef_host = coef.cpu().tolist()
            for lg in (10, 14, 17):
                n = 1 << lg
                with torch.cuda.stream(stream):
                    k = torch.tensor(np.resize(pairs, (n, 2)).view(np.int64), device="cuda:0")
                    out = torch.empty((n, 3), dtype=torch.float64, device="cuda:0")
                    pol = torch.empty((n, 3), dtype=torch.float32, device="cuda:0")
                    thr = torch.empty((n, 2), dtype=torch.int64, device="cuda:0")
                    acc = torch.empty((n, 3), dtype=torch.float32, device="cuda:0")
                    bits = k[:, 1:2]
                    n_held = sum(((bits >> c) & 1) for c in range(40)).clamp(max=3)
                    uniform = (torch.arange(3, device="cuda:0")[None, :] < n_held).double() / n_held.double()
                stream.synchronize()
                slots = list(range(n_snap))

                def one():
                    ctx.full_chance_sdcfr_average_at(0, k.data_ptr(), n, slots, ptrs, n_snap, coef.data_ptr(), out.data_ptr())

                def route():
                    with torch.cuda.stream(stream):
                        acc.zero_()
                        for i in range(n_snap):
                            ctx.full_chance_sdcfr_policy_at(0, k.data_ptr(), n, [t[i].data_ptr() for t in store], pol.data_ptr(), thr.data_ptr())
                            acc.add_(pol * coef_host[i])                 # a rounded product, then a rounded sum: two launches, the library's two operations
                        x = acc.double()
                        s = (x[:, 0:1] + x[:, 1:2]) + x[:, 2:3]          # the library's order
                        return torch.where(s > 0, x / s, uniform)

                first, ms = median_ms(one)
                _, route_ms = median_ms(route)
                with torch.cuda.stream(stream):
                    same = bool(torch.equal(out, route()))                # the two routes are timed on the same rows, bit for bit
                assert same, "average_at and the policy_at route disagree"
                tflops = n * n_snap * FLOP_PER_PAIR / (ms * 1e-3) / 1e12
                rec["average"][f"pairs{n}_snap{n_snap}"] = dict(first_call_ms=first, average_at_ms=ms, route_ms=route_ms, ratio=ms / route_ms, tflops=tflops,
                                                                 of_peak=tflops / PEAK_TFLOPS, rows_equal=same)
                flush()
            del store, coef
        torch.cuda.empty_cache()

    # ---- the grid rule's sweep: average_at at 100 snapshots under forced workgroup counts ----
    if "grid" in stages:
        pairs = W.subgame_keys(F.root_of(deck, acts), sub_decks)
        pairs = pairs[((pairs[:, 0] >> np.uint64(62)) & np.uint64(1)) == 0]
        n_snap = 100
        store, coef = random_store(n_snap, 200)
        ptrs = [t.data_ptr() for t in store]
        for lg in (10, 14, 17, 20):
            n = 1 << lg
            tiles = n // 16
            with torch.cuda.stream(stream):
                k = torch.tensor(np.resize(pairs, (n, 2)).view(np.int64), device="cuda:0")
                out = torch.empty((n, 3), dtype=torch.float64, device="cuda:0")
            stream.synchronize()
            one = lambda: ctx.full_chance_sdcfr_average_at(0, k.data_ptr(), n, list(range(n_snap)), ptrs, n_snap, coef.data_ptr(), out.data_ptr())
            entry = {}
            grids = sorted({max(1, tiles // t) for t in (1, 2, 4, 8, 16, 32, 64)} | {g for g in (256, 512, 1024, 2048, 4096) if g <= tiles})
            try:
                for g in [0] + grids:                                       # 0: the library's rule
                    ctx.full_chance_debug_sdcfr_average_grid(g)
                    timed(one)
                    ms = float(np.median([timed(one) for _ in range(3)]))
                    entry["rule" if g == 0 else f"wg{g}"] = dict(ms=ms, tiles_per_wg=None if g == 0 else tiles / g, us_per_snapshot=1e3 * ms / n_snap,
                                                                  tflops=n * n_snap * FLOP_PER_PAIR / (ms * 1e-3) / 1e12)
            finally:
                ctx.full_chance_debug_sdcfr_average_grid(0)
            rec["grid"][f"pairs{n}_snap{n_snap}"] = entry
            flush()
        del store, coef
        torch.cuda.empty_cache()

    def deep_with_snapshots(t, n_snap):
        d = FullChanceDeepCFR(t, batch=1, traversal="frontier")
        store, _ = random_store(n_snap, 7)
        with torch.cuda.stream(stream):
            for p in (0, 1):
                for i in range(n_snap):
                    d.strategy_buffers[p].add_strategy(None, i, params=[x[(i + p) % n_snap] for x in store])
        stream.synchronize()
        return d

    def match_entry(d, n, R):
        sets = [d._snapshot_set(p) for p in (0, 1)]
        first, ms = median_ms(lambda: d.solver.sdcfr_match(n, [s[0] for s in sets], None, 1))
        flop = n * 2 * R * a.match_snapshots * FLOP_PER_PAIR
        tflops = flop / (ms * 1e-3) / 1e12
        return dict(first_call_ms=first, match_ms=ms, episodes_per_s=n / (ms * 1e-3), pairs=n * 2 * R, tflops=tflops, of_peak=tflops / PEAK_TFLOPS,
                    launches_per_chunk=1 + 2 * 4 * R)

    # ---- the match beside policy_store() + match, R = 3 on 8 decks ----
    if "match" in stages:
        t = FullChanceMCCFRTrainer(decks=sub_decks, root_actions=tuple(acts[:18]), capacity_log2=4, batch=1, ctx=ctx)
        d = deep_with_snapshots(t, a.match_snapshots)
        for lg in (16, 20):
            n = 1 << lg
            entry = match_entry(d, n, 3)
            made = []

            def build():
                made.append(d.policy_store())

            _, entry["store_build_ms"] = median_ms(build)
            _, entry["store_match_ms"] = median_ms(lambda: made[-1].solver.match(n, 1))
            entry["store_rows"] = int(made[-1].counters()["rows"])
            for s in made:
                s.close()
            entry["store_route_ms"] = entry["store_build_ms"] + entry["store_match_ms"]
            entry["ratio"] = entry["match_ms"] / entry["store_route_ms"]
            rec["match"][f"R3_decks8_episodes{n}"] = entry
            flush()
        t.close()

    # ---- the match where no store fits ----
    if "beyond" in stages:
        for R, train, prefix in ((5, sub_decks, tuple(acts[:6])), (6, decks[:8], ())):
            t = FullChanceMCCFRTrainer(decks=train, root_actions=prefix, capacity_log2=4, batch=1, ctx=ctx)
            d = deep_with_snapshots(t, a.match_snapshots)
            for lg in (16, 20):
                rec["beyond"][f"R{R}_decks8_episodes{1 << lg}"] = match_entry(d, 1 << lg, R)
                flush()
            t.close()
        torch.cuda.empty_cache()

    # ---- one use: trained from the deal, measured from the deal ----
    if "use" in stages:
        train, held = decks[72:], decks[64:72]
        t = FullChanceMCCFRTrainer(decks=train, root_actions=(), capacity_log2=4, batch=1, ctx=ctx)
        d = FullChanceDeepCFR(t, batch=1, train_backend="hip", traversal="frontier", decks_per_iteration=8)
        wall, its = 0.0, 0
        while wall < a.budget_s:
            t0 = time.perf_counter()
            d.train(5, advantage_epochs=10, resume=True)
            stream.synchronize()
            wall += time.perf_counter() - t0
            its += 5
        m = FullChanceMCCFRTrainer(decks=train, root_actions=(), capacity_log2=a.mccfr_capacity_log2, batch=1, ctx=ctx)
        t0 = time.perf_counter()
        m.train(100, sample=8, seed=1)
        mccfr_s = time.perf_counter() - t0
        use = dict(decks=len(train), decks_per_iteration=8, batch=1, iterations=its, train_wall_s=wall, snapshots=[len(b._slots) for b in d.strategy_buffers],
                   losses=[x[-1] for x in d.training_history["losses"]], episodes=a.use_episodes, mccfr_iterations=100, mccfr_wall_s=mccfr_s,
                   mccfr_rows=int(m.counters()["rows"]))
        ctx.mccfr_seed(0x5C09A)
        for where, on in (("train", train[:64]), ("held_out", held)):
            for who, opp in (("uniform", None), ("mccfr_100", m)):
                t0 = time.perf_counter()
                r = d.match(a.use_episodes, opponent=opp, decks=on, stream_id=3)
                use[f"{where}_vs_{who}"] = dict(reward=r["reward"], std_error=r["std_error"], nets_scopas=r["a_scopas"], opponent_scopas=r["b_scopas"],
                                                by_seat=[s["reward"] for s in r["by_seat"]], wall_s=time.perf_counter() - t0)
            r = m.evaluate_vs_random(a.use_episodes, decks=on, stream_id=3)
            use[f"{where}_mccfr_100_vs_uniform"] = dict(reward=r[0], std_error=r[1])
        rec["use"] = use
        m.close()
        t.close()
        flush()
    print(flush())
    ctx.close()


if __name__ == "__main__":
    main()
