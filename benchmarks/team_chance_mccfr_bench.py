#!/usr/bin/env python3
"""Deal-sampled external-sampling MCCFR on Team MiniScopa over a set of deals (scopa_team_chance_mccfr_*): time per iteration, split into the walk launch
and the apply launch, next to the two things it can be measured against in the same run.  Prints one JSON line and writes it to --out.

    python benchmarks/team_chance_mccfr_bench.py [--iters 100] [--warmup 10] [--out profiles/team_chance_mccfr_bench.json]
                                                 [--one-deal-parent a.json,b.json,c.json --one-deal-this d.json,e.json,f.json]

sizes       n = 6 (packet_deals(fix_seat0=True)) and n = 24 (packet_deals), the packets below.  Every figure of a size is from ONE process.
all deals   per batch B in (64, 1024): `iteration_us`: HIP events on the context's stream around one scopa_team_chance_mccfr_iterate call of k
            iterations after --warmup (two launches per iteration, no host synchronisation inside), divided by k; k = --iters at B = 64 and is scaled
            down with B (at least 10).  `walk_us` / `apply_us`: the same around each of k scopa_team_chance_mccfr_walk launches and the apply that
            follows it (an apply on an empty delta buffer would skip every row).
sampled     `sampled_half`: B = 64 with m = n / 2 deals per iteration, chance.sample_deals(n, m, t, k, seed): `iteration_us` around one iterate call
            with its k lists (uploaded once, inside the window); the split with the list of the first iteration kept for every launch (a list the
            device already holds is not uploaded again).
baselines   `cfr_iteration_us`: scopa_team_chance_cfr_iterate on the same handle, same timing.  `one_deal_iteration_us[B]`: scopa_team_mccfr_iterate(B)
            on deal 0 of the set on the same context; `n_times_one_deal_us[B]` = n x that: the n one-deal solvers the chance form replaces share no row.
            No ratio is a target: the record states what was measured against what and leaves the judgement to the reader.
one deal    --one-deal-parent / --one-deal-this: records of benchmarks/team_mccfr_bench.py run alternately at the parent commit and at this one on one
            machine (the walk is one definition shared with the one-deal kernel since this solver exists); kept as `one_deal_walk_us`: per batch the
            runs' walk-launch times, their mean and their spread (max - min).
The tables are not compared here: tests/test_gpu_team_chance_mccfr.py holds the kernels to the restatement."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PACKETS = [[0, 5, 10, 15], [1, 4, 11, 14], [2, 7, 8, 13], [3, 6, 9, 12]]
SEED = 0x5C09A


def one_deal_walks(files):
    out = {}
    for f in files:
        with open(f) as fh:
            rec = json.loads(fh.readline())
        for B, r in rec["batched"].items():
            out.setdefault(B, []).append(r["walk_us"])
    return {B: dict(runs=v, mean=sum(v) / len(v), spread=max(v) - min(v)) for B, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--one-deal-parent", default=None)
    ap.add_argument("--one-deal-this", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from scopa_amd import _lib
    from scopa_amd.algorithms import team_chance
    from scopa_amd.algorithms.chance import sample_deals
    stream = torch.cuda.Stream()
    ctx = _lib.Context(0, stream=stream.cuda_stream)
    ctx.mccfr_seed(SEED)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        stream.synchronize()
        return e0.elapsed_time(e1) * 1e3        # us

    def split(game, B, k, deals):
        """(walk_us, apply_us): events around each of k walk launches and the apply after it"""
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3 * k)]
        it0 = game.mccfr_counters()[2]
        game.mccfr_walk(it0, B, deals)
        game.mccfr_apply()
        for j in range(k):
            ev[3 * j].record(stream)
            game.mccfr_walk(it0 + 1 + j, B, deals)
            ev[3 * j + 1].record(stream)
            game.mccfr_apply()
            ev[3 * j + 2].record(stream)
        stream.synchronize()
        return (sum(ev[3 * j].elapsed_time(ev[3 * j + 1]) for j in range(k)) * 1e3 / k, sum(ev[3 * j + 1].elapsed_time(ev[3 * j + 2]) for j in range(k)) * 1e3 / k)

    sizes = {}
    for n, perms in ((6, team_chance.packet_deals(PACKETS, fix_seat0=True)), (24, team_chance.packet_deals(PACKETS))):
        game = _lib.TeamChanceGame(perms, ctx)
        all_deals, one_deal = {}, {}
        for B in (64, 1024):
            k = max(10, a.iters * 64 // B)
            game.tables_reset()
            game.mccfr_iterate(B, min(a.warmup, k))
            it_us = timed(lambda: game.mccfr_iterate(B, k)) / k
            walk_us, apply_us = split(game, B, k, None)
            all_deals[str(B)] = dict(iterations_timed=k, iteration_us=it_us, walk_us=walk_us, apply_us=apply_us, traversal_pairs_per_iteration=n * B,
                                     pairs_per_s=n * B / it_us * 1e6)
        m, k = n // 2, a.iters
        game.tables_reset()
        t0 = game.mccfr_counters()[2]
        game.mccfr_iterate(64, a.warmup, sample_deals(n, m, t0, a.warmup, SEED))
        lists = sample_deals(n, m, t0 + a.warmup, k, SEED)
        it_us = timed(lambda: game.mccfr_iterate(64, k, lists)) / k
        walk_us, apply_us = split(game, 64, k, lists[0])
        sampled = dict(batch=64, m=m, iterations_timed=k, iteration_us=it_us, walk_us=walk_us, apply_us=apply_us, traversal_pairs_per_iteration=m * 64)
        game.tables_reset()
        game.cfr_iterate(a.warmup)
        cfr_us = timed(lambda: game.cfr_iterate(a.iters)) / a.iters
        game.close()
        ctx.team_set_deal(perms[0])
        for B in (64, 1024):
            k = max(10, a.iters * 64 // B)
            ctx.team_tables_reset()
            ctx.team_mccfr_iterate(B, min(a.warmup, k))
            one_deal[str(B)] = timed(lambda: ctx.team_mccfr_iterate(B, k)) / k
        sizes[str(n)] = dict(n=n, G=game.G, all_deals=all_deals, sampled_half=sampled, cfr_iteration_us=cfr_us, one_deal_iteration_us=one_deal,
                             n_times_one_deal_us={B: n * v for B, v in one_deal.items()})
    rec = dict(bench="team_chance_mccfr", packets=PACKETS, seed=SEED, iters=a.iters, warmup=a.warmup, device=torch.cuda.get_device_name(0), launches_per_iteration=2,
               measured_against=["cfr_iteration_us: scopa_team_chance_cfr_iterate on the same handle", "n_times_one_deal_us: n x scopa_team_mccfr_iterate on one deal of the set"],
               sizes=sizes)
    if a.one_deal_parent and a.one_deal_this:
        rec["one_deal_walk_us"] = dict(bench="benchmarks/team_mccfr_bench.py, runs alternated on one machine", parent=one_deal_walks(a.one_deal_parent.split(",")),
                                       this=one_deal_walks(a.one_deal_this.split(",")))
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
