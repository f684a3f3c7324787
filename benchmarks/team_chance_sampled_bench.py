#!/usr/bin/env python3
"""Team MiniScopa over a set of deals, deal-sampled and simultaneous iterations (scopa_team_chance_cfr_iterate_sampled): time per iteration at
m = n, n/2 and n/4 listed deals, alternating and simultaneous, next to scopa_team_chance_cfr_iterate in the same process, and the exploitability
after an equal number of deal sweeps.  Prints one JSON line and writes it to --out.

    python benchmarks/team_chance_sampled_bench.py [--iters 50] [--warmup 5] [--sweeps 960] [--out profiles/team_chance_sampled_bench.json]

sizes       n = 6 (packet_deals(fix_seat0=True)) and n = 24 (packet_deals), the packets below.
device      `cfr_iterate_us`: HIP events on the context's stream around one scopa_team_chance_cfr_iterate call of --iters iterations after --warmup,
            divided by --iters.  `sampled[m][alternating]`: the same around one cfr_iterate_sampled call whose lists are
            chance.sample_deals(n, m, 0, iters, seed 1) (m = n: every deal, listed), `iteration_us` and its ratio to `cfr_iterate_us`.  `all_deals`: the
            call without a list (no marking launch, no table lookups).  All in one process, one handle per size.  The sampled call uploads its lists and
            synchronises the stream once before its first launch; that is inside its window.
bytes       `reduce_bytes[m]`: stated from the code (k_team_chance_reduce_sampled), both teams: per global row the key and the occurrence offset
            (12 B), the regret and strategy rows read and written (128 B), the sigma row written (32 B); per occurrence of the row, listed or not, its
            id (4 B) and its deal's entry of the mark table (4 B, a table of n entries); per LISTED occurrence the 64-byte increment row.  Only the
            last term falls with m: the launch has a lane per global row and walks every occurrence id.
curves      `exploitability_at_equal_sweeps[m]`: [(deal sweeps = iterations x m, exploitability), ...] of algorithms.team_chance.solve with
            DCFR(1.5, 0, 2) on the 24-deal game, full and sample = n/2 and n/4 (seed 1), checked every 240 deal sweeps up to --sweeps.
The tables are not compared here: tests/test_gpu_team_chance_sampled.py holds the kernels to the restatement."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PACKETS = [[0, 5, 10, 15], [1, 4, 11, 14], [2, 7, 8, 13], [3, 6, 9, 12]]
TEAM_ROWS = (1 + 4 + 256 + 768 + 20736 + 41472, 16 + 64 + 2304 + 6912 + 82944 + 165888)     # local rows of team 0 (depths 0, 1, 4, 5, 8, 9) and team 1


def reduce_bytes(n, m, rows_global):
    return sum(rows_global[p] * (12 + 128 + 32) + n * TEAM_ROWS[p] * 8 + m * TEAM_ROWS[p] * 64 for p in (0, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sweeps", type=int, default=960)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from scopa_amd import _lib
    from scopa_amd.algorithms import team_chance
    from scopa_amd.algorithms.chance import sample_deals
    stream = torch.cuda.Stream()
    ctx = _lib.Context(0, stream=stream.cuda_stream)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        stream.synchronize()
        return e0.elapsed_time(e1) * 1e3        # us

    sizes = {}
    for n, perms in ((6, team_chance.packet_deals(PACKETS, fix_seat0=True)), (24, team_chance.packet_deals(PACKETS))):
        game = _lib.TeamChanceGame(perms, ctx)
        keys, _ = game.index()
        team = ((keys >> np.uint64(60)).astype(np.int64) & 3) >> 1
        rows_global = (int(np.count_nonzero(team == 0)), int(np.count_nonzero(team == 1)))
        game.cfr_iterate(a.warmup)
        exact_us = timed(lambda: game.cfr_iterate(a.iters)) / a.iters
        sampled, all_deals = {}, {}
        for alternating in (1, 0):
            game.cfr_iterate_sampled(None, a.warmup, alternating=alternating)
            us = timed(lambda: game.cfr_iterate_sampled(None, a.iters, alternating=alternating)) / a.iters
            all_deals[f"alternating{alternating}"] = dict(iteration_us=us, ratio_to_cfr_iterate=us / exact_us)
        for m in (n, n // 2, n // 4):
            warm, lists = sample_deals(n, m, 0, a.warmup, 1), sample_deals(n, m, 0, a.iters, 1)
            row = {}
            for alternating in (1, 0):
                game.cfr_iterate_sampled(warm, alternating=alternating)
                us = timed(lambda: game.cfr_iterate_sampled(lists, alternating=alternating)) / a.iters
                row[f"alternating{alternating}"] = dict(iteration_us=us, ratio_to_cfr_iterate=us / exact_us)
            row["reduce_bytes"] = reduce_bytes(n, m, rows_global)
            sampled[str(m)] = row
        exact_again_us = timed(lambda: game.cfr_iterate(a.iters)) / a.iters
        sizes[str(n)] = dict(n=n, G=game.G, rows_of_team=rows_global, cfr_iterate_us=exact_us, cfr_iterate_us_at_the_end=exact_again_us, all_deals=all_deals, sampled=sampled)
        game.close()

    curves, n = {}, 24
    for m in (n, n // 2, n // 4):
        iters, every = a.sweeps // m, 240 // m
        game, _, curve = team_chance.solve(team_chance.packet_deals(PACKETS), "dcfr", eps=0.0, max_iters=iters, check_every=every, device=ctx,
                                           sample=None if m == n else m, seed=1, alpha=1.5, beta=0.0, gamma=2.0)
        curves[str(m)] = [(t * m, e) for t, e in curve]
        game.close()
    rec = dict(bench="team_chance_sampled", packets=PACKETS, iters=a.iters, warmup=a.warmup, device=torch.cuda.get_device_name(0), sizes=sizes,
               exploitability_at_equal_sweeps_n24=curves)
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
