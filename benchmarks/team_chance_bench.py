#!/usr/bin/env python3
"""Team MiniScopa over a set of deals (scopa_team_chance_*): time per iteration and per launch kind, next to n x the one-deal solver, and the
exploitability curves of CFR+ and DCFR on the 24-deal packet game.  Prints one JSON line and writes it to --out.

    python benchmarks/team_chance_bench.py [--iters 50] [--warmup 5] [--curve-iters 60] [--check-every 10] [--out profiles/team_chance_bench.json]

sizes       n = 6 (packet_deals(fix_seat0=True)) and n = 24 (packet_deals), the packets below.
device      `iteration_us`: HIP events on the context's stream around one scopa_team_chance_cfr_iterate call of --iters iterations after --warmup (six
            launches per iteration, no host synchronisation inside), divided by --iters.  `launch_us`: the same around --iters single launches of each of
            the three kernels (scopa_team_chance_cfr_launch: subtrees, tops, reduce), per traverser.  `exploitability_ms`: one call, host clock.
one deal    `one_deal_iteration_us`: scopa_team_cfr_iterate on deal 0 of the set, timed the same way in the same run; `n_times_one_deal_us` = n x that.
bytes       `bytes_per_iteration`: stated from the code (scopa_team_chance.hip), both traversals: per deal every row's map entry (4 B) and sigma row
            (32 B) are read once by the subtree and top workgroups, the four ancestor rows again per subtree (256 x 4 x 36 B), every depth-12 payoff byte once,
            the 256 subtree values cross once each way; a traverser's row writes 64 B into the increment image and the reduce reads them back with the
            occurrence id (4 B); per global row of the traverser's team the reduce reads the key and the occurrence offset (12 B), reads and writes the
            regret and strategy rows (128 B) and writes the sigma row (32 B).
curves      `curves[variant]`: [(iteration, exploitability), ...] of algorithms.team_chance.solve on the 24-deal game, every --check-every iterations.
The tables are not compared here: tests/test_gpu_team_chance.py holds the kernels to the restatement."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PACKETS = [[0, 5, 10, 15], [1, 4, 11, 14], [2, 7, 8, 13], [3, 6, 9, 12]]
N_CHOICE, N_LEAVES = 321365, 331776
TEAM_ROWS = (1 + 4 + 256 + 768 + 20736 + 41472, 16 + 64 + 2304 + 6912 + 82944 + 165888)     # local rows of team 0 (depths 0, 1, 4, 5, 8, 9) and team 1


def bytes_per_iteration(n, team_rows_global):
    total = 0
    for p in (0, 1):
        sweep = n * (N_CHOICE * 36 + 256 * 4 * 36 + N_LEAVES + 256 * 8 * 2 + 8)
        image = n * TEAM_ROWS[p] * (64 + 64 + 4)
        reduce_rows = team_rows_global[p] * (12 + 128 + 32)
        total += sweep + image + reduce_rows
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--curve-iters", type=int, default=60)
    ap.add_argument("--check-every", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from scopa_amd import _lib
    from scopa_amd.algorithms import team_chance
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
        iteration_us = timed(lambda: game.cfr_iterate(a.iters)) / a.iters
        launch_us = {}
        for p in (0, 1):
            for part, name in ((0, "subtrees"), (1, "tops"), (2, "reduce")):
                for _ in range(3):
                    game.cfr_launch(p, part)
                launch_us[f"{name}_traverser{p}"] = timed(lambda: [game.cfr_launch(p, part) for _ in range(a.iters)]) / a.iters
        game.exploitability()
        t0 = time.perf_counter()
        expl = game.exploitability()
        exploitability_ms = 1e3 * (time.perf_counter() - t0)
        ctx.team_set_deal(perms[0])
        ctx.team_cfr_iterate(a.warmup, root_values=False)
        one_us = timed(lambda: ctx.team_cfr_iterate(a.iters, root_values=False)) / a.iters
        bpi = bytes_per_iteration(n, rows_global)
        sizes[str(n)] = dict(n=n, G=game.G, rows_of_team=rows_global, increment_image_bytes=n * N_CHOICE * 64, iteration_us=iteration_us, launch_us=launch_us,
                             launches_per_iteration=6, one_deal_iteration_us=one_us, n_times_one_deal_us=n * one_us, ratio_to_n_one_deal=iteration_us / (n * one_us),
                             bytes_per_iteration=bpi, effective_GBps=bpi / iteration_us * 1e-3, exploitability_ms_host_clock=exploitability_ms,
                             exploitability_after_timing=float(expl[0]))
        game.close()

    curves = {}
    for variant in ("cfr+", "dcfr"):
        game, _, curve = team_chance.solve(team_chance.packet_deals(PACKETS), variant, eps=0.0, max_iters=a.curve_iters, check_every=a.check_every, device=ctx)
        curves[variant] = curve
        game.close()
    rec = dict(bench="team_chance", packets=PACKETS, iters=a.iters, warmup=a.warmup, device=torch.cuda.get_device_name(0), sizes=sizes, curves_n24=curves)
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
