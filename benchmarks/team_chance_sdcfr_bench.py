#!/usr/bin/env python3
"""Deep CFR on Team MiniScopa over a set of deals (scopa_team_chance_sdcfr_*, TeamChanceDeepCFR): the policy launch and the walk launch apart, the
iteration, the average-policy call and the exploitability call, next to a CFR and an MCCFR iteration on the same handle in the same run.  Prints one
JSON line and writes it to --out.

    python benchmarks/team_chance_sdcfr_bench.py [--reps 10] [--wall 20] [--out profiles/team_chance_sdcfr_bench.json]
    python benchmarks/team_chance_sdcfr_bench.py --n 6        # one size, in this process (what the driver above starts, one fresh process per size)

sizes       n = 6 (packet_deals(fix_seat0=True)) and n = 24 (packet_deals), the packets below.  Every figure of a size is from ONE process.
traverse    per batch B in (64, 1024), m in (n, n / 2) and traverser: HIP events on the context's stream around --reps calls that make the policy launch
            alone (`policy_us`), the walk launch alone over those tables (`walk_us`; scopa_team_chance_debug_sdcfr's launches hook) and whole calls
            (`call_us`), each divided by the calls; one ring of 1653 * m * B rows, written again by every call.
iteration   `iteration_us[B]`: TeamChanceDeepCFR(batch=B, memory_size = one iteration's rows where that exceeds 100 000) after one warm-up iteration:
            events around `--iter-reps` queued iterations (both teams' traversal calls, 10 optimiser epochs each, the snapshots), divided by them.
average     `average_policy_us`: events around scopa_team_chance_sdcfr_average_policy for both teams over a store of 100 snapshots of random nets.
expl        `exploitability_us`: wall time of TeamChanceGame.exploitability on that table (the call synchronises).
baselines   `cfr_iteration_us`, `mccfr_iteration_us[B]`: scopa_team_chance_cfr_iterate / _mccfr_iterate on the same handle, events around --reps
            iterations.
curve       n = 6 only: exploitability of DCFR (chunks of 10 iterations) and of TeamChanceDeepCFR(batch=64) after --wall seconds of wall time each,
            exploitability calls not counted.
No ratio is a target: the record states what was measured against what.  tests/test_gpu_team_chance_sdcfr.py holds the kernels to the restatement."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PACKETS = [[0, 5, 10, 15], [1, 4, 11, 14], [2, 7, 8, 13], [3, 6, 9, 12]]
SEED = 0x5C09A
ROWS = 1653


def one_size(n, a):
    import numpy as np
    import torch
    from scopa_amd import _lib
    from scopa_amd.algorithms import schedule, team_chance
    from scopa_amd.algorithms.deep_cfr import TeamChanceDeepCFR
    stream = torch.cuda.Stream()
    ctx = _lib.Context(0, stream=stream.cuda_stream)
    ctx.mccfr_seed(SEED)
    perms = team_chance.packet_deals(PACKETS, fix_seat0=(n == 6))
    assert len(perms) == n
    game = _lib.TeamChanceGame(perms, ctx)

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            fn()
        e1.record(stream)
        stream.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps        # us

    gen = torch.Generator().manual_seed(1)
    shapes, fan = [(128, 34), (128,), (64, 128), (64,), (16, 64), (16,)], [34, 34, 128, 128, 64, 64]
    net = lambda: [(torch.randn(s, generator=gen) / f ** 0.5).cuda().contiguous() for s, f in zip(shapes, fan)]
    image = torch.zeros((2, _lib.lib().scopa_sdcfr_image_floats()), dtype=torch.float32, device="cuda:0")
    nets = [net(), net()]
    torch.cuda.synchronize()
    for p in range(2):
        ctx.sdcfr_pack_weights(p, *(t.data_ptr() for t in nets[p]), image.data_ptr())
    ctx.synchronize()

    traverse = {}
    for B in (64, 1024):
        for m in (n, n // 2):
            deals = None if m == n else list(range(0, n, 2))
            cap = ROWS * m * B
            with torch.cuda.stream(stream):
                feat = torch.empty((cap, 34), dtype=torch.float32, device="cuda:0")
                reg = torch.empty((cap, 16), dtype=torch.float32, device="cuda:0")
                vals = torch.empty(m * B, dtype=torch.float32, device="cuda:0")
            stream.synchronize()
            for trav in (0, 1):
                call = lambda: game.sdcfr_traverse(trav, B, image.data_ptr(), feat.data_ptr(), reg.data_ptr(), 0, cap, 0, vals.data_ptr(), 1, 0, deals)
                call()
                stream.synchronize()
                rec = dict(batch=B, m=m, traverser=trav, rows=cap, call_us=timed(call, a.reps))
                game.debug_sdcfr(launches=1)
                rec["policy_us"] = timed(call, a.reps)
                game.debug_sdcfr(launches=2)
                rec["walk_us"] = timed(call, a.reps)
                game.debug_sdcfr()
                rec["policy_us_per_deal"] = rec["policy_us"] / m
                rec["walk_GBps"] = cap * 200 / rec["walk_us"] / 1e3
                traverse[f"B{B}_m{m}_t{trav}"] = rec
            del feat, reg, vals
            torch.cuda.empty_cache()

    iteration = {}
    for B in (64, 1024):
        torch.manual_seed(0)
        d = TeamChanceDeepCFR(game, batch=B, seed=SEED, memory_size=max(100000, ROWS * n * B))
        d._resolve(d._queue_iteration(10, loop_index=0))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        queued = [d._queue_iteration(10, loop_index=1 + j) for j in range(a.iter_reps)]
        e1.record(stream)
        for q in queued:
            d._resolve(q)
        stream.synchronize()
        iteration[str(B)] = e0.elapsed_time(e1) * 1e3 / a.iter_reps
        del d
        torch.cuda.empty_cache()

    S = 100
    store = [torch.stack([net()[i] for _ in range(S)]).contiguous() for i in range(6)]
    slots = torch.arange(S, dtype=torch.int32, device="cuda:0")
    coef = torch.full((S,), 1.0 / S, dtype=torch.float32, device="cuda:0")
    table = torch.zeros((game.G, 4), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    avg = lambda: [game.sdcfr_average_policy(t, S, [x.data_ptr() for x in store], S, slots.data_ptr(), coef.data_ptr(), table.data_ptr()) for t in (0, 1)]
    avg()
    stream.synchronize()
    average_us = timed(avg, 2)
    host_table = table.cpu().numpy()
    game.exploitability(host_table)
    t0 = time.perf_counter()
    game.exploitability(host_table)
    expl_us = (time.perf_counter() - t0) * 1e6

    game.tables_reset()
    game.cfr_iterate(2)
    cfr_us = timed(lambda: game.cfr_iterate(1), a.reps)
    mccfr = {}
    for B in (64, 1024):
        game.tables_reset()
        game.mccfr_iterate(B, 2)
        mccfr[str(B)] = timed(lambda: game.mccfr_iterate(B, 1), a.reps)

    rec = dict(n=n, G=game.G, traverse=traverse, iteration_us=iteration, average_policy_us=average_us, average_policy_snapshots=S, exploitability_us=expl_us,
               cfr_iteration_us=cfr_us, mccfr_iteration_us=mccfr)
    if n == 6:
        curve = {}
        game.tables_reset()
        t_run, it = 0.0, 0
        while t_run < a.wall:
            t0 = time.perf_counter()
            game.cfr_iterate(schedule("dcfr", it, 10))
            ctx.synchronize()
            t_run += time.perf_counter() - t0
            it += 10
        curve["dcfr"] = dict(iterations=it, seconds=t_run, exploitability=float(game.exploitability()[0]))
        torch.manual_seed(0)
        d = TeamChanceDeepCFR(game, batch=64, seed=SEED)
        t_run, it = 0.0, 0
        while t_run < a.wall:
            t0 = time.perf_counter()
            d._resolve(d._queue_iteration(10, loop_index=it))
            t_run += time.perf_counter() - t0
            it += 1
        curve["deep_cfr"] = dict(iterations=it, seconds=t_run, batch=64, exploitability=d.exploitability()["exploitability"])
        curve["uniform"] = float(game.exploitability(d.uniform_table())[0])
        rec["after_wall_time"] = curve
    game.close()
    ctx.close()
    rec["device"] = torch.cuda.get_device_name(0)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=None, choices=(6, 24))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--iter-reps", type=int, default=3)
    ap.add_argument("--wall", type=float, default=20.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.n is not None:
        line = json.dumps(one_size(a.n, a))
    else:
        sizes = {}
        for n in (6, 24):   # a fresh process per size
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--n", str(n), "--reps", str(a.reps), "--iter-reps", str(a.iter_reps), "--wall", str(a.wall)],
                                 check=True, capture_output=True, text=True).stdout
            sizes[str(n)] = json.loads(out.strip().splitlines()[-1])
        line = json.dumps(dict(bench="team_chance_sdcfr", packets=PACKETS, seed=SEED, reps=a.reps, iter_reps=a.iter_reps, wall_seconds=a.wall,
                               rows_per_traversal=ROWS, row_bytes=200, sizes=sizes))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
