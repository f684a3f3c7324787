#!/usr/bin/env python3
"""The exact weighted CFR iteration of FullScopa across a set of decks (scopa_full_chance_cfr_iterate) on sub-games of 2, 3 and 4 rounds, beside the
exploitability call on the same forest and beside the sampled solver.  Prints one JSON line and writes it to --out (rewritten after every stage, so
a run that is cut short leaves what it measured).

    python benchmarks/full_chance_cfr_bench.py [--seed 42] [--iterations 50] [--warmup 5] [--capacity-log2 24] [--curve-chunks 10] [--curve-cfr 10]
                                               [--curve-mccfr 50] [--batch 64] [--out profiles/full_chance_cfr_bench.json]

Every figure is from ONE run of this script, one process, timed with HIP events on the context's stream around whole synchronous calls.
decks       packet_decks(deck --seed, 4, 64, 1): decks that share their first four rounds, so every one of them fits the round-2 root of the random
            play (RandomState(0)) on deck 0 and its descendants one and two rounds further down (the exploitability bench's packet).
iterate_ms  per (R, decks) in (2, 8), (2, 64), (3, 8), (3, 64), (4, 2), on a handle of those decks at the root with R rounds to go, DCFR(1.5, 0, 2)
            weights, alternating (and, as `simultaneous`, one sweep an iteration): after a call of --warmup iterations, `call_ms` = a call of
            --iterations iterations and `one_ms` = a call of 1; per_iteration_ms = (call_ms - one_ms) / (iterations - 1), setup_ms = one_ms -
            per_iteration_ms (forest, keys, the two sorts a level, the claim and the write-back).  `exploitability_ms` = one exploitability call
            (which = 0) on the same handle, root and decks, after a first call that lays out its scratch: the yardstick.  `launches` = the kernel
            launches an iteration makes.
curve       on the round-3 root with 8 training decks, from empty stores: (BR0 + BR1) / 2 of the average policy against the wall time spent in the
            solver's calls, for DCFR(1.5, 0, 2) and CFR+ from cfr_iterate (--curve-chunks chunks of --curve-cfr alternating iterations) and for MCCFR
            at --batch (chunks of --curve-mccfr iterations).  With R = 3 the response has imperfect recall across rounds: the figure is a lower
            bound on the exploitability, and CFR has no convergence proof on these rows."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((2, 8), (2, 64), (3, 8), (3, 64), (4, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--iterations", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--capacity-log2", type=int, default=24)
    ap.add_argument("--curve-chunks", type=int, default=10)
    ap.add_argument("--curve-cfr", type=int, default=10)
    ap.add_argument("--curve-mccfr", type=int, default=50)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from scopa_amd import _lib
    from scopa_amd.algorithms import packet_decks, schedule
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import full_mccfr_ref as F
    stream = torch.cuda.Stream()
    ctx = _lib.Context(0, stream=stream.cuda_stream)
    ctx.mccfr_seed(0x5C09A)
    deck = _lib.full_deal_py_seed(a.seed)
    _, acts = F.random_root(deck, 4, np.random.RandomState(0))          # the round-2 root is its first two rounds, the descendants the next ones
    decks = packet_decks(deck, 4, 64, 1)

    def state_after(n_rounds):
        s = _lib.FullState(deck=deck)
        for x in acts[:6 * n_rounds]:
            s.step(x)
        return s.s

    rec = dict(bench="full_chance_cfr", runs=1, seed=a.seed, device=torch.cuda.get_device_name(0), iterations=a.iterations, warmup=a.warmup,
               capacity_log2=a.capacity_log2, iterate_ms={}, curve={})

    def flush():
        line = json.dumps(rec)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return line

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        out = fn()
        e1.record(stream)
        stream.synchronize()
        return e0.elapsed_time(e1), out

    dcfr = dict(alpha=1.5, beta=0.0, gamma=2.0)
    for R, n in SHAPES:
        h = _lib.FullChanceMCCFR(ctx, decks[:n], state_after(6 - R), a.capacity_log2)
        L = 4 * R
        entry = dict(leaves=n * 36 ** R, nodes=n * 31 * (36 ** R - 1) // 35)
        for name, alternating, launches in (("alternating", True, 5 * L), ("simultaneous", False, 3 * L + 1)):
            h.reset()
            t = a.warmup
            h.cfr_iterate(a.warmup, schedule("dcfr", 0, a.warmup, **dcfr), alternating)
            call_ms, _ = timed(lambda: h.cfr_iterate(a.iterations, schedule("dcfr", t, a.iterations, **dcfr), alternating))
            t += a.iterations
            one_ms, _ = timed(lambda: h.cfr_iterate(1, schedule("dcfr", t, 1, **dcfr), alternating))
            per = (call_ms - one_ms) / max(a.iterations - 1, 1)
            entry[name] = dict(call_ms=call_ms, one_ms=one_ms, per_iteration_ms=per, setup_ms=one_ms - per, launches=launches)
        entry["rows"] = h.counters()["rows"]
        h.exploitability(None, 0)
        entry["exploitability_ms"], entry["result"] = timed(lambda: h.exploitability(None, 0))
        rec["iterate_ms"][f"R{R}_decks{n}"] = entry
        flush()
        h.close()

    train, root3 = decks[:8], state_after(3)

    def curve(name, step):
        h = _lib.FullChanceMCCFR(ctx, train, root3, a.capacity_log2)
        pts, wall = [dict(iterations=0, wall_s=0.0, **h.exploitability(None, 0))], 0.0
        for c in range(a.curve_chunks):
            t0 = time.perf_counter()
            done = step(h, c)
            wall += time.perf_counter() - t0
            pts.append(dict(iterations=done, wall_s=wall, **h.exploitability(None, 0)))
            rec["curve"][name] = pts
            flush()
        h.close()

    k = a.curve_cfr
    for variant, params in (("dcfr", dcfr), ("cfr+", {})):
        def step(h, c, variant=variant, params=params):
            h.cfr_iterate(k, schedule(variant, c * k, k, **params), True)
            return (c + 1) * k
        curve(variant, step)

    def step_mccfr(h, c):
        h.iterate(a.batch, a.curve_mccfr)
        return (c + 1) * a.curve_mccfr
    curve(f"mccfr_batch{a.batch}", step_mccfr)
    print(flush())
    ctx.close()


if __name__ == "__main__":
    main()
