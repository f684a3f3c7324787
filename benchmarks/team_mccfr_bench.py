#!/usr/bin/env python3
"""External-sampling MCCFR on Team MiniScopa on the device (scopa_team_mccfr_*) against the host routes.  Prints one JSON line (and writes it to --out).

    python benchmarks/team_mccfr_bench.py [--seed 42] [--batches 64,1024,4096] [--iters 200] [--warmup 20] [--replay-iters 20] [--host-iters 3]
                                          [--reference-traversal-s T0,T1] [--out profiles/team_mccfr_bench.json]

Every figure is from ONE run of this script and is labelled so in the record.
batched     per batch B: `iteration_us`: HIP events on the context's stream around one scopa_team_mccfr_iterate(B, n) call after --warmup iterations
            (two launches per iteration, no host synchronisation inside), divided by n; n = --iters for B <= 64 and is scaled down to keep the window
            near the same number of traversals (at least 20).  `walk_us` / `apply_us`: the same around each of n scopa_team_mccfr_traverse and the
            scopa_team_mccfr_apply that follows it (an apply on an empty delta buffer would skip every row).  `visits_per_s`: 69 964 decision visits per
            pair of traversals (the reference's count, forced plies included) x B / iteration time; `sampled_visits_per_s` counts only the 12 364 visits
            that draw (depths 0..11).
atomics     `atomic_bytes_per_pair`, a byte model stated from the code (scopa_team_mccfr.hip): per pair of traversals 2 x 3 600 uint64 arrival counts and,
            for the 2 x 1 731 traverser instances less those of depths 0..4 (31 + 6 per pair, kept in LDS), up to b + 1 float64 adds each -- 8 bytes per
            atomic; increments that are exactly 0.0 are not sent, so this is an upper bound.
replay      `replay_iteration_ms`: HIP events around scopa_team_mccfr_replay calls of --replay-iters iterations, upload of the uniforms included.
host        `numpy_batched_iteration_ms` (batch 64) and `numpy_replay_iteration_ms`: the float64 restatement tests/team_mccfr_ref.py on one core.
reference   `reference_python_traversal_s`: ONLY with --reference-traversal-s: the wall time of the reference's own MCCFRTrainer._sample from the root for
            traverser 0 and 1, as tests/tools/gen_team_mccfr_golden.py printed it on the machine that wrote the fixture (another machine's CPU: recorded as
            given, a measurement of one full traversal each, not an extrapolation).
The device tables are not compared here: tests/test_gpu_team_mccfr.py holds the kernels to the restatement."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DRAWS, SAMPLED = 69964, 9781 + 2583
STAGE = ((1, 4), (5, 4), (25, 3), (100, 3), (400, 2), (1200, 2))     # the traverser's plies: instances, cards


def atomic_bytes_per_pair():
    deep = [sum(n * (b + 1) for k, (n, b) in enumerate(STAGE) if k not in lds) for lds in ((0, 1, 2), (0, 1))]   # traverser 0: depths 0, 1, 4 in LDS; 1: depths 2, 3
    return 8 * (2 * 3600 + sum(deep))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--batches", default="64,1024,4096")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--replay-iters", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--reference-traversal-s", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.iters >= 200, "at least 200 iterations after warm-up at the smallest batch"
    import torch
    from scopa_amd import _lib
    stream = torch.cuda.Stream()
    ctx = _lib.Context(0, stream=stream.cuda_stream)
    perm = _lib.deal_py_seed(a.seed)
    ctx.team_set_deal(perm)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        stream.synchronize()
        return e0.elapsed_time(e1) * 1e3        # us

    batched = {}
    for B in (int(x) for x in a.batches.split(",")):
        n = max(20, a.iters * 64 // max(B, 64))
        ctx.team_tables_reset()
        ctx.team_mccfr_iterate(B, min(a.warmup, n))
        it_us = timed(lambda: ctx.team_mccfr_iterate(B, n)) / n
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3 * n)]
        it0 = ctx.team_mccfr_counters()[2]
        for k in range(n):
            ev[3 * k].record(stream)
            ctx.team_mccfr_traverse(it0 + k, 0, B)
            ev[3 * k + 1].record(stream)
            ctx.team_mccfr_apply()
            ev[3 * k + 2].record(stream)
        stream.synchronize()
        walk = sum(ev[3 * k].elapsed_time(ev[3 * k + 1]) for k in range(n)) * 1e3 / n
        apply = sum(ev[3 * k + 1].elapsed_time(ev[3 * k + 2]) for k in range(n)) * 1e3 / n
        batched[str(B)] = dict(iterations_timed=n, iteration_us=it_us, walk_us=walk, apply_us=apply, visits_per_s=DRAWS * B / it_us * 1e6,
                               sampled_visits_per_s=SAMPLED * B / it_us * 1e6, atomic_GBps=atomic_bytes_per_pair() * B / walk * 1e-3)
    expl = float(ctx.team_exploitability()[0])

    ctx.team_tables_reset()
    u = np.random.RandomState(1).random_sample(DRAWS * a.replay_iters)
    ctx.team_mccfr_replay(2, u)
    replay_ms = timed(lambda: ctx.team_mccfr_replay(a.replay_iters, u)) / a.replay_iters * 1e-3
    rec = dict(bench="team_mccfr", runs=1, seed=a.seed, warmup=a.warmup, device=torch.cuda.get_device_name(0), batched=batched, launches_per_iteration=2,
               atomic_bytes_per_pair_upper_bound=atomic_bytes_per_pair(), replay_iterations_timed=a.replay_iters, replay_iteration_ms=replay_ms,
               replay_visits_per_s=DRAWS / replay_ms * 1e3, exploitability_after_batched_runs=expl)

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle as O
    O.build()
    import team_mccfr_ref as M
    mc = M.MCRef(perm)
    st = mc.state()
    mc.iterate(st, 64, 0x5C09A, 0)
    t0 = time.perf_counter()
    for it in range(a.host_iters):
        mc.iterate(st, 64, 0x5C09A, 1 + it)
    rec["numpy_batched_iteration_ms_batch64"] = 1e3 * (time.perf_counter() - t0) / a.host_iters
    st = mc.state()
    t0 = time.perf_counter()
    upos = 0
    for it in range(a.host_iters):
        upos = mc.iteration(st, u, upos)
    rec["numpy_replay_iteration_ms"] = 1e3 * (time.perf_counter() - t0) / a.host_iters
    rec["speedup_vs_numpy_batch64"] = rec["numpy_batched_iteration_ms_batch64"] * 1e3 / batched["64"]["iteration_us"] if "64" in batched else None
    rec["replay_speedup_vs_numpy"] = rec["numpy_replay_iteration_ms"] / replay_ms
    if a.reference_traversal_s:
        t = [float(x) for x in a.reference_traversal_s.split(",")]
        rec["reference_python_traversal_s"] = t
        rec["reference_python_iteration_s"] = sum(t)
        rec["reference_python_note"] = ("MCCFRTrainer._sample from the root, one call per traverser, timed by tests/tools/gen_team_mccfr_golden.py on the CPU of the machine that "
                                        "wrote the fixture: measured whole traversals, another machine than the device's host")
        rec["replay_speedup_vs_reference_python"] = sum(t) * 1e3 / replay_ms
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
