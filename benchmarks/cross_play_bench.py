#!/usr/bin/env python3
"""The exact cross-play matrix and the K-policy best-response launch (scopa_cross_play, scopa_best_response) on the seed-42 deal, against the
only route to the same diagonal without them: K synchronous scopa_exploitability calls with an explicit policy.  Prints one JSON line.

    python benchmarks/cross_play_bench.py [--sizes 16,64] [--reps 30]

`*_ms` of the new calls are HIP events on the context's stream around one call (median of --reps after warm-up: the launches alone, no host
synchronisation inside); `exploitability_calls_ms` is the host clock around the K calls (each copies its policy in, launches, copies four
numbers out and synchronises).  The K tables are seeded Dirichlet rows; every number the two routes share is checked to agree bit for bit."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def event_ms(stream, fn, reps):
    import torch
    for _ in range(3):
        fn()
    stream.synchronize()
    pairs = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        pairs.append((e0, e1))
    stream.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in pairs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,64")
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    import torch
    from scopa_amd import _lib
    stream = torch.cuda.Stream()
    ctx = _lib.Context(0, stream=stream.cuda_stream)
    I = ctx.set_deal(_lib.deal_py_seed(42))
    nlegal = ctx.tree_export()["infoset_nlegal"].astype(np.int64)
    legal = np.arange(4)[None, :] < nlegal[:, None]
    rng = np.random.default_rng(42)
    out = {"bench": "cross_play", "device": torch.cuda.get_device_name(0), "n_infosets": I, "reps": args.reps, "by_K": {}}
    for K in (int(x) for x in args.sizes.split(",")):
        g = np.where(legal[None], rng.gamma(0.7, size=(K, I, 4)), 0.0)
        pols = g / g.sum(2, keepdims=True)
        d_pol = torch.as_tensor(pols, device="cuda:0")
        d_mat = torch.empty((K, K, 4), dtype=torch.float64, device="cuda:0")
        d_br = torch.empty((K, 2, I, 4), dtype=torch.float64, device="cuda:0")
        d_out4 = torch.empty((K, 4), dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        r = {"pairs": K * K,
             "cross_play_ms": round(event_ms(stream, lambda: ctx.cross_play(K, d_pol.data_ptr(), d_mat.data_ptr()), args.reps), 4),
             "best_response_ms": round(event_ms(stream, lambda: ctx.best_response(K, d_pol.data_ptr(), d_br.data_ptr(), d_out4.data_ptr()), args.reps), 4),
             "best_response_no_tables_ms": round(event_ms(stream, lambda: ctx.best_response(K, d_pol.data_ptr(), 0, d_out4.data_ptr()), args.reps), 4)}
        ctx.exploitability(policy=pols[0])
        ts = []
        for _ in range(max(args.reps // 10, 3)):
            t0 = time.perf_counter()
            each = [ctx.exploitability(policy=p) for p in pols]
            ts.append(1e3 * (time.perf_counter() - t0))
        r["exploitability_calls_ms"] = round(statistics.median(ts), 4)
        r["exploitability_call_ms"] = round(r["exploitability_calls_ms"] / K, 4)
        stream.synchronize()
        want = np.array([[e["exploitability"], e["br0"], e["br1"], e["value_p0"]] for e in each])
        r["same_bits"] = bool(np.array_equal(d_out4.cpu().numpy().view(np.uint64), want.view(np.uint64))
                              and np.array_equal(torch.diagonal(d_mat[..., 0]).cpu().numpy().view(np.uint64), want[:, 3].copy().view(np.uint64)))
        out["by_K"][K] = r
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
