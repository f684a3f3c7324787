#!/usr/bin/env python3
"""External-sampling MCCFR on FullScopa over the device infoset store (scopa_full_mccfr_*).  Prints one JSON line and writes it to --out
(rewritten after every stage, so a run that is cut short leaves what it measured).

    python benchmarks/full_mccfr_bench.py [--seed 42] [--batches 64,1024,16384] [--capacity-log2 26] [--curve 0,10,100] [--curve-batch 1024]
                                          [--episodes 1048576] [--out profiles/full_mccfr_bench.json]

Every figure is from ONE run of this script, one process, timed with HIP events on the context's stream.
iteration   per batch B, on a fresh store, from the deal's root: `traverse_ms` = the two traversal launches of one iteration (traverser 0, then 1),
            `apply_ms` = its two apply launches, each between events; `choice_visits_per_s` = B x (121 303 + 74 648) / traverse time.  A traverse
            call ends in the host's read of the dropped counter, so the window holds that round trip too.  `rows`, `dropped` and
            `store_bytes_used` = rows x 128 after the timed iterations.  A store that fills is recorded, not hidden: `store_full` and the
            dropped count (a dropped insert costs a full probe of 64 slots, so a full store also times differently).
model       `atomics_per_traversal` / `float64_atomics_per_traversal` / `bytes_read_per_traversal_lower_bound`, stated from the code: a traverser node
            with n cards makes n float64 adds and one uint32 add, an opponent node the same; every choice visit reads one 8-byte key word per probed
            slot (at least one) and the 24-byte regret row.
match       `match_episodes_per_s`: scopa_full_mccfr_match on --episodes episodes from the deal's root.
curve       `curve`: evaluate_vs_random on --episodes episodes after each count of --curve iterations at --curve-batch: mean reward of the average
            policy against uniform play, its standard error, rows and dropped at that point.  Should the store fill, the curve ends there and
            the record says where.
host        `restatement_round2_pair_s`: tests/full_mccfr_ref.py, one traversal per traverser from a round-2 root, one host core (5 439 choice visits)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S_ROOT = (6 ** 6 - 1) // 5
VISITS = (13 * S_ROOT, 8 * S_ROOT)
# per round entry: traverser 0 meets 1 own 3-card node, 3 opponent 3-card, 3 own 2-card, 6 opponent 2-card; traverser 1: 1 opp 3, 1 own 3, 3 opp 2, 3 own 2
F64_ATOMICS = ((1 * 3 + 3 * 3 + 3 * 2 + 6 * 2) * S_ROOT, (1 * 3 + 1 * 3 + 3 * 2 + 3 * 2) * S_ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--batches", default="64,1024,16384")
    ap.add_argument("--capacity-log2", type=int, default=26)
    ap.add_argument("--curve", default="0,10,100")
    ap.add_argument("--curve-batch", type=int, default=1024)
    ap.add_argument("--episodes", type=int, default=1 << 20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from scopa_amd import _lib
    stream = torch.cuda.Stream()
    ctx = _lib.Context(0, stream=stream.cuda_stream)
    ctx.mccfr_seed(0x5C09A)
    deck = _lib.full_deal_py_seed(a.seed)
    rec = dict(bench="full_mccfr", runs=1, seed=a.seed, device=torch.cuda.get_device_name(0), capacity_log2=a.capacity_log2,
               store_bytes=128 << a.capacity_log2, choice_visits_per_traversal=list(VISITS), terminals_per_traversal=6 ** 6,
               atomics_per_traversal=[f + v for f, v in zip(F64_ATOMICS, VISITS)], float64_atomics_per_traversal=list(F64_ATOMICS),
               bytes_read_per_traversal_lower_bound=[32 * v for v in VISITS], iteration={}, curve=[])

    def flush():
        line = json.dumps(rec)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return line

    def timed(fn):
        """-> (ms, the ScopaError the call raised or None)"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        err = None
        e0.record(stream)
        try:
            fn()
        except _lib.ScopaError as e:
            if e.status != _lib.SCOPA_ENOMEM:
                raise
            err = e
        e1.record(stream)
        stream.synchronize()
        return e0.elapsed_time(e1), err

    for B in (int(x) for x in a.batches.split(",")):
        h = _lib.FullMCCFR(ctx, deck, None, a.capacity_log2)
        n = 3 if B <= 1024 else 1
        h.iterate(min(B, 64), 1)                       # warm-up: code objects, first touches
        h.reset()
        trav = app = 0.0
        full = False
        it0 = h.counters()["iterations"]
        for k in range(n):
            for t in range(2):
                ms, err = timed(lambda: h.traverse(t, it0 + 2 * k + t, 0, B))
                trav += ms
                full = full or err is not None
                app += timed(h.apply)[0]
        c = h.counters()
        rec["iteration"][str(B)] = dict(iterations_timed=n, traverse_ms=trav / n, apply_ms=app / n, iteration_ms=(trav + app) / n,
                                        choice_visits_per_s=B * sum(VISITS) * n / trav * 1e3, rows=c["rows"], dropped=c["dropped"],
                                        store_bytes_used=128 * c["rows"], store_full=full)
        h.close()
        flush()

    h = _lib.FullMCCFR(ctx, deck, None, a.capacity_log2)
    h.match(1 << 12)
    ms, _ = timed(lambda: h.match(a.episodes))
    rec["match_episodes"], rec["match_episodes_per_s"] = a.episodes, a.episodes / ms * 1e3
    flush()

    def evaluate(done, full):
        s = h.match(a.episodes)
        n = float(a.episodes)
        mean = float(s[0] + s[1]) / 2.0 / n
        var = max(float(s[2] + s[3]) / 4.0 / n - mean * mean, 0.0)
        c = h.counters()
        rec["curve"].append(dict(iterations=done, batch=a.curve_batch, mean_reward=mean, standard_error=float(np.sqrt(var / n)), agent_scopas=float(s[4]) / n,
                                 opponent_scopas=float(s[5]) / n, rows=c["rows"], dropped=c["dropped"], store_full=full))
        flush()

    done = 0
    for target in (int(x) for x in a.curve.split(",")):
        full = False
        while done < target and not full:
            try:
                h.iterate(a.curve_batch, 1)
            except _lib.ScopaError as e:
                if e.status != _lib.SCOPA_ENOMEM:
                    raise
                full = True
            done += 1
        evaluate(done, full)
        if full:
            break
    h.close()

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle as O
    O.build()
    import full_mccfr_ref as F
    root, _ = F.random_root(deck, 2, np.random.RandomState(0))
    rows = F.Rows()
    t0 = time.perf_counter()
    for t in range(2):
        F.walk(root, t, 0, 0, 0x5C09A, rows)
    rec["restatement_round2_pair_s"] = time.perf_counter() - t0
    rec["restatement_round2_pair_choice_visits"] = rows.choice
    print(flush())
    ctx.close()


if __name__ == "__main__":
    main()
