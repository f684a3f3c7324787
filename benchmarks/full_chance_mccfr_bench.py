#!/usr/bin/env python3
"""External-sampling MCCFR on FullScopa over a SET of decks (scopa_full_chance_*), against the one-deck solver (scopa_full_mccfr_*).  Prints one JSON
line and writes it to --out (rewritten after every stage, so a run that is cut short leaves what it measured).

    python benchmarks/full_chance_mccfr_bench.py [--seed 42] [--decks 8,64] [--batch 64] [--runs 3] [--curve 0,10,100] [--held-out 64]
                                                 [--episodes 262144] [--out profiles/full_chance_mccfr_bench.json]

Every figure is from ONE run of this script, one process, timed with HIP events on the context's stream.
iteration   per deck count n, decks = packet_decks(deck of --seed, 0, n, --seed): `chance_ms` = one scopa_full_chance_iterate call of one iteration over
            all n decks at --batch (two traversal launches of n x batch walks, two applies, the closing read of the dropped counter) on a store
            that already holds the decks' rows; `one_deck_ms` = n scopa_full_mccfr_iterate calls of one iteration at the same batch, one handle per
            deck, each on a store that already holds its deck's rows.  --runs runs of each, interleaved; `*_runs_ms` lists them, `*_ms` is their
            median, `ratio` = chance_ms / one_deck_ms, `ratio_spread` = (min, max) of the per-run ratios.  Both walks make the same number of choice
            visits (n x batch x 195 951), so the ratio is also the ratio of the cost per choice visit.  `rows` and `dropped` after the timed runs.
curve       the generalisation curve: for each n, after each count of --curve iterations at --batch, the mean reward of the average policy against
            uniform play (scopa_full_chance_match, --episodes episodes) on the n training decks and on --held-out decks of the same packet that the
            solver never walked.  `packet` names the packet: "deal" = decks that share the four table cards only (the stock and both hands differ, so
            two decks share next to no infoset and nothing learned carries over); "round4" = decks that share the first four rounds, below a root
            after four rounds of uniformly random play: the 12 cards left are dealt differently, and rows are shared wherever a hand, table and
            counts recur.
update      --update FILE measures nothing: it reads the record in FILE, adds the blocks below from figures measured elsewhere, and writes it back.
            --one-deck-parent / --one-deck-this: comma lists of records of benchmarks/full_mccfr_bench.py (--batches 64,1024 --capacity-log2 22
            --curve 0) run at the parent commit and at this one, alternated on one GPU -> `one_deck_walk_parent_vs_this`: the cost of moving the
            walk into scopa_full_mccfr_walk.h for the one-deck solver.  --regret-error-over-budget X: the largest "largest regret error / budget"
            that tests/test_gpu_full_chance.py printed (pytest -s) -> `largest_regret_error_over_budget`."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S_ROOT = (6 ** 6 - 1) // 5
VISITS = 21 * S_ROOT                   # choice visits of one traversal per traverser from the deal


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--decks", default="8,64")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--curve", default="0,10,100")
    ap.add_argument("--held-out", type=int, default=64)
    ap.add_argument("--episodes", type=int, default=1 << 18)
    ap.add_argument("--out", default=None)
    ap.add_argument("--update", default=None)
    ap.add_argument("--one-deck-parent", default="")
    ap.add_argument("--one-deck-this", default="")
    ap.add_argument("--regret-error-over-budget", type=float, default=None)
    a = ap.parse_args()
    if a.update:
        with open(a.update) as f:
            rec = json.load(f)
        runs = {}
        for side, files in (("parent", a.one_deck_parent), ("this", a.one_deck_this)):
            for k, name in enumerate(x for x in files.split(",") if x):
                with open(name) as f:
                    r = json.load(f)
                runs[f"{side}_{k + 1}"] = {b: dict(traverse_ms=v["traverse_ms"], apply_ms=v["apply_ms"], rows=v["rows"], dropped=v["dropped"]) for b, v in r["iteration"].items()}
        if runs:
            rec["one_deck_walk_parent_vs_this"] = dict(note="benchmarks/full_mccfr_bench.py --batches 64,1024 --capacity-log2 22 --curve 0 at the parent commit and at this "
                                                       "one, alternated on one GPU: traverse_ms = the two traversal launches of an iteration", runs=runs)
        if a.regret_error_over_budget is not None:
            rec["largest_regret_error_over_budget"] = a.regret_error_over_budget
        with open(a.update, "w") as f:
            f.write(json.dumps(rec) + "\n")
        print(json.dumps(rec))
        return
    import torch
    from scopa_amd import _lib
    from scopa_amd.algorithms import packet_decks
    stream = torch.cuda.Stream()
    ctx = _lib.Context(0, stream=stream.cuda_stream)
    ctx.mccfr_seed(0x5C09A)
    deck = _lib.full_deal_py_seed(a.seed)
    rec = dict(bench="full_chance_mccfr", seed=a.seed, device=torch.cuda.get_device_name(0), batch=a.batch, runs=a.runs,
               choice_visits_per_traversal_pair=VISITS, iteration={}, curve=[])

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

    def cap_for(rows):
        return max(12, int(np.ceil(np.log2(4.0 * rows))))                 # a store at most a quarter full

    ns = [int(x) for x in a.decks.split(",")]
    for n in ns:
        decks = packet_decks(deck, 0, n, a.seed)
        cap = cap_for(n * 143304)
        h = _lib.FullChanceMCCFR(ctx, decks, None, cap)
        ones = [_lib.FullMCCFR(ctx, d, None, 20) for d in decks]
        h.iterate(a.batch, 2)                                              # warm-up: code objects, first touches, most rows claimed
        for o in ones:
            o.iterate(a.batch, 2)
        chance, one = [], []
        for _ in range(a.runs):
            chance.append(timed(lambda: h.iterate(a.batch, 1)))
            one.append(timed(lambda: [o.iterate(a.batch, 1) for o in ones]))
        c = h.counters()
        ratios = [x / y for x, y in zip(chance, one)]
        rec["iteration"][str(n)] = dict(capacity_log2=cap, store_bytes=128 << cap, chance_runs_ms=chance, one_deck_runs_ms=one, chance_ms=float(np.median(chance)),
                                        one_deck_ms=float(np.median(one)), ratio=float(np.median(chance) / np.median(one)), ratio_spread=[min(ratios), max(ratios)],
                                        choice_visits_per_s=n * a.batch * VISITS / np.median(chance) * 1e3, rows=c["rows"], dropped=c["dropped"],
                                        one_deck_rows=sum(o.counters()["rows"] for o in ones), one_deck_dropped=sum(o.counters()["dropped"] for o in ones))
        h.close()
        for o in ones:
            o.close()
        flush()

    def evaluate(h, held):
        out = {}
        for name, ds in (("train", None), ("held_out", held)):
            s = h.match(a.episodes, 0, ds)
            n = float(a.episodes)
            mean = float(s[0] + s[1]) / 2.0 / n
            var = max(float(s[2] + s[3]) / 4.0 / n - mean * mean, 0.0)
            out[name] = dict(mean_reward=mean, standard_error=float(np.sqrt(var / n)))
        return out

    rng = np.random.RandomState(0)
    late = _lib.FullState(deck=deck)
    for _ in range(24):
        legal = late.legal()
        late.step(legal[rng.randint(len(legal))])
    for packet, rounds, root in (("deal", 0, None), ("round4", 4, late.s)):
        for n in ns:
            every = packet_decks(deck, rounds, n + a.held_out, a.seed)
            decks, held = every[:n], every[n:]
            h = _lib.FullChanceMCCFR(ctx, decks, root, cap_for(n * 143304) if rounds == 0 else 18)
            done = 0
            for target in (int(x) for x in a.curve.split(",")):
                if target > done:
                    h.iterate(a.batch, target - done)
                    done = target
                c = h.counters()
                rec["curve"].append(dict(packet=packet, decks=n, held_out_decks=a.held_out, iterations=done, batch=a.batch, episodes=a.episodes, rows=c["rows"],
                                         dropped=c["dropped"], **evaluate(h, held)))
                flush()
            h.close()
    print(flush())
    ctx.close()


if __name__ == "__main__":
    main()
