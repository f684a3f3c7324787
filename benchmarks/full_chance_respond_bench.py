#!/usr/bin/env python3
"""The sampled best response of FullScopa over a set of decks (scopa_full_chance_respond_iterate, _harden) beside the MCCFR iteration it is cut from
(scopa_full_chance_iterate), and the figure it exists for: a lower bound on a store's exploitability, set beside the exact one where there is one and
taken from the deal's root where there is none.  Prints one JSON line and writes it to --out (rewritten after every stage).

    python benchmarks/full_chance_respond_bench.py [--seed 42] [--decks 8,64] [--batch 64] [--runs 5] [--train 100] [--respond 10,100,1000]
                                                   [--episodes 65536] [--out profiles/full_chance_respond_bench.json]

Every figure is from ONE run of this script, one process, timed with HIP events on the context's stream.  No threshold is set anywhere.
iteration   per root ("round3": after 18 plies of uniformly random play on the deck of --seed, decks = packet_decks(deck, 3, n, --seed); "deal":
            packet_decks(deck, 0, n, --seed)) and deck count n: `iterate_ms` = one scopa_full_chance_iterate call of one iteration at --batch on a
            store that already holds the decks' rows; `respond_ms` = one scopa_full_chance_respond_iterate call of one iteration at the same batch
            of a second store against the first (average policy), that store warm too.  --runs runs of each, interleaved; `*_runs_ms` lists them,
            `*_ms` is their median, `ratio` = respond_ms / iterate_ms.  Both walk the same number of nodes.
bound       per root, on 8 decks: a store trained --train MCCFR iterations at --batch, then ONE responder trained on against it and hardened after
            each count of --respond iterations; per count the seat-swapped match of the hardened responder against the store (--episodes episodes:
            `reward` +- `std_error`, and by seat) and, at the round-3 root, the responder's exact value from cross_play (`exact_reward`, by seat) beside
            the store's exact br0, br1 and (br0 + br1) / 2 from the sweeps' own pure response.  From the deal the exact fields are null: nothing exact
            exists there, and the sampled figure is the bound."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--decks", default="8,64")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--train", type=int, default=100)
    ap.add_argument("--respond", default="10,100,1000")
    ap.add_argument("--episodes", type=int, default=1 << 16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from scopa_amd import _lib
    from scopa_amd.algorithms import FullChanceMCCFRTrainer, packet_decks
    from scopa_amd.algorithms.full_chance import response_report
    stream = torch.cuda.Stream()
    ctx = _lib.Context(0, stream=stream.cuda_stream)
    ctx.mccfr_seed(0x5C09A)
    deck = _lib.full_deal_py_seed(a.seed)
    rng = np.random.RandomState(0)
    late, prefix = _lib.FullState(deck=deck), []
    for _ in range(18):
        legal = late.legal()
        prefix.append(int(legal[rng.randint(len(legal))]))
        late.step(prefix[-1])
    roots = (("round3", 3, tuple(prefix)), ("deal", 0, ()))
    rec = dict(bench="full_chance_respond", seed=a.seed, device=torch.cuda.get_device_name(0), batch=a.batch, runs=a.runs, iteration=[], bound=[])

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

    def cap_for(rounds, n):
        return max(12, int(np.ceil(np.log2(4.0 * n * 143304)))) if rounds == 0 else 20           # a store at most a quarter full

    for name, rounds, acts in roots:
        for n in (int(x) for x in a.decks.split(",")):
            decks = packet_decks(deck, rounds, n, a.seed)
            t = FullChanceMCCFRTrainer(decks=decks, root_actions=acts, capacity_log2=cap_for(rounds, n), batch=a.batch, ctx=ctx)
            r = FullChanceMCCFRTrainer(decks=decks, root_actions=acts, capacity_log2=cap_for(rounds, n), batch=a.batch, ctx=ctx)
            t.solver.iterate(a.batch, 2)                                   # warm-up: code objects, first touches, most rows claimed
            r.solver.respond_iterate(t.solver, 0, a.batch, 2)
            it, rs = [], []
            for _ in range(a.runs):
                it.append(timed(lambda: t.solver.iterate(a.batch, 1)))
                rs.append(timed(lambda: r.solver.respond_iterate(t.solver, 0, a.batch, 1)))
            rec["iteration"].append(dict(root=name, decks=n, capacity_log2=cap_for(rounds, n), iterate_runs_ms=it, respond_runs_ms=rs,
                                         iterate_ms=float(np.median(it)), respond_ms=float(np.median(rs)), ratio=float(np.median(rs) / np.median(it)),
                                         rows=t.counters()["rows"], respond_rows=r.counters()["rows"], dropped=t.counters()["dropped"] + r.counters()["dropped"]))
            t.close()
            r.close()
            flush()

    for name, rounds, acts in roots:
        decks = packet_decks(deck, rounds, 8, a.seed)
        t = FullChanceMCCFRTrainer(decks=decks, root_actions=acts, capacity_log2=cap_for(rounds, 8), batch=a.batch, ctx=ctx)
        t.train(a.train)
        r, done, exact = None, 0, None
        for target in (int(x) for x in a.respond.split(",")):
            if r is None:
                r = t.sampled_response(target)
            else:
                r.solver.respond_iterate(t.solver, 0, a.batch, target - done)
                r.solver.harden()
            done = target
            rep = response_report(r, t, a.episodes)
            if exact is None and rep["exact_reward"] is not None:          # the sub-game fits the sweeps: the store's own exact figures, once
                exact = t.exploitability()
            rec["bound"].append(dict(root=name, decks=8, trained_iterations=a.train, response_iterations=done, batch=a.batch, episodes=a.episodes,
                                     reward=rep["reward"], std_error=rep["std_error"], reward_by_seat=[s["reward"] for s in rep["by_seat"]],
                                     exact_reward=rep["exact_reward"], exact_by_seat=rep["exact_by_seat"], store_exact=exact,
                                     response_rows=r.counters()["rows"], store_rows=t.counters()["rows"], dropped=r.counters()["dropped"]))
            flush()
        r.close()
        t.close()
    print(flush())
    ctx.close()


if __name__ == "__main__":
    main()
