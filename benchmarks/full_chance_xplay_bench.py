#!/usr/bin/env python3
"""FullScopa over decks, store against store: the exact cross-play matrix (scopa_full_chance_cross_play) and the sampled match of two stores
(scopa_full_chance_pair_match).  Prints one JSON line and writes it to --out (rewritten after every stage, so a run that is cut short leaves what it
measured).

    python benchmarks/full_chance_xplay_bench.py [--seed 42] [--batch 64] [--iterations 20] [--capacity-log2 22] [--calls 10] [--warmup 2]
                                                 [--episodes-log2 22] [--use-iterations 100] [--out profiles/full_chance_xplay_bench.json]

Every figure is from ONE run of this script, one process, timed with HIP events on the context's stream.  No threshold is set on any timing: the
baselines are the host loop that cross-play replaces and the parent's `match` and `exploitability`, measured in the same run.
decks       packet_decks(deck --seed, 4, 72, 1): decks of one packet that share their first four rounds, so every one fits the round-2 root of the
            random play (RandomState(0)) on deck 0 and its descendants one and two rounds further down.
stores      16 stores of 2^--capacity-log2 slots, store j trained --iterations iterations at --batch on the first 64 decks from the round-2 root
            under Philox seed 0x5C09A + j (as benchmarks/full_chance_exploit_bench.py trains its one store).
cross_play  per (R, decks, K) -- R = 2 on 8 and 64 decks and R = 3 on 8 decks with K = 1 / 4 / 16, R = 3 on 64 decks and R = 4 on 2 decks with
            K = 1 / 4 (K = 16 there exceeds K x decks x 36^R <= 1 << 24): `first_ms` (the call that allocates or re-uses the scratch), then --warmup
            calls, then HIP events around --calls calls: `call_ms` is their mean.
            `host_loop`: what the call replaces, the route that existed: per ordered pair (a, b) the rows of store a's player 0 and of store b's
            player 1 (taken with tables_get once per store, outside the timing) merged, written to a third handle with tables_set, and one
            exploitability call on it, which gives the reward alone.  All K^2 pairs where K <= 4; at K = 16 the first 8 pairs, `total_ms`
            extrapolated to 256 (`extrapolated`).  `equal_bits`: its values equal the matrix's [a][b][0] on bits.
            `exploitability_ms`: one exploitability call of store 0 on the same forest, mean of --calls after --warmup.
            `bytes`: the byte model of the call -- what must cross the memory bus if the caches keep nothing between launches and everything
            within one: per level the states written once (64 B a node; 4 B a leaf) and read by the policy and the expand launch, the K prob
            images written and read once (24 B a node and store), V read and written once per row ([K^2][4] doubles a node; [K][4] at the lowest
            level, whose row b is read by each of the K pairs (a, b) above it), the leaves read once per store.  The stores' own lines are not
            in it (`probe_bytes_upper`: one 128-byte line per node and store, the bound if no two nodes shared a pair).  `frac_of_hbm_peak` is
            bytes / call_ms against 8 TB/s; the call also holds 3 L + 2 launches and one host synchronisation, so it is a figure for the whole
            call, not for its widest kernel.
pair_match  2^--episodes-log2 episodes from the DEAL's root of a store trained 2 iterations at --batch on 8 decks that share three rounds, against a
            second such store, and `match` (uniform opponent) on the same handle: mean of 3 calls after 1.
worked_use  store A: --use-iterations MCCFR iterations at --batch from the deal on 8 decks that share three rounds; store B: the same training, then
            solve_cfr(--use-iterations) on the round-3 root (random play, RandomState(0), on deck 0).  Their cross-play on that root on the training
            decks and on 8 held-out decks of the packet, and B's match against A from the deal's root (2^18 episodes) on both."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((2, 8, (1, 4, 16)), (2, 64, (1, 4, 16)), (3, 8, (1, 4, 16)), (3, 64, (1, 4)), (4, 2, (1, 4)))
HBM_PEAK = 8.0e12


def level_sizes(R, n):
    """nodes of the 4 R choice levels of n trees, then the leaves"""
    out, base = [], n
    for k in range(4 * R):
        if k and k % 4 == 0:
            base *= 36
        out.append(base * (1, 3, 9, 18)[k % 4])
    return out, base * 36


def byte_model(R, n, K):
    sizes, leaves = level_sizes(R, n)
    T, L = sum(sizes), len(sizes)
    states = 64 * T + 2 * 64 * T + 4 * leaves                                   # written once, read by policy and by expand; the packed leaves
    prob = 2 * 24 * K * T
    v = K * 4 * leaves + 32 * K * sizes[L - 1]                                  # the lowest level: leaves in per store, [K][4] out
    for k in range(L - 1):
        rows_in = K * K                                                         # (row b of the lowest level is read once per pair above it)
        v += 32 * rows_in * sizes[k + 1] + 32 * K * K * sizes[k]
    return dict(states=states, prob=prob, values=v, total=states + prob + v, probe_bytes_upper=128 * K * T, nodes=T, leaves=leaves)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--capacity-log2", type=int, default=22)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--episodes-log2", type=int, default=22)
    ap.add_argument("--use-iterations", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from scopa_amd import _lib
    from scopa_amd.algorithms import FullChanceMCCFRTrainer, full_chance, packet_decks
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle as O
    O.build()
    import full_mccfr_ref as F
    stream = torch.cuda.Stream()
    ctx = _lib.Context(0, stream=stream.cuda_stream)
    deck = _lib.full_deal_py_seed(a.seed)
    _, acts = F.random_root(deck, 4, np.random.RandomState(0))
    decks = packet_decks(deck, 4, 72, 1)

    def state_after(n_rounds):
        s = _lib.FullState(deck=deck)
        for x in acts[:6 * n_rounds]:
            s.step(x)
        return s.s

    rec = dict(bench="full_chance_xplay", runs=1, seed=a.seed, device=torch.cuda.get_device_name(0), batch=a.batch, iterations=a.iterations,
               capacity_log2=a.capacity_log2, calls=a.calls, warmup=a.warmup, hbm_peak_Bps=HBM_PEAK,
               baselines="the host loop (tables_set + exploitability per pair) and the parent's match and exploitability, measured in this run; no threshold is set",
               cross_play={}, pair_match={}, worked_use={})

    def flush():
        line = json.dumps(rec)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return line

    def timed(fn, calls=1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(calls):
            out = fn()
        e1.record(stream)
        stream.synchronize()
        return e0.elapsed_time(e1) / calls, out

    stores = []
    for j in range(16):
        ctx.mccfr_seed(0x5C09A + j)
        h = _lib.FullChanceMCCFR(ctx, decks[:64], state_after(2), a.capacity_log2)
        h.iterate(a.batch, a.iterations)
        stores.append(h)
    rec["rows"] = [h.counters()["rows"] for h in stores]
    third = _lib.FullChanceMCCFR(ctx, decks[:64], state_after(2), a.capacity_log2)
    tables, player1 = [], []
    for h in stores:
        t = h.tables_get()
        tables.append(t)
        player1.append(((t[0][:, 0] >> np.uint64(62)) & np.uint64(1)).astype(bool))

    def host_pair(x, y, root, ds):
        (ka, na, Ra, Sa), (kb, nb, Rb, Sb) = tables[x], tables[y]
        p0, p1 = ~player1[x], player1[y]
        third.tables_set(np.concatenate([ka[p0], kb[p1]]), np.concatenate([na[p0], nb[p1]]), np.concatenate([Ra[p0], Rb[p1]]), np.concatenate([Sa[p0], Sb[p1]]))
        return third.exploitability(root, 0, ds)["value"]

    for R, n, Ks in SHAPES:
        root, ds = state_after(6 - R), decks[:n]
        for K in Ks:
            hs = stores[:K]
            first, out = timed(lambda: _lib.FullChanceMCCFR.cross_play(hs, root, 0, ds))
            timed(lambda: _lib.FullChanceMCCFR.cross_play(hs, root, 0, ds), a.warmup)
            ms, out = timed(lambda: _lib.FullChanceMCCFR.cross_play(hs, root, 0, ds), a.calls)
            timed(lambda: stores[0].exploitability(root, 0, ds), a.warmup)
            ex_ms, _ = timed(lambda: stores[0].exploitability(root, 0, ds), a.calls)
            pairs = [(x, y) for x in range(K) for y in range(K)][:16 if K <= 4 else 8]

            def loop():
                return [host_pair(x, y, root, ds) for x, y in pairs]

            loop_ms, values = timed(loop)
            same = all(np.float64(v).tobytes() == np.float64(out[x, y, 0]).tobytes() for v, (x, y) in zip(values, pairs))
            model = byte_model(R, n, K)
            rec["cross_play"][f"R{R}_decks{n}_K{K}"] = dict(
                leaves=model["leaves"], nodes=model["nodes"], first_ms=first, call_ms=ms, exploitability_ms=ex_ms,
                host_loop=dict(pairs_timed=len(pairs), per_pair_ms=loop_ms / len(pairs), total_ms=loop_ms / len(pairs) * K * K, extrapolated=len(pairs) < K * K,
                               equal_bits=bool(same), speedup=loop_ms / len(pairs) * K * K / ms),
                bytes=model, achieved_Bps=model["total"] / (ms * 1e-3), frac_of_hbm_peak=model["total"] / (ms * 1e-3) / HBM_PEAK,
                reward=out[:, :, 0].tolist())
            flush()
    for h in stores + [third]:
        h.close()

    # the sampled match from the deal's root
    use_decks = packet_decks(deck, 3, 16, 1)
    n = 1 << a.episodes_log2
    pair = []
    for j in range(2):
        ctx.mccfr_seed(0x5C09A + j)
        h = _lib.FullChanceMCCFR(ctx, use_decks[:8], None, 23)
        h.iterate(a.batch, 2)
        pair.append(h)
    timed(lambda: pair[0].pair_match(pair[1], n, 1))
    pm_ms, pm = timed(lambda: pair[0].pair_match(pair[1], n, 1), 3)
    timed(lambda: pair[0].match(n, 1))
    m_ms, m = timed(lambda: pair[0].match(n, 1), 3)
    rec["pair_match"] = dict(episodes=n, decks=8, rows=[h.counters()["rows"] for h in pair], pair_match_ms=pm_ms, match_ms=m_ms, ratio=pm_ms / m_ms,
                             episodes_per_s=n / (pm_ms * 1e-3), pair_match_sums=pm.tolist(), match_sums=m.tolist(),
                             bytes_per_episode_model=30 * 128, achieved_Bps=n * 30 * 128 / (pm_ms * 1e-3),
                             frac_of_hbm_peak=n * 30 * 128 / (pm_ms * 1e-3) / HBM_PEAK,
                             note="30 choice plies an episode, one 128-byte store line each where the pair is held: an upper bound on the bytes, the lines of early rounds are shared by all episodes")
    flush()
    for h in pair:
        h.close()

    # the worked use of the README row
    ctx.mccfr_seed(0x5C09A)
    root_acts = [int(x) for x in acts[:18]]
    A = FullChanceMCCFRTrainer(decks=use_decks[:8], capacity_log2=24, batch=a.batch, ctx=ctx)
    B = FullChanceMCCFRTrainer(decks=use_decks[:8], capacity_log2=24, batch=a.batch, ctx=ctx)
    A.train(a.use_iterations)
    B.train(a.use_iterations)
    same_training = A.counters()["rows"] == B.counters()["rows"]
    B.solve_cfr(a.use_iterations, variant="dcfr", root_actions=root_acts)
    held = use_decks[8:16]

    def clean(e):
        return {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in e.items()}

    rec["worked_use"] = dict(
        iterations=a.use_iterations, batch=a.batch, decks=8, rows=[A.counters()["rows"], B.counters()["rows"]], same_training=bool(same_training),
        cross_play_training=full_chance.cross_play([A, B], root_actions=root_acts).tolist(),
        cross_play_held_out=full_chance.cross_play([A, B], root_actions=root_acts, decks=held).tolist(),
        exploitability_training=[A.exploitability(root_acts), B.exploitability(root_acts)],
        match_training=clean(B.evaluate_vs(A, 1 << 18)), match_held_out=clean(B.evaluate_vs(A, 1 << 18, decks=held)))
    A.close()
    B.close()
    print(flush())
    ctx.close()


if __name__ == "__main__":
    main()
