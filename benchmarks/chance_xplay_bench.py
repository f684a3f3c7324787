#!/usr/bin/env python3
"""Policy against policy on the chance game over the 495-deal hidden-hand set (chance.hidden_hand_deals([0, 5, 10, 15])): scopa_chance_cross_play,
scopa_chance_best_response and scopa_chance_match against what a user had before them.  Prints one JSON line (and writes it to --out).

    python benchmarks/chance_xplay_bench.py [--sizes 1,16,64] [--reps 10] [--episodes 4194304] [--out profiles/chance_xplay_bench.json]

cross-play    `cross_play_ms`: HIP events on the context's stream around one call (median of --reps after warm-up, the two launches alone).
              `composition_ms`: the host clock around the route without it -- per deal scopa_set_deal on a second context, K
              scopa_chance_policy_for_deal scatters, scopa_cross_play, a copy out; the 495 results summed on the host in deal order (median of 3).
              `composition_set_deal_ms` is the part of it spent in scopa_set_deal, for a reader who keeps 495 contexts alive instead.
best response `best_response_ms` (with and without the tables): HIP events as above.  `exploitability_calls_ms`: the host clock around K
              scopa_chance_exploitability calls with an explicit policy (median of 3).
match         `match_ms`: the host clock around one synchronous call of --episodes episodes (median of 5 after warm-up), and episodes per second.
The K tables are seeded Dirichlet rows over the keys; every number two routes share is checked to agree bit for bit (`same_bits`)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def event_ms(stream, fn, reps):
    import torch
    for _ in range(2):
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


def composition(L, game, one, perms, n_infosets, d_pol, K):
    """today's route to the cross-play matrix -> (matrix [K][K][4], ms in all, ms in scopa_set_deal)"""
    import torch
    G = game.G
    d_local = torch.empty((K, 1653, 4), dtype=torch.float64, device="cuda:0")
    d_mat = torch.empty((K, K, 4), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    t0, t_deal, per = time.perf_counter(), 0.0, []
    for d, perm in enumerate(perms):
        t1 = time.perf_counter()
        I = one.set_deal(perm)
        t_deal += time.perf_counter() - t1
        assert I == int(n_infosets[d])
        local = d_local.view(-1)[:K * I * 4].view(K, I, 4)
        for k in range(K):
            rc = L.scopa_chance_policy_for_deal(game._h, C.c_void_p(d_pol.data_ptr() + k * G * 32), d, C.c_void_p(local.data_ptr() + k * I * 32))
            assert rc == 0
        one.cross_play(K, local.data_ptr(), d_mat.data_ptr())
        one.synchronize()
        per.append(d_mat.cpu().numpy())
    s = per[0].copy()
    for x in per[1:]:
        s = s + x
    s = s / float(len(per))
    return s, 1e3 * (time.perf_counter() - t0), 1e3 * t_deal


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,16,64")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--episodes", type=int, default=1 << 22)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from scopa_amd import _lib
    from scopa_amd.algorithms import chance
    L = _lib.lib()
    stream = torch.cuda.Stream()
    ctx = _lib.Context(0, stream=stream.cuda_stream)
    one = _lib.Context(0)
    perms = chance.hidden_hand_deals([0, 5, 10, 15])
    multi = _lib.MultiDeal(ctx, len(perms))
    multi.set_perms(perms)
    n_infosets = multi.build()
    game = _lib.ChanceGame(multi)
    G, n = game.G, game.n
    keys, _ = game.index()
    nlegal = ((keys >> np.uint64(1)) & np.uint64(7)).astype(np.int64)
    legal = np.arange(4)[None, :] < nlegal[:, None]
    rng = np.random.default_rng(495)
    out = {"bench": "chance_xplay", "device": torch.cuda.get_device_name(0), "deals": n, "keys": G, "largest_deal_infosets": int(n_infosets.max()),
           "reps": args.reps, "by_K": {}}
    sizes = [int(x) for x in args.sizes.split(",")]
    for K in sizes:
        gam = np.where(legal[None], rng.gamma(0.7, size=(K, G, 4)), 0.0)
        pols = gam / gam.sum(2, keepdims=True)
        d_pol = torch.as_tensor(pols, device="cuda:0")
        d_mat = torch.empty((K, K, 4), dtype=torch.float64, device="cuda:0")
        d_br = torch.empty((K, 2, G, 4), dtype=torch.float64, device="cuda:0")
        d_out4 = torch.empty((K, 4), dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        reps = args.reps if K < 64 else max(args.reps // 2, 3)
        r = {"workgroups": n * K * K,
             "cross_play_ms": round(event_ms(stream, lambda: game.cross_play(K, d_pol.data_ptr(), d_mat.data_ptr()), reps), 4)}
        mats, ts, tds = None, [], []
        for _ in range(3 if K < 64 else 1):
            mats, t, td = composition(L, game, one, perms, n_infosets, d_pol, K)
            ts.append(t)
            tds.append(td)
        r["composition_ms"], r["composition_set_deal_ms"] = round(statistics.median(ts), 3), round(statistics.median(tds), 3)
        r["best_response_ms"] = round(event_ms(stream, lambda: game.best_response(K, d_pol.data_ptr(), d_br.data_ptr(), d_out4.data_ptr()), reps), 4)
        r["best_response_no_tables_ms"] = round(event_ms(stream, lambda: game.best_response(K, d_pol.data_ptr(), 0, d_out4.data_ptr()), reps), 4)
        game.exploitability(pols[0])
        ts = []
        for _ in range(3 if K < 64 else 1):
            t0 = time.perf_counter()
            each = [game.exploitability(p) for p in pols]
            ts.append(1e3 * (time.perf_counter() - t0))
        r["exploitability_calls_ms"] = round(statistics.median(ts), 3)
        stream.synchronize()
        want = np.array(each)
        got4, got = d_out4.cpu().numpy(), d_mat.cpu().numpy()
        r["same_bits"] = bool(np.array_equal(got4.view(np.uint64), want.view(np.uint64))
                              and np.array_equal(got.view(np.uint64), np.ascontiguousarray(mats).view(np.uint64))
                              and np.array_equal(np.ascontiguousarray(np.diagonal(got[..., 0])).view(np.uint64), want[:, 3].copy().view(np.uint64)))
        out["by_K"][K] = r
        del d_pol, d_br, d_mat, d_out4
    # the match: two Dirichlet tables, --episodes episodes, seats split evenly
    gam = np.where(legal[None], rng.gamma(0.7, size=(2, G, 4)), 0.0)
    d_pair = torch.as_tensor(gam / gam.sum(2, keepdims=True), device="cuda:0")
    torch.cuda.synchronize()
    N = int(args.episodes)
    ts, st = [], None
    for i in range(7):
        t0 = time.perf_counter()
        st = game.match(d_pair[0].data_ptr(), d_pair[1].data_ptr(), N, (N + 1) // 2, 16)
        if i >= 2:
            ts.append(1e3 * (time.perf_counter() - t0))
    ms = statistics.median(ts)
    out["match"] = {"episodes": N, "match_ms": round(ms, 3), "match_ms_min_max": [round(min(ts), 3), round(max(ts), 3)],
                    "episodes_per_s": round(N / (ms * 1e-3)), "episodes_counted": int(st[:, 0].sum())}
    game.close()
    multi.close()
    one.close()
    ctx.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
