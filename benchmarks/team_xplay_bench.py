#!/usr/bin/env python3
"""Team MiniScopa, policy against policy over a set of deals (scopa_team_chance_cross_play / scopa_team_chance_match): time per cross-play call at
K = 1, 4, 16 and per sampled match, next to the two routes to the same numbers that existed before.  Prints one JSON line and writes it to --out.

    python benchmarks/team_xplay_bench.py [--reps 10] [--warmup 2] [--episodes 4194304] [--out profiles/team_xplay_bench.json]

sizes       n = 6 (packet_deals(fix_seat0=True)) and n = 24 (packet_deals), the packets below.  The K tables are random rows normalised over the legal
            slots (padding 0), made on the device.
device      `cross_play_us[K]`: HIP events on the context's stream around --reps scopa_team_chance_cross_play calls after --warmup (three launches per
            call, no host synchronisation inside; the first warm-up call also builds the leaf scopas and the scratch), divided by --reps.
            `match_us`: the same around one scopa_team_chance_match call of --episodes episodes (the call synchronises; the events bracket its launches).
yardsticks  in the same process.  `host_loop_ms[K]`: what a user had to write before -- per (deal, a, b) two TeamChanceGame.policy_for_deal scatters
            and one scopa_team_policy_value on a context holding that deal (scopa_team_set_deal once per deal) -- on the host clock; it gives the reward
            entry only.  `exploitability_ms`: one scopa_team_chance_exploitability call on a device table, host clock: the only earlier call that values a policy on the
            set of deals (against itself and its best responses).
bytes       stated from the code (scopa_team_xplay.hip).  `requested`: per (deal, a, b) every row's map entry (4 B) and table row (32 B) once, every
            depth-12 node's payoff and scopa byte (2 B), the 256 x 32 B subtree values written and read back, 32 B of per-deal image; then the mean reads
            n x K^2 x 32 B and writes K^2 x 32 B.  `unique`: the same with every table row counted once per (deal, table) and the map and leaves once per
            deal -- what has to come from HBM if the caches hold everything the K^2 pairs share.  Match: per episode 12 plies x (4 B map + 32 B row), 2 B
            at the leaf, the draw of the deal costs no memory.
The numbers are not compared here: tests/test_gpu_team_xplay.py holds the kernels to the restatement."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PACKETS = [[0, 5, 10, 15], [1, 4, 11, 14], [2, 7, 8, 13], [3, 6, 9, 12]]
N_CHOICE, N_LEAVES = 321365, 331776
KS = (1, 4, 16)


def cross_play_bytes(n, k):
    pairs = k * k
    mean = n * pairs * 32 + pairs * 32
    requested = n * pairs * (N_CHOICE * 36 + N_LEAVES * 2 + 256 * 64 + 32) + mean
    unique = n * (k * N_CHOICE * 32 + N_CHOICE * 4 + N_LEAVES * 2) + n * pairs * (256 * 64 + 32) + mean
    return dict(requested=requested, unique=unique)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--episodes", type=int, default=1 << 22)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from scopa_amd import _lib
    from scopa_amd.algorithms import team_chance
    stream = torch.cuda.Stream()
    ctx = _lib.Context(0, stream=stream.cuda_stream)
    dev = torch.device("cuda", 0)

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
        nleg = torch.as_tensor(4 - ((keys >> np.uint64(60)).astype(np.int64) >> 2), device=dev)
        gen = torch.Generator(device=dev).manual_seed(1234 + n)
        tables = torch.rand((max(KS), game.G, 4), dtype=torch.float64, device=dev, generator=gen) + 0.05
        tables = torch.where(torch.arange(4, device=dev)[None, None, :] < nleg[None, :, None], tables, torch.zeros_like(tables))
        tables = (tables / tables.sum(2, keepdim=True)).contiguous()
        torch.cuda.synchronize()

        cross_us, cross_bytes, host_ms, checks = {}, {}, {}, {}
        for k in KS:
            out = torch.empty((k, k, 4), dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            call = lambda: game.cross_play(k, tables.data_ptr(), out.data_ptr())
            for _ in range(a.warmup):
                call()
            cross_us[str(k)] = timed(lambda: [call() for _ in range(a.reps)]) / a.reps
            cross_bytes[str(k)] = cross_play_bytes(n, k)
            got = out.cpu().numpy()
            # the route a user had before: per (deal, a, b) two scatters and a synchronising one-deal value pass
            t0 = time.perf_counter()
            loop = np.zeros((n, k, k))
            for d in range(n):
                ctx.team_set_deal(perms[d])
                for ia in range(k):
                    for ib in range(k):
                        la = game.policy_for_deal(tables[ia], d, as_tensor=True)
                        lb = game.policy_for_deal(tables[ib], d, as_tensor=True)
                        loop[d, ia, ib] = ctx.team_policy_value(la.data_ptr(), lb.data_ptr())
            host_ms[str(k)] = 1e3 * (time.perf_counter() - t0)
            s = loop[0].copy()
            for d in range(1, n):
                s = s + loop[d]
            checks[str(k)] = bool(np.array_equal((s / float(n)).view(np.uint64), np.ascontiguousarray(got[..., 0]).view(np.uint64)))

        out4 = (C.c_double * 4)()
        expl = lambda: game.ctx._ck(_lib.lib().scopa_team_chance_exploitability(game._h, C.c_void_p(tables.data_ptr()), C.byref(out4), None, None),
                                    "scopa_team_chance_exploitability")      # the raw call on the device table: no copy of the policy in the timed region
        expl()
        t0 = time.perf_counter()
        expl()
        exploitability_ms = 1e3 * (time.perf_counter() - t0)

        pa, pb = tables[0], tables[1]
        game.match(pa.data_ptr(), pb.data_ptr(), 1 << 16, 1 << 15, 16)
        st = {}
        match_us = timed(lambda: st.update(sums=game.match(pa.data_ptr(), pb.data_ptr(), a.episodes, (a.episodes + 1) // 2, 16)))
        exact = team_chance.cross_play(game, tables[:2])
        rep = team_chance.match_report(st["sums"], exact)
        sizes[str(n)] = dict(n=n, G=game.G, cross_play_us=cross_us, cross_play_bytes=cross_bytes,
                             cross_play_unique_GBps={k: cross_bytes[k]["unique"] / cross_us[k] * 1e-3 for k in cross_us},
                             cross_play_requested_GBps={k: cross_bytes[k]["requested"] / cross_us[k] * 1e-3 for k in cross_us},
                             workgroups={str(k): 256 * n * k * k for k in KS}, lds_bytes_per_workgroup=40160, workgroups_per_cu_by_lds=4,
                             host_loop_ms_host_clock=host_ms, host_loop_gives_the_same_reward_bits=checks,
                             host_loop_over_cross_play={k: host_ms[k] * 1e3 / cross_us[k] for k in cross_us},
                             exploitability_ms_host_clock=exploitability_ms, match_episodes=a.episodes, match_us=match_us,
                             match_episodes_per_s=a.episodes / match_us * 1e6, match_bytes=a.episodes * (12 * 36 + 2),
                             match_reward=rep["reward"], match_exact_reward=rep["exact_reward"], match_exact_std_error=rep["exact_std_error"])
        game.close()

    rec = dict(bench="team_xplay", packets=PACKETS, reps=a.reps, warmup=a.warmup, device=torch.cuda.get_device_name(0), sizes=sizes)
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
