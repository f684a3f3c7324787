#!/usr/bin/env python3
"""Team MiniScopa solved on the device (scopa_team_cfr_iterate) against the two host routes a user had before it.  Prints one JSON line (and writes
it to --out).

    python benchmarks/team_cfr_bench.py [--seed 42] [--iters 200] [--warmup 20] [--host-iters 3] [--out profiles/team_cfr_bench.json]
                                        [--reference-root /path/to/reference [--reference-only]] [--reference-subtree-s SECONDS]

device      `iteration_us`: HIP events on the context's stream around one scopa_team_cfr_iterate call of --iters iterations after --warmup
            (four launches per iteration, no host synchronisation inside), divided by --iters.  `launch_us`: the same around --iters single launches of each
            of the two kernels (scopa_team_cfr_launch), per traverser.  `value_pass_us`: scopa_team_minimax (two launches and one 8-byte copy), host clock.
bytes       `bytes_per_traversal`: what one traversal moves, stated from the code (scopa_team_cfr.hip), per traverser: every row's sigma (32 B) is read
            once and written once, its regret row read once; the traverser's rows also read their strategy row and write both; every depth-12 node reads
            its payoff byte and reads and writes the traverser's leaf_reach_sum; the 256 subtree values cross once each way.  The four ancestor rows each
            subtree workgroup reads again (256 x 4 x 32 B) are counted too.
host        `numpy_iteration_ms`: the float64 restatement tests/team_cfr_ref.py (level-vectorised numpy, one core), mean of --host-iters iterations.
reference   `reference_python_iteration_s_extrapolated`: ONLY with --reference-root (a checkout of the reference; --reference-only skips everything that
            needs a GPU) or with --reference-subtree-s (the figure such a run printed, measured on another machine's CPU: recorded as given).  One
            traversal of a depth-4 subtree by the reference's own CFRTrainer._cfr_recursive is timed (7 735 nodes) and scaled by the tree's 1 980 245
            nodes, two traversals per iteration: an EXTRAPOLATION, not a measurement of a whole iteration.
The device tables after --warmup + --iters iterations from reset are not compared here: tests/test_gpu_team_cfr.py holds the kernels to the restatement."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_CHOICE, N_LEAVES, N_NODES = 321365, 331776, 1980245
TEAM_ROWS = (1 + 4 + 256 + 768 + 20736 + 41472, 16 + 64 + 2304 + 6912 + 82944 + 165888)     # rows of team 0 (depths 0, 1, 4, 5, 8, 9) and team 1


def bytes_per_traversal(trav):
    sigma = N_CHOICE * 32 * 2 + 256 * 4 * 32            # read + written once, plus the subtree workgroups' ancestor rows
    regret = N_CHOICE * 32 + TEAM_ROWS[trav] * 32       # read everywhere, written on the traverser's rows
    strategy = TEAM_ROWS[trav] * 32 * 2
    leaves = N_LEAVES * (1 + 8 + 8)
    return sigma + regret + strategy + leaves + 256 * 8 * 2 + 8


def reference_leg(a):
    """the reference-Python figure: timed here from a checkout, or folded in as given; always labelled an extrapolation"""
    dt = a.reference_subtree_s
    if a.reference_root:
        import importlib
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import refshim
        ns = refshim.import_reference(a.reference_root)
        tg = importlib.import_module("envs.team_mini_scopa_game")
        ts = importlib.import_module("envs.openspiel_team_mini_scopa")
        import pyspiel
        game = pyspiel.load_game("team_mini_scopa_tpi")
        st = ts.TPIMiniScopaState(game, env=tg.TeamMiniScopaEnv(seed=a.seed), skip_reset=True)
        for c in (2, 0, 3, 1):
            st.apply_action(st.legal_actions()[c])
        tr = ns.vanilla.CFRTrainer(game)
        t0 = time.perf_counter()
        tr._cfr_recursive(st, 0, 1.0, 1.0)
        dt = time.perf_counter() - t0
    if dt is None:
        return {}
    return dict(reference_python_subtree_traversal_s=dt, reference_python_iteration_s_extrapolated=dt * N_NODES / 7735 * 2,
                reference_python_note="extrapolated from one depth-4 subtree traversal (7 735 of 1 980 245 nodes)"
                                      + ("" if a.reference_root else ", timed on another machine's CPU") + ": not a measured iteration")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--reference-root", default=None)
    ap.add_argument("--reference-only", action="store_true")
    ap.add_argument("--reference-subtree-s", type=float, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.iters >= 200, "at least 200 iterations after warm-up"
    if a.reference_only:
        print(json.dumps(reference_leg(a)))
        return
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

    ctx.team_cfr_iterate(a.warmup, root_values=False)
    iteration_us = timed(lambda: ctx.team_cfr_iterate(a.iters, root_values=False)) / a.iters
    launch_us = {}
    for p in (0, 1):
        for part, name in ((0, "subtrees"), (1, "top")):
            for _ in range(5):
                ctx.team_cfr_launch(p, part)
            launch_us[f"{name}_traverser{p}"] = timed(lambda: [ctx.team_cfr_launch(p, part) for _ in range(a.iters)]) / a.iters
    ctx.team_minimax()
    t0 = time.perf_counter()
    for _ in range(20):
        vstar = ctx.team_minimax()
    value_pass_us = 1e6 * (time.perf_counter() - t0) / 20
    expl = ctx.team_exploitability()
    bpt = [bytes_per_traversal(0), bytes_per_traversal(1)]
    rec = dict(bench="team_cfr", seed=a.seed, iters=a.iters, warmup=a.warmup, device=torch.cuda.get_device_name(0), iteration_us=iteration_us, launch_us=launch_us,
               launches_per_iteration=4, value_pass_us_host_clock=value_pass_us, bytes_per_traversal=bpt, bytes_per_iteration=sum(bpt),
               effective_GBps=sum(bpt) / iteration_us * 1e-3, minimax_value=vstar, exploitability_after_run=float(expl[0]))

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle as O
    O.build()
    import team_cfr_ref as T
    ref = T.Ref(perm)
    tabs = ref.tables()
    ref.iterate(*tabs, 1)
    t0 = time.perf_counter()
    ref.iterate(*tabs, a.host_iters)
    rec["numpy_iteration_ms"] = 1e3 * (time.perf_counter() - t0) / a.host_iters
    rec["speedup_vs_numpy"] = rec["numpy_iteration_ms"] * 1e3 / iteration_us

    rec.update(reference_leg(a))
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
