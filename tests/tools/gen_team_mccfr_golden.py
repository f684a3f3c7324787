"""Writes tests/golden/team_mccfr.npz: the reference's own MCCFRTrainer._sample (src/algorithms/mc_cfr.py) run on TPIMiniScopaGame
(src/envs/openspiel_team_mini_scopa.py) under np.random.seed.  BUILD CONTAINER ONLY: it imports the reference through oracle/refshim.py; the file it
writes holds data only and is what tests/test_team_mccfr_ref.py pins tests/team_mccfr_ref.py to.

Cases: from depth-4 states of the seed-42 and seed-7 deals, 3 iterations of both traversers; and from the root of the seed-42 deal one full iteration().
Per case, everything in the reference's dict insertion order (first visit), nodes named by their place in the tree, so no strings are needed:
    <case>_case        [seed, np.random.seed, iterations, root path ...]
    <case>_n_draws     np.random.choice calls, counted; the global stream afterwards is checked to be the seeded stream advanced by exactly that many
                       random_sample() draws, so <case>_uniforms = those draws (kept for the depth-4 cases; the root case keeps their count, the first and
                       last 8 and regenerates the rest from the seed)
    <case>_rows        the visited choice nodes: row within the root's subtree, level-major (tests/team_cfr_ref.py: Ref.off[d] + mixed-radix path)
    <case>_team        the player of each key, <case>_regret / _strategy [n][4] zero-padded
    <case>_forced      [m][2] (depth-12 node within the subtree, depth 12..15) of the visited forced nodes, <case>_forced_team,
                       <case>_forced_regret / _forced_strategy [m]
    <case>_seconds     wall time of each _sample call here (the reference's Python, one core), in call order

    python tests/tools/gen_team_mccfr_golden.py
"""
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import refshim  # noqa: E402
from gen_team_cfr_golden import savez_reproducible  # noqa: E402

# (name, deal seed, root path of legal-action indices, np.random.seed, iterations, keep the uniforms)
CASES = [("s42_d4", 42, (2, 0, 3, 1), 11, 3, True), ("s7_d4", 7, (0, 1, 2, 3), 12, 3, True), ("s42_root", 42, (), 13, 1, False)]


def main():
    ns = refshim.import_reference()
    tg = importlib.import_module("envs.team_mini_scopa_game")
    ts = importlib.import_module("envs.openspiel_team_mini_scopa")
    import pyspiel
    import team_cfr_ref as T
    game = pyspiel.load_game("team_mini_scopa_tpi")

    def root_state(seed, path):
        st = ts.TPIMiniScopaState(game, env=tg.TeamMiniScopaEnv(seed=seed), skip_reset=True)
        for c in path:
            st.apply_action(st.legal_actions()[c])
        return st

    calls = [0]
    real_choice = np.random.choice

    def counting_choice(*a, **kw):
        calls[0] += 1
        return real_choice(*a, **kw)

    out = {}
    for name, seed, path, np_seed, n_iters, keep in CASES:
        d0 = len(path)
        root = root_state(seed, path)
        trainer = ns.mc.MCCFRTrainer(game)
        np.random.seed(np_seed)
        calls[0] = 0
        np.random.choice = counting_choice
        seconds = []
        try:
            for _ in range(n_iters):
                for p in (0, 1):
                    t0 = time.perf_counter()
                    trainer._sample(root.clone(), p, np.ones(2), np.ones(2))
                    seconds.append(time.perf_counter() - t0)
        finally:
            np.random.choice = real_choice
        n_draws = calls[0]
        after = np.random.get_state()
        np.random.seed(np_seed)
        u = np.random.random_sample(n_draws)
        again = np.random.get_state()
        assert after[2] == again[2] and np.array_equal(after[1], again[1]), "np.random.choice did not draw one random_sample each"

        off, o = {}, 0
        for d in range(d0, 12):
            off[d] = o
            o += T.WIDTH[d] // T.WIDTH[d0]
        rows, team, reg, strat, forced, fteam, freg, fstrat = [], [], [], [], [], [], [], []
        for (player, key), node in trainer.info_sets.items():
            hist = key[key.index(":A[") + 3:-1]
            st, kp = root_state(seed, ()), []
            for a in (int(x) for x in hist.split("-")) if hist else ():
                kp.append(st.legal_actions().index(a))
                st.apply_action(a)
            assert st.information_state_string(st.current_player()) == key and tuple(kp[:d0]) == tuple(path) and st.current_player() == player
            d, idx = len(kp), 0
            for k in range(d0, min(d, 12)):
                idx = idx * T.branch(k) + kp[k]
            if d < 12:
                assert node.regret_sum.size == T.branch(d)
                rows.append(off[d] + idx)
                team.append(player)
                reg.append(np.pad(node.regret_sum, (0, 4 - node.regret_sum.size)))
                strat.append(np.pad(node.strategy_sum, (0, 4 - node.strategy_sum.size)))
            else:
                assert node.regret_sum.size == 1
                forced.append((idx, d))
                fteam.append(player)
                freg.append(node.regret_sum[0])
                fstrat.append(node.strategy_sum[0])
        out[name + "_case"] = np.array([seed, np_seed, n_iters, *path], np.int64)
        out[name + "_n_draws"] = np.array(n_draws, np.int64)
        out[name + "_uniforms"] = u if keep else np.concatenate([u[:8], u[-8:]])
        out[name + "_rows"] = np.array(rows, np.int32)
        out[name + "_team"] = np.array(team, np.int8)
        out[name + "_regret"] = np.array(reg, np.float64).reshape(-1, 4)
        out[name + "_strategy"] = np.array(strat, np.float64).reshape(-1, 4)
        out[name + "_forced"] = np.array(forced, np.int32).reshape(-1, 2)
        out[name + "_forced_team"] = np.array(fteam, np.int8)
        out[name + "_forced_regret"] = np.array(freg, np.float64)
        out[name + "_forced_strategy"] = np.array(fstrat, np.float64)
        out[name + "_seconds"] = np.array(seconds, np.float64)
        print(name, "draws", n_draws, "choice nodes", len(rows), "forced nodes", len(forced), "seconds per _sample call", [round(s, 3) for s in seconds])
    dst = os.path.join(ROOT, "tests", "golden", "team_mccfr.npz")
    savez_reproducible(dst, out)
    print(dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
