"""Writes tests/golden/team_cfr.npz: the reference's own CFRTrainer._cfr_recursive (src/algorithms/vanilla_cfr.py) run on TPIMiniScopaGame
(src/envs/openspiel_team_mini_scopa.py) from depth-4 states.  BUILD CONTAINER ONLY: it imports the reference through oracle/refshim.py; the file it
writes holds data only and is what tests/test_team_cfr_ref.py pins tests/team_cfr_ref.py to.

Per case (seed, root path of legal-action indices, reaches), after 3 iterations of both traversers, everything in the reference's dict insertion
order (DFS pre-order), so no strings are needed:
    <case>_root_values   [6]        the traversals' return values, (iteration, traverser) order
    <case>_regret / _strategy / _local   [1255][4]   the choice nodes' arrays, zero-padded
    <case>_forced_strategy   [5184]   strategy_sum of the forced nodes (their regret_sum is checked to be 0 and local_strategy 1 here)
and once: 32 sampled information-state strings of the seed-42 cases with their paths (`keys`, `key_paths` padded with -1), to pin the key parser.

    python tests/tools/gen_team_cfr_golden.py
"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import refshim  # noqa: E402

CASES = [("s42_a", 42, (2, 0, 3, 1), (1.0, 1.0)), ("s42_b", 42, (0, 0, 0, 0), (1.0, 1.0)), ("s7_a", 7, (2, 0, 3, 1), (1.0, 1.0)),
         ("s7_b", 7, (0, 0, 0, 0), (1.0, 1.0)), ("s42_a_reach", 42, (2, 0, 3, 1), (0.75, 0.3))]
N_ITERS = 3


def savez_reproducible(path, arrays):
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            zi = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            z.writestr(zi, buf.getvalue())


def main():
    ns = refshim.import_reference()
    tg = importlib.import_module("envs.team_mini_scopa_game")
    ts = importlib.import_module("envs.openspiel_team_mini_scopa")
    import pyspiel
    game = pyspiel.load_game("team_mini_scopa_tpi")

    def root_state(seed, path):
        st = ts.TPIMiniScopaState(game, env=tg.TeamMiniScopaEnv(seed=seed), skip_reset=True)
        for c in path:
            st.apply_action(st.legal_actions()[c])
        return st

    out, sampled = {}, []
    rng = np.random.RandomState(12)
    for name, seed, path, (r0, r1) in CASES:
        root = root_state(seed, path)
        trainer = ns.vanilla.CFRTrainer(game)
        values = [trainer._cfr_recursive(root.clone(), p, r0, r1) for _ in range(N_ITERS) for p in (0, 1)]
        nodes = list(trainer.info_set_map.items())
        choice = [n for _, n in nodes if n.legal_actions.size > 1]
        forced = [n for _, n in nodes if n.legal_actions.size == 1]
        assert (len(choice), len(forced)) == (1255, 5184), (len(choice), len(forced))
        assert all(n.regret_sum[0] == 0.0 and n.local_strategy[0] == 1.0 for n in forced)

        def pad(rows):
            a = np.zeros((len(rows), 4))
            for i, r in enumerate(rows):
                a[i, :r.size] = r
            return a

        out[name + "_root_values"] = np.array(values, np.float64)
        out[name + "_regret"] = pad([n.regret_sum for n in choice])
        out[name + "_strategy"] = pad([n.strategy_sum for n in choice])
        out[name + "_local"] = pad([n.local_strategy for n in choice])
        out[name + "_forced_strategy"] = np.array([n.strategy_sum[0] for n in forced], np.float64)
        out[name + "_case"] = np.array([seed, *path], np.int64)
        out[name + "_reaches"] = np.array([r0, r1], np.float64)
        if seed == 42 and (r0, r1) == (1.0, 1.0):
            for i in sorted(rng.choice(len(nodes), 16, replace=False)):
                key = nodes[i][0]
                hist = key[key.index(":A[") + 3:-1]
                st, kp = root_state(seed, ()), []
                for a in (int(x) for x in hist.split("-")):
                    kp.append(st.legal_actions().index(a))
                    st.apply_action(a)
                assert st.information_state_string(st.current_player()) == key
                sampled.append((key, kp))
        print(name, "values", values)
    out["keys"] = np.array([k for k, _ in sampled])
    out["key_paths"] = np.array([p + [-1] * (16 - len(p)) for _, p in sampled], np.int8)
    dst = os.path.join(ROOT, "tests", "golden", "team_cfr.npz")
    savez_reproducible(dst, out)
    print(dst, os.path.getsize(dst), "bytes;", len(sampled), "keys, depths", sorted({len(p) for _, p in sampled}))


if __name__ == "__main__":
    main()
