"""CPU checks of tests/full_chance_frontier_ref.py, the restatement the GPU suite of the frontier traversal (test_gpu_full_chance_frontier.py) is held
to, and of what the feature adds on the host: names in header, binding and library, the row counts beyond the forest's cap, the solver's argument.

The restatement's level-by-level walk is held to a plain depth-first recursive external-sampling traversal over real states that asks the policy one
node at a time, with the float64 forward pass of exact-arithmetic nets (bit-exact in float32) as the policy."""
import os
import re

import numpy as np
import pytest

import full_chance_frontier_ref as FR
import full_chance_ref as W
import full_chance_sdcfr_ref as S
import full_mccfr_ref as F

from conftest import ROOT

SEED = 0x5C09A
NEW = ("scopa_full_chance_sdcfr_traverse_frontier", "scopa_full_chance_sdcfr_policy_at", "scopa_full_chance_debug_sdcfr_scratch")


def game_of(oracle, R, n):
    from scopa_amd.algorithms import packet_decks
    r0 = 6 - R
    deck = oracle.full_deal_py_seed(42)
    st, _ = F.random_root(deck, r0, np.random.RandomState(100 * r0 + 42))
    return st, packet_decks(deck, r0, n, 5, fix_seat=0)


def dfs(root, deck, trav, tid, iteration, policy_fn):
    """depth first over real states, one node at a time -> (value, rows {rank: (pair, regret [40])}, visits, widths {level: paths})"""
    R = 6 - int(root.s.round_number)
    rank0, w, r = {}, 1, 0
    for k in range(4 * R):
        if (k & 1) == trav:
            rank0[k] = r
            r += w
            w *= S.CARDS[k & 3]
    rows, visits = {}, [0]

    def rec(st, k, p):
        if st.s.terminal:
            v = np.float32(st.s.r2[0] / 2.0)
            return v if trav == 0 else np.float32(-v)
        mover = int(st.s.step) & 1
        hand = sorted(F.hand(st, mover))
        if len(hand) == 1:
            return rec(F.child(st, hand[0]), k, p)
        n = len(hand)
        assert mover == (k & 1) and n == S.CARDS[k & 3]
        visits[0] += 1
        key = W.wide_key(st, mover)
        pol, thr = policy_fn(np.array([key], np.uint64), mover)
        if mover != trav:
            a = S.action_of(thr[0], FR.draw_N(k, p, tid, iteration, trav, SEED), n)
            return rec(F.child(st, hand[a]), k + 1, p)
        av = [rec(F.child(st, hand[a]), k + 1, p * n + a) for a in range(n)]
        v, ri, d = S.row_of(pol[0], av, n)
        assert rank0[k] + p not in rows
        rows[rank0[k] + p] = (key, S.regret_row(key[1], ri, d))
        return v

    return rec(W.root_on(root, deck), 0, 0), rows, visits[0]


@pytest.mark.parametrize("R,n", [(1, 3), (2, 2)])
def test_walk_frontier_equals_depth_first_recursion(oracle, R, n):
    root, decks = game_of(oracle, R, n)
    nets = [S.exact_net(7), S.exact_net(8)]
    fn = FR.host_policy_fn(nets, exact=True)
    drawn = set()
    for trav in (0, 1):
        for d in range(n):
            tid = (7 * d + trav, (1 << 32) - 1)[d == n - 1]
            got = FR.walk_frontier(root, decks[d], trav, tid, 5, SEED, fn)
            value, rows, visits = dfs(root, decks[d], trav, tid, 5, fn)
            assert np.float32(got["value"]).tobytes() == np.float32(value).tobytes()
            assert visits == got["visits"] == S.visits_per_traversal(R, trav) == (13, 8)[trav] * (6 ** R - 1) // 5
            assert sorted(rows) == sorted(got["rows"]) == list(range(S.rows_per_traversal(R)))
            for rank, (key, reg) in rows.items():
                assert got["rows"][rank][0] == key and got["rows"][rank][1].tobytes() == reg.tobytes(), (trav, d, rank)
            # rank order: level-major over the traverser's levels (the round bits and the held cards never go down), ascending path within
            lv = [((key[0] >> 59) & 7, -bin(key[1]).count("1")) for key, _ in (got["rows"][r] for r in range(len(rows)))]
            assert lv == sorted(lv)
            drawn.update(got["path"].values())
    assert len(drawn) > 1                                                  # the draws are not all one slot


def test_new_names_and_row_counts(sl):
    hdr = open(os.path.join(ROOT, "include", "scopa.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = sl.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in sl.SYMBOLS and hasattr(L, name) and getattr(L, name).argtypes is not None
    assert L.scopa_full_chance_sdcfr_traverse_frontier.argtypes == L.scopa_full_chance_sdcfr_traverse.argtypes
    assert all(hasattr(sl.FullChanceMCCFR, m) for m in ("sdcfr_traverse_frontier", "debug_sdcfr_scratch"))
    assert all(hasattr(sl.Context, m) for m in ("full_chance_sdcfr_policy_at", "full_chance_debug_sdcfr_scratch"))
    from scopa_amd.algorithms.deep_cfr.full_chance_deep_cfr import default_memory_size, rows_per_traversal
    assert [rows_per_traversal(r) for r in (5, 6)] == [S.rows_per_traversal(5), S.rows_per_traversal(6)] == [6220, 37324]
    assert [S.visits_per_traversal(r, t) for r in (5, 6) for t in (0, 1)] == [20215, 12440, 121303, 74648]
    assert default_memory_size(6, 1, 1) == 8 * 37324
    # refusals that need no GPU: they come before the device is touched
    assert L.scopa_full_chance_sdcfr_policy_at(None, 0, None, 0, *([None] * 8)) == sl.SCOPA_EINVAL
    assert L.scopa_full_chance_debug_sdcfr_scratch(None, 0) == sl.SCOPA_EINVAL
    assert L.scopa_full_chance_sdcfr_traverse_frontier(None, None, 0, 1, 0, None, *([None] * 8), 1, 0, None, 0, 0) == sl.SCOPA_EINVAL
    import inspect
    from scopa_amd.algorithms.deep_cfr import FullChanceDeepCFR
    assert inspect.signature(FullChanceDeepCFR.__init__).parameters["traversal"].default == "forest"
    for fn in ("exploitability", "policy_store", "evaluate_vs_random"):
        assert inspect.signature(getattr(FullChanceDeepCFR, fn)).parameters["root_actions"].default is None
