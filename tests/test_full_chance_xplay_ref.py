"""The restatement of FullScopa's store-against-store measures across decks (tests/full_chance_xplay_ref.py) held to code that does not share its
own: one depth-first recursion per deck for every ordered pair and quantity (it adds in another order, hence a tolerance, not bits);
full_chance_exploit_ref.solve on the diagonal, on a merged table off it, and for the pure-response identity; full_chance_ref.match for the pair match
against an empty opponent.  The last section guards the comparisons of tests/test_gpu_full_chance_xplay.py: deliberately wrong variants must differ
from the right one on the inputs used, so that a comparison on bits can tell a wrong kernel from a right one.

Tolerances of section 1: a value is a tree of at most 8 mixes (R = 2) of convex combinations, each adding a relative error of a few ulp (2.2e-16) of
the largest leaf: |r| <= 10.5 and scopas <= 36 give 1e-12 with two orders to spare, r * r <= 110.25 gives 1e-11."""
import numpy as np
import pytest

import full_chance_exploit_ref as XE
import full_chance_ref as W
import full_chance_xplay_ref as XP
import full_mccfr_ref as F
import test_gpu_full_chance_exploit as G            # (fixture builders are plain CPU code; only the module's tests carry the gpu mark)

SEED = 0x5C09A
TOL = np.array([1e-12, 1e-11, 1e-12, 1e-12])
# (round of the root, decks, fixed seat, deck seed): R = 1 and R = 2; the last two are the GPU tests' R = 2 sets.  Below deck 42's roots nobody sweeps
# the table at R = 2, so the scopa quantities are zero there; deck 11's set has leaves with 0..2 and 0..3 scopas (SCOPA_SET)
SETS = [(5, 3, None, 42), (4, 3, 0, 42), (4, 5, 0, 42), (4, 5, 0, 11)]
SCOPA_SET = (4, 5, 0, 11)
_CASES = {}


def planted(tree):
    """(R, S) over every pair of the forest by full_chance_ref.rows_for, with a zero-total strategy row, a one-hot row and a row of no positive regret"""
    pairs = G.level_pairs(tree)
    keys = np.array(pairs, np.uint64).reshape(-1, 2)
    R, S = W.rows_for(keys)
    tR, tS = XE.table_of(keys, R), XE.table_of(keys, S)
    tS[pairs[0]] = [0.0, 0.0, 0.0]
    tS[pairs[1]] = [0.0, 3.0, 0.0]
    tS[pairs[-1]] = [1e-13, 0.0, 0.0]
    tR[pairs[0]] = [-1.0, 0.0, -2.0]
    tR[pairs[2]] = [0.0, 0.0, 5.0] if W.key_actions(pairs[2]) == 3 else [0.0, 5.0, 0.0]
    return tR, tS


def case(oracle, r0, n, fix_seat, deck_seed=42):
    """(root, decks, forest, the tables of three stores: trained by 3 restated iterations at batch 4, planted, empty), computed once"""
    if (r0, n, fix_seat, deck_seed) not in _CASES:
        decks, _, root = G.packet(oracle, r0, n, fix_seat, deck_seed)
        rows, counter = W.Rows(), 0
        for _ in range(3):
            counter = W.iterate(root, decks, 4, SEED, rows, counter)
        tree = XP.tree_of(root, decks, 6 - r0)
        _CASES[r0, n, fix_seat, deck_seed] = (root, decks, tree, [(rows.R, rows.S), planted(tree), ({}, {})])
    return _CASES[r0, n, fix_seat, deck_seed]


def policy_of(table, which):
    R, S = table
    return (lambda key, n: F.average_probs(S, key, n)) if which == 0 else (lambda key, n: F.sigma_of(R.get(key, [0.0] * 3), n))


def dfs(st, pols):
    """[K][K][4] below `st` on the deck it carries: entry [a][b] for pols[a] as player 0 against pols[b] as player 1"""
    K = len(pols)
    if st.s.terminal:
        r = st.s.r2[0] / 2.0
        return np.broadcast_to(np.array([r, r * r, float(st.s.scopas[0]), float(st.s.scopas[1])]), (K, K, 4))
    p = st.s.step & 1
    h = sorted(F.hand(st, p))
    if len(h) == 1:
        return dfs(F.child(st, h[0]), pols)
    key = W.wide_key(st, p)
    P = np.array([pol(key, len(h)) for pol in pols])                        # [K][n]
    out = np.zeros((K, K, 4))
    for s, c in enumerate(h):
        w = P[:, s][:, None, None] if p == 0 else P[:, s][None, :, None]
        out = out + w * dfs(F.child(st, c), pols)
    return out


# ---- 1. a depth-first recursion per deck, every ordered pair and quantity ------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("r0,n,fix_seat,deck_seed", SETS)
def test_cross_play_by_depth_first_recursion(oracle, r0, n, fix_seat, deck_seed, which):
    root, decks, tree, tables = case(oracle, r0, n, fix_seat, deck_seed)
    got = XP.cross_play(tree, tables, which)
    pols = [policy_of(t, which) for t in tables]
    want = sum(dfs(W.root_on(root, d), pols) for d in decks) / len(decks)
    assert got.shape == (3, 3, 4) and np.all(np.abs(got - want) <= TOL), np.abs(got - want).max(axis=(0, 1))
    assert np.all(got[:, :, 1] >= got[:, :, 0] ** 2 - 1e-11) and np.all(got[:, :, 2:] >= 0.0)       # a second moment and two counts
    assert len({got[a, b, 0] for a in range(3) for b in range(3)}) == 9                             # nine different games
    assert np.array_equal(got[2, 2], want[2, 2]) or np.all(np.abs(got[2, 2] - want[2, 2]) <= TOL)


def test_leaves_carry_the_four_quantities(oracle):
    root, decks, tree, _ = case(oracle, *SCOPA_SET)
    levels, leaf4, n = tree
    ex = G.tree_of(root, decks, 2)
    assert n == 5 and [k for _, _, k in levels] == [k for _, _, k in ex[0]] and leaf4[0] == ex[1]      # the forest of exploitability, node for node
    assert leaf4[1] == [x * x for x in leaf4[0]] and all(len(q) == 5 * 1296 for q in leaf4)
    assert max(leaf4[2]) >= 1.0 and max(leaf4[3]) >= 1.0 and len(set(zip(leaf4[2], leaf4[3]))) > 2     # scopas are made below the root


# ---- 2. the existing route: exploitability's value on the diagonal and on a merged table off it -------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("r0,n,fix_seat,deck_seed", SETS)
def test_diagonal_and_merged_store_are_solves_value_on_bits(oracle, r0, n, fix_seat, deck_seed, which):
    root, decks, tree, tables = case(oracle, r0, n, fix_seat, deck_seed)
    ex_tree = G.tree_of(root, decks, 6 - r0)
    got = XP.cross_play(tree, tables, which)
    for a, (R, S) in enumerate(tables):
        assert G.same_bits(got[a, a, 0], XE.solve(ex_tree, R, S, which)["out4"][3])
    player = lambda k: (k[0] >> 62) & 1
    for a, b in ((0, 1), (1, 0), (0, 2), (2, 1)):
        R = {**{k: v for k, v in tables[a][0].items() if player(k) == 0}, **{k: v for k, v in tables[b][0].items() if player(k) == 1}}
        S = {**{k: v for k, v in tables[a][1].items() if player(k) == 0}, **{k: v for k, v in tables[b][1].items() if player(k) == 1}}
        assert G.same_bits(got[a, b, 0], XE.solve(ex_tree, R, S, which)["out4"][3]), (a, b)


# ---- 3. a pure response planted as a store plays to the value the response pass reports ---------------------------------------------------------------
def hot_table(rows):
    keys, n_act, action, _ = rows
    return {tuple(k): [1.0 if s == a else 0.0 for s in range(3)] for k, a in zip(keys.tolist(), action)}


@pytest.mark.parametrize("r0,n,fix_seat,deck_seed", SETS)
def test_pure_response_identity(oracle, r0, n, fix_seat, deck_seed):
    root, decks, tree, tables = case(oracle, r0, n, fix_seat, deck_seed)
    ex_tree = G.tree_of(root, decks, 6 - r0)
    for a in (0, 1):
        R, S = tables[a]
        res = XE.solve(ex_tree, R, S, 0)
        hot0, hot1 = hot_table(res["rows"][0]), hot_table(res["rows"][1])
        got = XP.cross_play(tree, [(R, S), ({}, hot0), ({}, hot1)], 0)
        assert got[1, 0, 0] == res["out4"][1] and got[0, 2, 0] == -res["out4"][2]                  # (==, not bits: a signed zero may differ)
        assert res["out4"][1] != res["out4"][3] and -res["out4"][2] != res["out4"][3]              # the responses are not the policy itself


# ---- 4. the pair match against an opponent without rows is the match against uniform play ----------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 65, 400])
def test_pair_match_with_an_empty_opponent_is_match(oracle, n):
    root, decks, _, tables = case(oracle, 4, 5, 0)
    other = {k: v for k, v in tables[1][1].items() if ((k[0] >> 59) & 7) == 7}                   # rows, but of no pair ever met
    for S_b in ({}, other):
        sums, r2 = XP.pair_match(root, decks, tables[0][1], S_b, n, SEED, 5)
        want, want_r2 = W.match(root, decks, tables[0][1], n, SEED, 5)
        assert np.array_equal(sums, want) and np.array_equal(r2, want_r2)


def test_pair_match_reads_the_opponents_rows(oracle):
    root, decks, _, tables = case(oracle, 4, 5, 0)
    a, b = tables[0][1], tables[1][1]
    sums, r2 = XP.pair_match(root, decks, a, b, 400, SEED, 5)
    _, r2_uni = W.match(root, decks, a, 400, SEED, 5)
    assert not np.array_equal(r2, r2_uni)                                                          # the opponent is not uniform play
    back, r2_back = XP.pair_match(root, decks, b, a, 400, SEED, 5)
    assert not np.array_equal(r2_back, r2) and not np.array_equal(back, sums)                      # nor is the match symmetric in its stores
    assert sums[0] == r2[:200].astype(np.int64).sum() and sums[1] == r2[200:].astype(np.int64).sum()
    assert sums[2] + sums[3] == (r2.astype(np.int64) ** 2).sum()


# ---- 5. guards: wrong variants differ on the inputs the GPU comparison uses ---------------------------------------------------------------------------
@pytest.mark.parametrize("r0,n,fix_seat,deck_seed", SETS)
def test_guard_prob_b_at_player_0s_levels_differs(oracle, r0, n, fix_seat, deck_seed):
    root, decks, tree, tables = case(oracle, r0, n, fix_seat, deck_seed)
    for which in (0, 1):
        right, wrong = XP.cross_play(tree, tables, which), XP.cross_play(tree, tables, which, swap_levels=True)
        for a in range(3):
            assert G.same_bits(right[a, a], wrong[a, a])                                           # the diagonal cannot tell
            for b in range(3):
                if a != b:                                                                         # (deck 42's sets have no scopas to tell by)
                    assert all(right[a, b, q] != wrong[a, b, q] for q in (range(4) if deck_seed == 11 else (0, 1))), (which, a, b)
        assert G.same_bits(np.swapaxes(right, 0, 1), wrong)                                        # the wrong kernel computes the transposed matrix


@pytest.mark.parametrize("r0,n,fix_seat,deck_seed", SETS)
def test_guard_slots_in_hand_order_differ(oracle, r0, n, fix_seat, deck_seed):
    root, decks, tree, tables = case(oracle, r0, n, fix_seat, deck_seed)
    wrong_tree = XP.tree_of(root, decks, 6 - r0, hand_order=True)
    right, wrong = XP.cross_play(tree, tables, 0), XP.cross_play(wrong_tree, tables, 0)
    assert all(right[a, b, 0] != wrong[a, b, 0] for a in range(2) for b in range(2))               # stores with rows: the row's slots name other cards
    assert abs(right[2, 2, 0] - wrong[2, 2, 0]) <= 1e-12                                           # uniform play does not care


def test_guard_the_four_quantities_differ_and_the_second_moment_is_no_square(oracle):
    root, decks, tree, tables = case(oracle, *SCOPA_SET)
    got = XP.cross_play(tree, tables, 0)
    assert np.all(got[:, :, 1] > got[:, :, 0] ** 2 + 0.1)                                          # E[r^2] is not E[r]^2: a kernel that squares late shows
    assert np.all(got[:, :, 2] != got[:, :, 3])                                                    # the two scopa counts are not swapped unseen
