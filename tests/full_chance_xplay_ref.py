"""CPU restatement of FullScopa over decks, store against store (scopa_amd/csrc/scopa_full_chance_xplay.hip; the procedures are stated under
`cross_play` and `pair_match` of scopa_full_chance in include/scopa.h) on full_chance_ref's wide_key and root_on, full_mccfr_ref's child, hand,
average_probs, sigma_of and pick, and full_exploit_ref's mix_up, in float64 and in the procedure's own order of adds.

TEST INFRASTRUCTURE.  It follows the steps literally -- a deck-major forest of one tree per evaluated deck, action slots in ascending card id, one
prob image per store, per ordered pair and quantity the bottom-up mix in slot order, root sums in deck order -- so the device's results are compared
with it on bits; tests/test_full_chance_xplay_ref.py holds it in turn to depth-first recursions, to full_chance_exploit_ref.solve and to
full_chance_ref.match.

  tree_of     step 1: (levels, leaf4, n_decks); levels as full_chance_exploit_ref.tree_of's, leaf4 = four lists: r = r2_p0 / 2.0, r * r, scopas[0],
              scopas[1] of the n 36^R terminal states
  cross_play  steps 2-3 -> float64 [K][K][4] for K tables (R, S), each {(A, B): [3]}
  pair_match  full_chance_ref.match with the opponent playing average_probs of its own rows
Variants for the separation guards (test_full_chance_xplay_ref.py): cross_play(swap_levels=True) takes prob_b at player 0's levels and prob_a at
player 1's; tree_of(hand_order=True) takes slots in hand order."""
import numpy as np

import oracle as O
import full_chance_ref as W
import full_exploit_ref as X
import full_mccfr_ref as F


def tree_of(root, decks, R, hand_order=False):
    assert not root.s.terminal and root.s.step % 6 == 0 and 6 - int(root.s.round_number) == R and len(decks) >= 1
    levels, cur = [], [W.root_on(root, deck) for deck in decks]
    for d in range(6 * R):
        p, n = d & 1, X.CARDS[d % 6]
        levels.append((p, n, [W.wide_key(st, p) for st in cur] if n >= 2 else None))
        nxt = []
        for st in cur:
            h = F.hand(st, p) if hand_order else sorted(F.hand(st, p))          # slot a: the a-th held card in ascending card id
            assert len(h) == n and (st.s.step & 1) == p
            nxt.extend(F.child(st, h[a]) for a in range(n))
        cur = nxt
    assert all(st.s.terminal for st in cur) and len(cur) == len(decks) * 36 ** R
    r = [st.s.r2[0] / 2.0 for st in cur]
    return levels, [r, [x * x for x in r], [float(st.s.scopas[0]) for st in cur], [float(st.s.scopas[1]) for st in cur]], len(decks)


def probs_of(levels, R, S, which):
    """step 2 for one store: per level the list of prob rows (None at a one-card ply)"""
    out = []
    for p, n, keys in levels:
        if keys is None:
            out.append(None)
            continue
        row = {k: F.average_probs(S, k, n) if which == 0 else F.sigma_of(R.get(k, [0.0] * 3), n) for k in set(keys)}
        out.append([row[k] for k in keys])
    return out


def mean_of(V, n_decks):
    """(0.0 + V[root 0] + V[root 1] + ...) / n, added in deck order"""
    assert len(V) == n_decks
    v = 0.0
    for x in V:
        v += x
    return v / n_decks


def value_of(levels, prob_a, prob_b, leaf, n_decks, swap_levels=False):
    """step 3 for one ordered pair and one quantity"""
    V = leaf
    for d in reversed(range(len(levels))):
        p, n, _ = levels[d]
        if n > 1:                             # (a one-card node takes its child's value: same index, same list)
            V = X.mix_up((prob_a if (p == 0) != swap_levels else prob_b)[d], V, n)
    return mean_of(V, n_decks)


def cross_play(tree, tables, which=0, swap_levels=False):
    """tables: K pairs (R, S) of {(A, B): [3]} regret and strategy rows -> float64 [K][K][4]"""
    levels, leaf4, n_decks = tree
    prob = [probs_of(levels, R, S, which) for R, S in tables]
    K = len(tables)
    out = np.zeros((K, K, 4))
    for a in range(K):
        for b in range(K):
            for q in range(4):
                out[a, b, q] = value_of(levels, prob[a], prob[b], leaf4[q], n_decks, swap_levels)
    return out


def pair_match(root, decks, S_a, S_b, n_episodes, seed, stream_id=0):
    """-> (sums [6] int64, r2 of a per episode): full_chance_ref.match with the opponent's rows S_b in uniform play's place"""
    sums, out = np.zeros(6, np.int64), np.zeros(n_episodes, np.int8)
    stream = stream_id & ((1 << 24) - 1)
    k = len(decks)
    for i in range(n_episodes):
        seat = 0 if 2 * i < n_episodes else 1
        st = W.root_on(root, decks[W.deck_of_episode(i, n_episodes, k)])
        while not st.s.terminal:
            p = st.s.step & 1
            h = sorted(F.hand(st, p))
            a = 0
            if len(h) > 1:
                prob = F.average_probs(S_a if p == seat else S_b, W.wide_key(st, p), len(h))
                a = F.pick(prob, O.philox_uniform(seed, i & 0xFFFFFFFF, i >> 32, (stream << 8) | int(st.s.step), W.MATCH_TAG))
            st.step(h[a])
        r2 = int(st.s.r2[seat])
        out[i] = r2
        sums[seat] += r2
        sums[2 + seat] += r2 * r2
        sums[4] += int(st.s.scopas[seat])
        sums[5] += int(st.s.scopas[1 - seat])
    return sums, out
