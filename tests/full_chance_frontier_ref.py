"""CPU restatement of the frontier form of Deep CFR's traversal on FullScopa over decks (scopa_full_chance_sdcfr_traverse_frontier in include/scopa.h;
scopa_amd/csrc/scopa_full_chance_sdcfr.hip): one traversal played on REAL states level by level with the Python rules of the FullScopa restatements
(full_mccfr_ref, full_chance_ref), no forest.

TEST INFRASTRUCTURE, written from the definitions.  A node is (choice level k, path p), p the mixed-radix number of the traverser's own slot choices so
far; the traverser's levels send slot a to path p n_k + a, the other player's draw one slot -- Philox at counter (k << 24 | p, traversal id, iteration,
240 + traverser) -- and keep p; the two one-card plies behind a round's last choice level are played through.  The policy is asked of
`policy_fn(keys2 [n][2] uint64, player) -> (policy [n][3] float32, thresholds [n][2] uint64)` ONCE per level, so with the device's own policy call in
that place no draw is ambiguous and rows, values and positions are compared on bits.  The float32 arithmetic of a row (row_of, regret_row), the slot
rule (action_of), the features and the ring position are tests/full_chance_sdcfr_ref.py's, imported unchanged."""
import numpy as np

import full_chance_ref as W
import full_chance_sdcfr_ref as S
import full_mccfr_ref as F
import sdcfr_policy_ref as P

from full_chance_sdcfr_ref import CARDS, action_of, features, regret_row, ring_row, row_of, rows_per_traversal, visits_per_traversal   # noqa: F401

PHILOX_TAG = 240


def draw_N(level, path, trav_id, iteration, traverser, seed):
    o = P.philox4x32_10(np.uint64((level << 24) | int(path)), np.uint64(trav_id & 0xFFFFFFFF), np.uint64(iteration), np.uint64(PHILOX_TAG + traverser), int(seed))
    return (int(o[0]) >> 5 << 26) | (int(o[1]) >> 6)


def held(keys2):
    """the held cards of key pairs [n][2]: popcount of word B"""
    return np.array([bin(int(b)).count("1") for b in np.asarray(keys2, np.uint64).reshape(-1, 2)[:, 1]], np.int32)


def host_policy_fn(nets, exact=False):
    """policy_fn from two nets on the host: the float64 forward pass rounded to float32 (bit-exact on exact-arithmetic nets with exact=True)"""
    def fn(keys2, player):
        n_act = held(keys2)
        pol = S.node_policy(nets[player], keys2, n_act, exact)[0].astype(np.float32)
        return pol, S.thresholds_all(pol, n_act)
    return fn


def _after(st, card, k):
    """the state behind choice level k after `card`: one step, and at a round's last choice level the two one-card plies too"""
    c = F.child(st, card)
    if (k & 3) == 3:
        for p in (0, 1):
            last = F.hand(c, p)
            assert len(last) == 1 and (int(c.s.step) & 1) == p
            c.step(last[0])
    return c


def walk_frontier(root_state, deck, traverser, trav_id, iteration, seed, policy_fn):
    """One traversal of `traverser` on `deck` below the round-boundary root `root_state`
    -> dict(rows={rank: (key pair (A, B), regret [40] float32)}, value float32, visits, path={(level, path): slot drawn}, R)"""
    st0 = W.root_on(root_state, deck)
    R = 6 - int(st0.s.round_number)
    L = 4 * R
    states, kept, path, visits = [st0], {}, {}, 0
    for k in range(L):
        p, n = k & 1, CARDS[k & 3]
        keys = np.array([W.wide_key(st, p) for st in states], np.uint64).reshape(-1, 2)
        assert (held(keys) == n).all() and all((int(st.s.step) & 1) == p and not st.s.terminal for st in states)
        pol, thr = policy_fn(keys, p)
        visits += len(states)
        nxt = []
        if p == traverser:
            kept[k] = (keys, np.asarray(pol, np.float32))
            for st in states:
                cards = sorted(F.hand(st, p))
                nxt.extend(_after(st, cards[a], k) for a in range(n))
        else:
            for q, st in enumerate(states):
                a = action_of(thr[q], draw_N(k, q, trav_id, iteration, traverser, seed), n)
                path[(k, q)] = a
                nxt.append(_after(st, sorted(F.hand(st, p))[a], k))
        states = nxt
    assert len(states) == 6 ** R and all(st.s.terminal for st in states)
    val = [np.float32(st.s.r2[0] / 2.0) if traverser == 0 else np.float32(-(st.s.r2[0] / 2.0)) for st in states]
    rank0, r = {}, 0
    for k in sorted(kept):
        rank0[k] = r
        r += len(kept[k][0])
    assert r == rows_per_traversal(R)
    rows = {}
    for k in sorted(kept, reverse=True):
        n = CARDS[k & 3]
        keys, pol = kept[k]
        up = []
        for f in range(len(keys)):
            v, ri, d = row_of(pol[f], val[f * n:f * n + n], n)
            rows[rank0[k] + f] = ((int(keys[f, 0]), int(keys[f, 1])), regret_row(keys[f, 1], ri, d))
            up.append(v)
        val = up
    assert len(val) == 1
    return dict(rows=rows, value=val[0], visits=visits, path=path, R=R)
