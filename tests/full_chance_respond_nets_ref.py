"""CPU restatement of the sampled best response to the Deep CFR nets on FullScopa over decks (scopa_full_chance_respond_nets_traverse / _iterate in
include/scopa.h; k_frn_claim, k_frn_expand, k_frn_step, k_frn_up in scopa_amd/csrc/scopa_full_chance_sdcfr.hip): the response traversals of
full_chance_respond_ref played LEVEL BY LEVEL on real states with the Python rules of the FullScopa restatements, all traversals of a call together,
as the device plays a chunk.

TEST INFRASTRUCTURE, written from the definitions.  A node is (traversal, choice level k, path p), p the mixed-radix number of the responder's own slot
choices so far -- full_chance_respond_ref.walk's q.  At the responder's levels every slot is expanded (slot a to path p n + a) and the row is touched in
`rows` (a full_chance_ref.Rows), sigma from its frozen regrets; at the other player's levels the opponent is asked ONCE per level,
`probs_at(keys2 [n][2] uint64, player) -> float64 [n][3]`, a row is played under the match's rule (full_chance_net_match_ref.probs_of), the draw is
full_chance_respond_ref's -- Philox at (state.step << 16 | p, b0 + i, iteration, deck_index << 8 | 144 + responder) -- and the path stays; the two
one-card plies behind a round's last choice level are played through.  On the way up v = sum of sigma[a] cfv[a] in slot order from 0.0, and the
increments cfv[a] - v go into the rows in the ORDER of the depth-first walk (a node after its sub-trees, the traversals one after the other), so with
an opponent that both restatements read alike the rows agree with full_chance_respond_ref.traverse on bits.  With the device's own average_at in
probs_at's place no draw is ambiguous.
Variant for the guards: tag= puts another tag base in 144's place."""
import numpy as np

import oracle as O
import full_chance_net_match_ref as M
import full_chance_ref as X
import full_chance_respond_ref as Q
import full_mccfr_ref as F

from full_chance_frontier_ref import _after
from full_chance_sdcfr_ref import CARDS

RESPOND_TAG = Q.RESPOND_TAG


def rows_probs_at(opp):
    """probs_at that reads a planted Rows (or {pair: strategy row}) as the store route's opponent is read: F.average_probs of its S, handed over as
    the row (the match's rule then divides a row whose total is 1 up to rounding: the probabilities move by an ulp at most, and a pick only where a
    draw falls into such a gap)"""
    S = getattr(opp, "S", opp)

    def fn(keys2, player):
        out = np.zeros((len(keys2), 3), np.float64)
        for i, k in enumerate(np.asarray(keys2, np.uint64).reshape(-1, 2).tolist()):
            n = X.key_actions(k)
            out[i, :n] = F.average_probs(S, tuple(k), n)
        return out
    return fn


def uniform_probs_at(keys2, player):
    """no snapshots: zero rows, which the match's rule plays uniformly"""
    return np.zeros((len(keys2), 3), np.float64)


def traverse(root, decks, resp, iteration, b0, nb, seed, rows, probs_at, listed=None, tag=RESPOND_TAG):
    """nb response traversals of `resp` on each listed deck (None: all), deck-major as the launch numbers them, level by level -> the root values
    [m * nb] float64"""
    listed = list(range(len(decks))) if listed is None else [int(d) for d in listed]
    travs = [(d, i) for d in listed for i in range(nb)]
    if not travs:
        return np.zeros(0)
    st0 = X.root_on(root, decks[0])
    L = 4 * (6 - int(st0.s.round_number))
    states = [[X.root_on(root, decks[d])] for d, _ in travs]              # per traversal, the level's nodes by path
    kept = [[] for _ in travs]                                            # per traversal, per responder level: (keys, sigma rows)
    for k in range(L):
        p, n = k & 1, CARDS[k & 3]
        keys = [[X.wide_key(st, p) for st in level] for level in states]
        assert all((int(st.s.step) & 1) == p and not st.s.terminal and len(F.hand(st, p)) == n for level in states for st in level)
        rows.choice += sum(len(level) for level in states)
        if p == resp:
            for t, level in enumerate(states):
                sig = []
                for key in keys[t]:
                    rows.touch(key)
                    sig.append(F.sigma_of(rows.R[key], n))
                kept[t].append((keys[t], sig, n))
                states[t] = [_after(st, sorted(F.hand(st, p))[a], k) for st in level for a in range(n)]
        else:
            flat = np.array([key for level in keys for key in level], np.uint64).reshape(-1, 2)
            pol = np.asarray(probs_at(flat, p), np.float64).reshape(-1, 3)
            at = 0
            for t, level in enumerate(states):
                d, i = travs[t]
                nxt = []
                for q, st in enumerate(level):
                    u = O.philox_uniform(seed, (int(st.s.step) << 16) | q, (b0 + i) & 0xFFFFFFFF, iteration, (d << 8) | (tag + resp))
                    a = F.pick(M.probs_of(pol[at], n), u)
                    at += 1
                    nxt.append(_after(st, sorted(F.hand(st, p))[a], k))
                states[t] = nxt
            assert at == len(pol)
    out = np.zeros(len(travs))
    for t, level in enumerate(states):
        assert all(st.s.terminal for st in level)
        rows.terminal += len(level)
        val = [-(st.s.r2[0] / 2.0) if resp else st.s.r2[0] / 2.0 for st in level]
        incs = []                                                         # per responder level, per path: the increments
        for keys_t, sig, n in reversed(kept[t]):
            up, inc = [], []
            for f in range(len(keys_t)):
                cfv = val[f * n:f * n + n]
                v = 0.0
                for a in range(n):
                    v += sig[f][a] * cfv[a]
                inc.append([cfv[a] - v for a in range(n)])
                up.append(v)
            incs.append(inc)
            val = up
        incs.reverse()
        assert len(val) == 1
        out[t] = val[0]

        def emit(j, f):                                                   # the adds in the depth-first walk's order: a node after its sub-trees
            keys_t, _, n = kept[t][j]
            if j + 1 < len(kept[t]):
                for a in range(n):
                    emit(j + 1, f * n + a)
            key = keys_t[f]
            for a in range(n):
                rows.dR[key][a] += incs[j][f][a]
                rows.A[key][a] += abs(incs[j][f][a])
            rows.count[key] += 1
        emit(0, 0)
    return out


def iterate(root, decks, batch, seed, rows, counter, probs_at, listed=None):
    """one iteration from the handle's counter: responder 0, apply, responder 1, apply over `listed` -> the counter after it"""
    for resp in range(2):
        traverse(root, decks, resp, counter, 0, batch, seed, rows, probs_at, listed)
        rows.apply()
        counter += 1
    return counter
