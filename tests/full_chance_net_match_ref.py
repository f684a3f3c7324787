"""CPU restatement of the match of the Deep CFR nets' average policy on FullScopa over decks (scopa_full_chance_sdcfr_match and
scopa_full_chance_sdcfr_average_at in include/scopa.h; scopa_amd/csrc/scopa_full_chance_sdcfr.hip): the episodes of full_chance_ref.match played
LEVEL BY LEVEL on real states with the Python rules of the FullScopa restatements, the policy asked ONCE per level and side.

TEST INFRASTRUCTURE, written from the definitions.  Episode i sits in seat 0 where 2 i < n and plays deck j % k (full_chance_ref.deck_of_episode); at
choice level k of the root's 4 R (mover k & 1, holding 3, 3, 2, 2 cards in a round) the episodes whose mover is the agent -- those of seat k & 1 --
hand their key pairs to `agent_fn(keys2 [m][2] uint64, player) -> rows [m][3] float64`; a row is played under the match's rule (probs_of: the sum of
its first n entries > 1e-12: row / sum, else uniform).  The opponent is None (uniform play), ("store", {pair: strategy row}) read as
full_mccfr_ref.average_probs reads it, or ("nets", fn) asked on the other episodes.  The draw is full_chance_ref.match's -- Philox at counter
(i, i >> 32, stream_id << 8 | state.step, 208) under the seed -- and the pick full_mccfr_ref.pick; the two one-card plies behind a round's last
choice level are played through.  With the device's own average_at in agent_fn's place no draw is ambiguous and sums, rewards and the trace are
compared on bits; host_rows_fn computes the rows in float64 (bit-exact in float32 on exact-arithmetic nets with one snapshot of coefficient 1).
Variants for the separation guard: seed_bits and stream_bits cut the seed and the stream id before they reach the Philox words."""
import numpy as np

import oracle as O
import full_chance_ref as W
import full_chance_sdcfr_ref as S
import full_mccfr_ref as F

from full_chance_sdcfr_ref import CARDS

LEVELS = 24                                # choice levels of the whole game: 4 a round


def held(keys2):
    """the held cards of key pairs [n][2]: popcount of word B, at most 3"""
    return np.array([min(bin(int(b)).count("1"), 3) for b in np.asarray(keys2, np.uint64).reshape(-1, 2)[:, 1]], np.int32)


def average_rows(snapshots, coefs, keys2, exact=False):
    """average_at's rows [n][3] float64 on the host: the FIFO average of full_chance_sdcfr_ref in float64; exact=True (exact-arithmetic nets, dyadic
    coefficients) restates the float32 accumulate bit for bit: acc = float32(acc + float32(coef * p)), then the float64 normalisation"""
    keys2 = np.asarray(keys2, np.uint64).reshape(-1, 2)
    n_act = held(keys2)
    if not exact:
        return S.average_policy(snapshots, coefs, keys2, n_act)[0]
    acc = np.zeros((len(keys2), 3), np.float32)
    for net, c in zip(snapshots, coefs):
        p = S.node_policy(net, keys2, n_act, exact=True)[0].astype(np.float32)
        acc = (acc + (np.float32(c) * p).astype(np.float32)).astype(np.float32)
    a = acc.astype(np.float64)
    live = np.arange(3)[None, :] < n_act[:, None]
    a = a * live
    s = (a[:, 0] + a[:, 1]) + a[:, 2]
    ok = (s > 0) & np.isfinite(s)
    return np.where(ok[:, None], a / np.where(ok, s, 1.0)[:, None], live / n_act[:, None].astype(np.float64)) * live


def host_rows_fn(sets, exact=False):
    """agent_fn from two snapshot sets [(snapshots, coefs) of player 0, of player 1]"""
    def fn(keys2, player):
        return average_rows(sets[player][0], sets[player][1], keys2, exact)
    return fn


def probs_of(row, n, threshold=1e-12):
    """the match's rule on a policy row: the sum of the first n entries, left to right from 0.0"""
    total = 0.0
    for a in range(n):
        total += float(row[a])
    if total > threshold:
        return [float(row[a]) / total for a in range(n)]
    return [1.0 / n] * n


def draw(seed, i, stream_id, step, seed_bits=64, stream_bits=24):
    seed = int(seed) & ((1 << seed_bits) - 1)
    stream = int(stream_id) & ((1 << stream_bits) - 1)
    return O.philox_uniform(seed, i & 0xFFFFFFFF, i >> 32, (stream << 8) | int(step), W.MATCH_TAG)


def _finish(st, seat, i, sums, out):
    r2 = int(st.s.r2[seat])
    out[i] = r2
    sums[seat] += r2
    sums[2 + seat] += r2 * r2
    sums[4] += int(st.s.scopas[seat])
    sums[5] += int(st.s.scopas[1 - seat])


def match_levels(root, decks, n_episodes, seed, agent_fn, opponent=None, stream_id=0, **cut):
    """-> (sums [6] int64, r2 of the agent per episode int8 [n], trace int8 [n][24]: the slot chosen at each choice level of the WHOLE game, -1 above
    the root), level by level"""
    n, k = int(n_episodes), len(decks)
    R = 6 - int(root.s.round_number)
    level0 = 4 * int(root.s.round_number)
    seats = [0 if 2 * i < n else 1 for i in range(n)]
    states = [W.root_on(root, decks[W.deck_of_episode(i, n, k)]) for i in range(n)]
    trace = np.full((n, LEVELS), -1, np.int8)
    for lv in range(4 * R):
        p, nl = lv & 1, CARDS[lv & 3]
        keys = np.array([W.wide_key(st, p) for st in states], np.uint64).reshape(-1, 2)
        assert all((int(st.s.step) & 1) == p and not st.s.terminal and len(F.hand(st, p)) == nl for st in states)
        mine = [i for i in range(n) if seats[i] == p]
        theirs = [i for i in range(n) if seats[i] != p]
        rows = {}
        if mine:
            rows.update(zip(mine, np.asarray(agent_fn(keys[mine], p), np.float64)))
        if theirs and opponent is not None and opponent[0] == "nets":
            rows.update(zip(theirs, np.asarray(opponent[1](keys[theirs], p), np.float64)))
        for i, st in enumerate(states):
            if i in rows:
                prob = probs_of(rows[i], nl)
            elif opponent is not None and opponent[0] == "store":
                prob = F.average_probs(opponent[1], (int(keys[i, 0]), int(keys[i, 1])), nl)
            else:
                prob = [1.0 / nl] * nl
            a = F.pick(prob, draw(seed, i, stream_id, st.s.step, **cut))
            trace[i, level0 + lv] = a
            st.step(sorted(F.hand(st, p))[a])
            if (lv & 3) == 3:
                for q in (0, 1):
                    last = F.hand(st, q)
                    assert len(last) == 1 and (int(st.s.step) & 1) == q
                    st.step(last[0])
    sums, out = np.zeros(6, np.int64), np.zeros(n, np.int8)
    for i, st in enumerate(states):
        assert st.s.terminal
        _finish(st, seats[i], i, sums, out)
    return sums, out, trace


def episode(root, decks, i, n_episodes, seed, agent_fn, opponent=None, stream_id=0, **cut):
    """episode i alone, depth first, the policy asked one node at a time -> (r2 of the agent, scopas of the agent, of the opponent, trace [24])"""
    n, k = int(n_episodes), len(decks)
    seat = 0 if 2 * i < n else 1
    st = W.root_on(root, decks[W.deck_of_episode(i, n, k)])
    trace, lv = np.full(LEVELS, -1, np.int8), 4 * int(root.s.round_number)
    while not st.s.terminal:
        p = int(st.s.step) & 1
        h = sorted(F.hand(st, p))
        a = 0
        if len(h) > 1:
            key = W.wide_key(st, p)
            if p == seat:
                prob = probs_of(np.asarray(agent_fn(np.array([key], np.uint64), p), np.float64)[0], len(h))
            elif opponent is not None and opponent[0] == "nets":
                prob = probs_of(np.asarray(opponent[1](np.array([key], np.uint64), p), np.float64)[0], len(h))
            elif opponent is not None:
                prob = F.average_probs(opponent[1], key, len(h))
            else:
                prob = [1.0 / len(h)] * len(h)
            a = F.pick(prob, draw(seed, i, stream_id, st.s.step, **cut))
            trace[lv] = a
            lv += 1
        st.step(h[a])
    return int(st.s.r2[seat]), int(st.s.scopas[seat]), int(st.s.scopas[1 - seat]), trace


def replay(root, decks, n_episodes, trace):
    """the traced slots played on host states -> (sums, r2, the key pair and Philox step of every traced choice: a list per episode of
    (level, player, (A, B), state.step)); every traced slot must be legal"""
    n, k = int(n_episodes), len(decks)
    level0 = 4 * int(root.s.round_number)
    sums, out, seen = np.zeros(6, np.int64), np.zeros(n, np.int8), []
    for i in range(n):
        seat = 0 if 2 * i < n else 1
        st = W.root_on(root, decks[W.deck_of_episode(i, n, k)])
        assert (trace[i, :level0] == -1).all()
        lv, met = level0, []
        while not st.s.terminal:
            p = int(st.s.step) & 1
            h = sorted(F.hand(st, p))
            a = 0
            if len(h) > 1:
                a = int(trace[i, lv])
                assert 0 <= a < len(h), (i, lv, a)
                met.append((lv, p, W.wide_key(st, p), int(st.s.step)))
                lv += 1
            st.step(h[a])
        assert lv == LEVELS
        seen.append(met)
        _finish(st, seat, i, sums, out)
    return sums, out, seen
