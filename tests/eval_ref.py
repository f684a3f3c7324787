"""Plain CPU restatement of the net-policy evaluator (scopa_amd/csrc/scopa_sdcfr.hip: k_eval_step, scopa_features_from_states,
scopa_eval_init_states) over the oracle's list-based State, episode by episode.

TEST INFRASTRUCTURE, written for this repository's tests: the GPU kernels are held to it exactly (integer states field for field, float32 features
as bits).  It uses numpy, oracle.State and the oracle's Philox4x32-10, and nothing of the product.

One ply of one episode i (evaluate_vs_random, deep_cfr.py:385-408):
  draw      u = u53(x0, x1) of Philox counter (i, i >> 32, ply_tag, stream_id) under key (seed low, seed high);
            u53 = ((x0 >> 5) * 2^26 + (x1 >> 6)) / 2^53
  weights   the mover is the trained seat and probs are given: float64(float32 probs[i][card]) of the mover's hand, in hand order; otherwise all 1
  fallback  the reference's (:394-397): ANY NaN among the legal slots, or a total that is not > 0, gives uniform.  A negative entry is outside the
            reference's domain (np.random.choice raises on it); it is clamped to 0 before the sum, as the kernel does.  +-inf is not a valid input.
  action    the first q with u < c_q, c_q the running float64 sum of w_q / tot in hand order (0.0 + w_0 / tot, + w_1 / tot, ...); the last one if none
Every float64 operation is one Python float operation (one rounding): the total is summed from 0.0 in hand order, each term is a division followed
by an add -- a division cannot be contracted with the add after it, so the device computes the same bits.
Terminal states -- cloned ones, whose step limit is 16, included -- are left alone.
"""
import ctypes as C
import math
import struct

import numpy as np

import oracle as O

# scopa_state, 16 bytes (include/scopa.h), restated: ordered hands and table as nibble lists, unused nibbles zero
STATE_DTYPE = np.dtype([("hand", "<u2", (2,)), ("table", "<u4"), ("nh", "u1", (2,)), ("nt", "u1"), ("step", "u1"),
                        ("ncap", "u1", (2,)), ("scopas", "u1", (2,))])
STEP_CLONED = 0x80
TWO53 = 9007199254740992.0


def root_state(perm):
    """The root of the deal `perm` (MiniScopaGame.reset: cards 0-3 to seat 0, 4-7 to seat 1, empty table)."""
    return O.State(perm=np.ascontiguousarray(perm, np.uint8))


def pack(state):
    """oracle.State -> one STATE_DTYPE record (a cloned env's step limit of 16 is the bit SCOPA_STEP_CLONED of `step`)."""
    return np.frombuffer(_pack_bytes(state), STATE_DTYPE)[0]


def _pack_bytes(state):
    s = state.s
    hand = [sum(int(s.hand[p][i]) << (4 * i) for i in range(s.nh[p])) for p in (0, 1)]
    table = sum(int(s.table[i]) << (4 * i) for i in range(s.nt))
    step = int(s.step) | (STEP_CLONED if int(s.max_steps) == 16 else 0)
    return struct.pack("<HHI8B", hand[0], hand[1], table, s.nh[0], s.nh[1], s.nt, step, s.ncap[0], s.ncap[1], s.scopas[0], s.scopas[1])


def pack_all(states):
    return np.frombuffer(b"".join(_pack_bytes(s) for s in states), STATE_DTYPE)


def features(state):
    """(feat float32 [34], mask float32 [16]) for the player to move: hand one-hot by card id, table multi-hot at 16.., slot 32 = 1, slot 33 = 0;
    the mask is the hand.  A terminal state (empty hand) gives a zero hand and mask."""
    s = state.s
    p = int(s.step) & 1
    f, m = np.zeros(34, np.float32), np.zeros(16, np.float32)
    for i in range(s.nh[p]):
        f[int(s.hand[p][i])] = m[int(s.hand[p][i])] = 1.0
    for i in range(s.nt):
        f[16 + int(s.table[i])] = 1.0
    f[32] = 1.0
    return f, m


def u53(x0, x1):
    return ((int(x0) >> 5) * 67108864.0 + (int(x1) >> 6)) / TWO53


_ctr, _key, _out = (C.c_uint32 * 4)(), (C.c_uint32 * 2)(), (C.c_uint32 * 4)()


def draw(i, ply_tag, stream_id, seed):
    """oracle.philox4x32_10([i, i >> 32, ply_tag, stream_id], [seed low, seed high]) -> u53 of its first two words (the same C function, called
    with preallocated buffers)."""
    _ctr[0], _ctr[1], _ctr[2], _ctr[3] = i & 0xFFFFFFFF, (i >> 32) & 0xFFFFFFFF, ply_tag & 0xFFFFFFFF, stream_id & 0xFFFFFFFF
    _key[0], _key[1] = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    O.lib().og_philox4x32_10(_ctr, _key, _out)
    return u53(_out[0], _out[1])


def action_weights(row, hand):
    """(w, tot): row = float32 [16] policy of the trained seat or None (uniform play), hand = the mover's cards in hand order."""
    n = len(hand)
    if row is None:
        return [1.0] * n, float(n)
    v = [float(np.float32(row[c])) for c in hand]
    w = [x if x > 0.0 else 0.0 for x in v]          # NaN and negative entries -> 0
    tot = 0.0
    for x in w:
        tot = tot + x
    if any(math.isnan(x) for x in v) or not tot > 0.0:   # deep_cfr.py:394-395
        return [1.0] * n, float(n)
    return w, tot


def pick(w, tot, u):
    c = 0.0
    for q, x in enumerate(w):
        c = c + x / tot
        if u < c:
            return q
    return len(w) - 1


def eval_step(states, probs, trained_seat, seed, stream_id, ply_tag):
    """One ply of every episode, in place on the list of oracle.State.  probs: float32 [n][16] or None; trained_seat: [n] ints.
    -> the chosen hand position of every episode (-1 where the state was terminal and left alone)."""
    chosen = []
    for i, st in enumerate(states):
        if st.is_terminal():
            chosen.append(-1)
            continue
        s = st.s
        p = int(s.step) & 1
        hand = [int(s.hand[p][q]) for q in range(s.nh[p])]
        u = draw(i, ply_tag, stream_id, seed)
        w, tot = action_weights(probs[i] if (probs is not None and p == int(trained_seat[i])) else None, hand)
        k = pick(w, tot, u)
        st.step(hand[k])
        chosen.append(k)
    return chosen


def match_numbers(final_states, seat):
    """What DeepCFR.evaluate_vs_random returns and stores, from the final packed states (STATE_DTYPE [n]) and the trained seat of every episode:
    (average reward of the trained seat by evaluate_game's rule (mini_scopa_game.py:106-114: r = captures + 2 scopas, reward = r - total / 2,
    0 when the total is 0), [mean scopas of the trained seat, of the random seat], the two halves by seat)."""
    seat = np.asarray(seat, np.int64)
    n = seat.size
    own_r, own_s, opp_s = np.zeros(n), np.zeros(n), np.zeros(n)
    for i in range(n):
        r = [int(final_states["ncap"][i][p]) + 2 * int(final_states["scopas"][i][p]) for p in (0, 1)]
        total = r[0] + r[1]
        own_r[i] = 0.0 if total == 0 else r[seat[i]] - total / 2.0
        own_s[i] = float(final_states["scopas"][i][seat[i]])
        opp_s[i] = float(final_states["scopas"][i][1 - seat[i]])
    halves = []
    for s in (0, 1):
        k = seat == s
        m = int(k.sum())
        halves.append({"episodes": m, "reward": float(own_r[k].mean()) if m else 0.0,
                       "reward_std_error": float(own_r[k].std() / np.sqrt(m)) if m else 0.0,
                       "trained_scopas": float(own_s[k].mean()) if m else 0.0, "opponent_scopas": float(opp_s[k].mean()) if m else 0.0})
    return float(own_r.mean()), [float(own_s.mean()), float(opp_s.mean())], halves
