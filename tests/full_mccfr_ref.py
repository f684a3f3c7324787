"""CPU restatement of the FullScopa sampling solver (scopa_amd/csrc/scopa_full_mccfr.hip, include/scopa.h) on the oracle's FullScopa engine.

TEST INFRASTRUCTURE, written for this repository's tests: plain Python over oracle.FullState (pinned to 48 reference playouts by
tests/golden/full_scopa.json), cloning by copying the ctypes struct.  The reference has no solver that runs on FullScopa, so this file is the yardstick
of the device kernels, and tests/test_full_mccfr_ref.py holds it in turn to exact enumeration (unbiasedness) and to the shape counts of the header.

  key       the packing of scopa_full_infoset_key, restated from the oracle's state
  walk      textbook external sampling against frozen regrets: opponent nodes add sigma to d_strategy and sample ONE action from a draw named by the
            node (state.step << 16 | q, traversal id, iteration, 160 + traverser); traverser nodes take every action and add cfv - v to d_regret
  apply     regret += d_regret, strategy += d_strategy
  match     the seat-swapped match of the average policy against uniform play, draws at (episode, episode >> 32, stream << 8 | step, 176)"""
import ctypes as C

import numpy as np

import oracle as O

WALK_TAG, MATCH_TAG = 160, 176
SUITS = ("denari", "coppe", "spade", "bastoni")


def clone(st):
    c = O.FullState.__new__(O.FullState)
    c.s = type(st.s).from_buffer_copy(st.s)
    c.perm = st.perm
    return c


def child(st, a):
    c = clone(st)
    c.step(a)
    return c


def root_of(deck, actions=()):
    st = O.FullState(perm=np.ascontiguousarray(deck, np.uint8))
    for a in actions:
        assert a in st.legal()
        st.step(a)
    return st


def random_root(deck, rounds, rng):
    """(state, actions): uniformly random legal play for `rounds` whole rounds from the deal"""
    st, acts = root_of(deck), []
    for _ in range(6 * rounds):
        legal = st.legal()
        acts.append(int(legal[rng.randint(len(legal))]))
        st.step(acts[-1])
    return st, acts


def hand(st, p):
    return [int(st.s.hand[p][i]) for i in range(st.s.nh[p])]


def key_of(st, p):
    s, deck = st.s, st.perm
    r = int(s.round_number)
    held = set(hand(st, p))
    sub = sum(1 << i for i in range(3) if int(deck[4 + 6 * r + 3 * p + i]) in held)
    table = 0
    for i in range(s.nt):
        table |= 1 << int(s.table[i])
    return (1 << 63) | (p << 62) | (r << 59) | (sub << 56) | (table << 16) | (int(s.ncap[p]) << 10) | (int(s.scopas[0]) << 5) | int(s.scopas[1])


def key_actions(key):
    return bin((int(key) >> 56) & 7).count("1")


def key_to_string(key, deck):
    """information_state_string of the decision node a key stands for on `deck` (the opponent's capture count from the cards dealt so far)"""
    key = int(key)
    p, r, sub = (key >> 62) & 1, (key >> 59) & 7, (key >> 56) & 7
    h = [int(deck[4 + 6 * r + 3 * p + i]) for i in range(3) if (sub >> i) & 1]
    t = [c for c in range(40) if (key >> (16 + c)) & 1]
    own = (key >> 10) & 63
    other = 4 + 6 * (r + 1) - len(t) - len(h) - (len(h) - p) - own
    cap = (other, own) if p else (own, other)
    name = lambda cards: "-".join(f"{c % 10 + 1}{SUITS[c // 10][0]}" for c in sorted(cards, key=lambda c: (c % 10 + 1, SUITS[c // 10])))
    return f"P{p}:R{r}:H[{name(h)}]:T[{name(t)}]:C[{cap[0]},{cap[1]}]:S[{(key >> 5) & 31},{key & 31}]"


def sigma_of(R, n):
    """InfoNode.current_strategy (scopa_mccfr_sigma.h): np.maximum, a left-to-right sum, elementwise divide"""
    pos = [R[i] if R[i] > 0.0 else 0.0 for i in range(n)]
    s = pos[0]
    for i in range(1, n):
        s += pos[i]
    return [1.0 / n] * n if s == 0.0 else [x / s for x in pos]


def pick(prob, u):
    acc = 0.0
    for i, x in enumerate(prob):
        acc += x
        if acc > u:
            return i
    return len(prob) - 1


class Rows:
    """rows by key: R, S (the tables), dR, dS, count (the increments of the traversals since the last apply) and A, the sum of |increment| added into
    each regret cell (what the reorder budget of the GPU tests is measured in)"""

    def __init__(self):
        self.R, self.S, self.dR, self.dS, self.A, self.count = {}, {}, {}, {}, {}, {}
        self.choice = self.terminal = 0

    def touch(self, key):
        if key not in self.count:
            self.dR[key], self.dS[key], self.A[key], self.count[key] = [0.0] * 3, [0.0] * 3, [0.0] * 3, 0
            self.R.setdefault(key, [0.0] * 3)
            self.S.setdefault(key, [0.0] * 3)

    def plant(self, keys, regret, strategy):
        self.__init__()
        for k, r, s in zip(keys, regret, strategy):
            self.R[int(k)], self.S[int(k)] = [float(x) for x in r], [float(x) for x in s]

    def apply(self):
        for k in self.count:
            for a in range(3):
                self.R[k][a] += self.dR[k][a]
                self.S[k][a] += self.dS[k][a]
        self.dR, self.dS, self.A, self.count = {}, {}, {}, {}

    def arrays(self, what):
        """(keys ascending, [n][3] float64) of one of R, S, dR, dS, A, or (keys, counts) for `count`"""
        d = getattr(self, what)
        keys = sorted(d)
        return np.array(keys, np.uint64), (np.array([d[k] for k in keys], np.uint32 if what == "count" else np.float64).reshape((len(keys),) if what == "count" else (len(keys), 3)))


def walk(st, trav, tid, iteration, seed, rows, q=0, uniform=False):
    """one traversal below `st`: the value of `st` for the traverser; increments into rows.  uniform=True: sigma is uniform whatever the regrets"""
    s = st.s
    if s.terminal:
        rows.terminal += 1
        v = s.r2[0] / 2.0
        return -v if trav else v
    p = s.step & 1
    h = hand(st, p)
    n = len(h)
    if n == 1:
        return walk(child(st, h[0]), trav, tid, iteration, seed, rows, q, uniform)
    key = key_of(st, p)
    rows.choice += 1
    rows.touch(key)
    sigma = [1.0 / n] * n if uniform else sigma_of(rows.R[key], n)
    if p != trav:
        for a in range(n):
            rows.dS[key][a] += sigma[a]
        rows.count[key] += 1
        u = O.philox_uniform(seed, (int(s.step) << 16) | q, tid, iteration, WALK_TAG + trav)
        return walk(child(st, h[pick(sigma, u)]), trav, tid, iteration, seed, rows, q, uniform)
    cfv = [walk(child(st, h[a]), trav, tid, iteration, seed, rows, q * n + a, uniform) for a in range(n)]
    v = 0.0
    for a in range(n):
        v += sigma[a] * cfv[a]
    for a in range(n):
        inc = cfv[a] - v
        rows.dR[key][a] += inc
        rows.A[key][a] += abs(inc)
    rows.count[key] += 1
    return v


def traverse(root, trav, iteration, b0, nb, seed, rows):
    for i in range(nb):
        walk(root, trav, (b0 + i) & 0xFFFFFFFF, iteration, seed, rows)


def iterate(root, batch, seed, rows, counter):
    """one iteration from the handle's counter: traverse(0), apply, traverse(1), apply -> the counter after it"""
    for trav in range(2):
        traverse(root, trav, counter, 0, batch, seed, rows)
        rows.apply()
        counter += 1
    return counter


def shape_counts(r0):
    """(choice visits as traverser 0, as traverser 1, terminals) of one traversal from the start of round r0, by the header's formula"""
    S = (6 ** (6 - r0) - 1) // 5
    return 13 * S, 8 * S, 6 ** (6 - r0)


# ---- exact enumeration under uniform sigma (the check that the walk IS external sampling) -------------------------------------------------------
def exact_regret(root, trav):
    """{key: [3]} the counterfactual regret increment of every traverser infoset when every player plays uniformly: the sum over the infoset's
    histories of (the opponent's reach) x (value of action a - value of the node), which is the expectation of one traversal's d_regret row"""
    out = {}

    def rec(st, reach):
        s = st.s
        if s.terminal:
            v = s.r2[0] / 2.0
            return -v if trav else v
        p = s.step & 1
        h = hand(st, p)
        n = len(h)
        if n == 1:
            return rec(child(st, h[0]), reach)
        if p != trav:
            return sum(rec(child(st, c), reach / n) for c in h) / n
        cfv = [rec(child(st, c), reach) for c in h]
        v = sum(cfv) / n
        row = out.setdefault(key_of(st, p), [0.0] * 3)
        for a in range(n):
            row[a] += reach * (cfv[a] - v)
        return v

    rec(root, 1.0)
    return out


# ---- average policy and match -------------------------------------------------------------------------------------------------------------------
def average_probs(S, key, n):
    row = S.get(key)
    if row is not None:
        total = 0.0
        for a in range(n):
            total += row[a]
        if total > 1e-12:
            return [row[a] / total for a in range(n)]
    return [1.0 / n] * n


def match(root, S, n_episodes, seed, stream_id=0):
    """-> (sums [6] int64, r2 of the agent per episode): the agent plays average_probs of S, the opponent uniformly"""
    sums, out = np.zeros(6, np.int64), np.zeros(n_episodes, np.int8)
    for i in range(n_episodes):
        seat = 0 if 2 * i < n_episodes else 1
        st = clone(root)
        while not st.s.terminal:
            p = st.s.step & 1
            h = hand(st, p)
            a = 0
            if len(h) > 1:
                prob = average_probs(S, key_of(st, p), len(h)) if p == seat else [1.0 / len(h)] * len(h)
                a = pick(prob, O.philox_uniform(seed, i & 0xFFFFFFFF, i >> 32, (stream_id << 8) | int(st.s.step), MATCH_TAG))
            st.step(h[a])
        r2 = int(st.s.r2[seat])
        out[i] = r2
        sums[seat] += r2
        sums[2 + seat] += r2 * r2
        sums[4] += int(st.s.scopas[seat])
        sums[5] += int(st.s.scopas[1 - seat])
    return sums, out


def exact_match_value(root, S, seat):
    """the expected reward (not x2) of the agent in `seat` from the root: average_probs of S against uniform play, by enumeration"""
    def rec(st):
        if st.s.terminal:
            return st.s.r2[seat] / 2.0
        p = st.s.step & 1
        h = hand(st, p)
        if len(h) == 1:
            return rec(child(st, h[0]))
        prob = average_probs(S, key_of(st, p), len(h)) if p == seat else [1.0 / len(h)] * len(h)
        return sum(pr * rec(child(st, c)) for pr, c in zip(prob, h) if pr > 0.0)
    return rec(root)
