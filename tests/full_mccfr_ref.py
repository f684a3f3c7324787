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
        self.choice = self.terminal = self.dropped = 0

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


    def copy(self):
        """an independent copy: a reference computed once stays as it was when a test goes on from it"""
        c = Rows()
        for name in ("R", "S", "dR", "dS", "A"):
            setattr(c, name, {k: list(v) for k, v in getattr(self, name).items()})
        c.count = dict(self.count)
        c.choice, c.terminal, c.dropped = self.choice, self.terminal, self.dropped
        return c

    def touch_all(self, keys):
        """rows the store holds without a visit (planted and not met): zero increments and a zero count, as delta_get reports them"""
        for k in keys:
            self.touch(int(k))


def walk(st, trav, tid, iteration, seed, rows, q=0, uniform=False, absent=frozenset()):
    """one traversal below `st`: the value of `st` for the traverser; increments into rows.  uniform=True: sigma is uniform whatever the regrets.
    A key in `absent` is a row the store cannot take (64 other keys from its home on): the visit is counted in rows.choice and in rows.dropped, the
    row is not touched, reads as a zero regret row and receives no add"""
    s = st.s
    if s.terminal:
        rows.terminal += 1
        v = s.r2[0] / 2.0
        return -v if trav else v
    p = s.step & 1
    h = hand(st, p)
    n = len(h)
    if n == 1:
        return walk(child(st, h[0]), trav, tid, iteration, seed, rows, q, uniform, absent)
    key = key_of(st, p)
    rows.choice += 1
    held = key not in absent
    if held:
        rows.touch(key)
    else:
        rows.dropped += 1
    sigma = [1.0 / n] * n if uniform or not held else sigma_of(rows.R[key], n)
    if p != trav:
        if held:
            for a in range(n):
                rows.dS[key][a] += sigma[a]
            rows.count[key] += 1
        u = O.philox_uniform(seed, (int(s.step) << 16) | q, tid, iteration, WALK_TAG + trav)
        return walk(child(st, h[pick(sigma, u)]), trav, tid, iteration, seed, rows, q, uniform, absent)
    cfv = [walk(child(st, h[a]), trav, tid, iteration, seed, rows, q * n + a, uniform, absent) for a in range(n)]
    v = 0.0
    for a in range(n):
        v += sigma[a] * cfv[a]
    if held:
        for a in range(n):
            inc = cfv[a] - v
            rows.dR[key][a] += inc
            rows.A[key][a] += abs(inc)
        rows.count[key] += 1
    return v


def traverse(root, trav, iteration, b0, nb, seed, rows, absent=frozenset()):
    for i in range(nb):
        walk(root, trav, (b0 + i) & 0xFFFFFFFF, iteration, seed, rows, absent=absent)


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
def average_probs(S, key, n, threshold=1e-12):
    """threshold: the rule's 1e-12; a guard passes another to restate a wrong kernel"""
    row = S.get(key)
    if row is not None:
        total = 0.0
        for a in range(n):
            total += row[a]
        if total > threshold:
            return [row[a] / total for a in range(n)]
    return [1.0 / n] * n


def match(root, S, n_episodes, seed, stream_id=0, split=None):
    """-> (sums [6] int64, r2 of the agent per episode): the agent plays average_probs of S, the opponent uniformly.  split: the first episode of
    seat 1 where a guard wants the kernel's rule (2 i < n: seat 0) moved; None is the rule itself"""
    sums, out = np.zeros(6, np.int64), np.zeros(n_episodes, np.int8)
    for i in range(n_episodes):
        seat = (0 if 2 * i < n_episodes else 1) if split is None else (0 if i < split else 1)
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


def subgame_keys(root):
    """every key of the sub-game below a root at a round boundary, ascending (the choice levels of full_exploit_ref.tree_of: 36^R histories)"""
    import full_exploit_ref as X              # (it imports this module)
    levels, _ = X.tree_of(root, 6 - int(root.s.round_number))
    return np.array(sorted({int(k) for _, n, ks in levels if n > 1 for k in ks}), np.uint64)


def edge_rows(keys, name):
    """(keys ascending, n_act, regret [n][3], strategy [n][3] of zeros): the project's edge table `name` (oracle/mccfr_edges.py) over `keys`, the
    position of a key in ascending order as the table's row index, the first three of its four slots"""
    import mccfr_edges as E
    keys = np.sort(np.asarray(keys, np.uint64))
    n_act = np.array([key_actions(k) for k in keys], np.int32)
    R = np.ascontiguousarray(E.edge_table(name, n_act)[:, :3])
    return keys, n_act, R, np.zeros_like(R)


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


# ---- the store: the probe sequence restated, and keys built to land where a test wants them -----------------------------------------------------------
# scopa_full_store.h (fm_hash, fm_find, fm_claim): the home of a key is fm_hash(key) & (2^capacity_log2 - 1), fm_hash = splitmix64's finaliser folded
# to 32 bits; a probe looks at the home and the slots after it (wrapping), MAX_PROBE of them at the most.  A change of the hash or of the limit there
# changes this block too.
MAX_PROBE = 64
FILLER_BASE = (1 << 63) | (7 << 59) | (0b111 << 56)         # round field 7: passes tables_set's validation (marker bit, 3 hand bits), never met by play


def fm_hash(keys):
    """fm_hash of a numpy uint64 array, in 64-bit wrap-around arithmetic -> uint64 array holding the 32-bit hash"""
    k = np.array(keys, np.uint64, ndmin=1)
    k ^= k >> np.uint64(30)
    k *= np.uint64(0xBF58476D1CE4E5B9)
    k ^= k >> np.uint64(27)
    k *= np.uint64(0x94D049BB133111EB)
    k ^= k >> np.uint64(31)
    return (k ^ (k >> np.uint64(32))) & np.uint64(0xFFFFFFFF)


def home_slot(key, capacity_log2):
    """the slot a probe for `key` starts at: int for one key, int64 array for an array of keys"""
    h = (fm_hash(key) & np.uint64((1 << capacity_log2) - 1)).astype(np.int64)
    return int(h[0]) if np.ndim(key) == 0 else h


def fillers(home, n, capacity_log2, tag=0):
    """n distinct keys FILLER_BASE | c << 16 whose home is `home`: the first n counters c at or above tag << 32 (tag < 256: c stays in the 40 table bits)"""
    assert 0 <= tag < 256 and 0 <= home < (1 << capacity_log2)
    out, c, chunk = [], tag << 32, 1 << 22
    while len(out) < n:
        assert c + chunk <= 1 << 40
        keys = np.uint64(FILLER_BASE) | (np.arange(c, c + chunk, dtype=np.uint64) << np.uint64(16))
        out.extend(keys[home_slot(keys, capacity_log2) == home][:n - len(out)].tolist())
        c += chunk
    return np.array(out, np.uint64)


def rows_for(keys):
    """(regret, strategy) [n][3] as a fixed function of the key: cell a of the regret row is byte a of the key's table field + 1 + a / 4, the strategy
    row twice that + 1/8; cells beyond the key's action count are 0.0 (the store does not keep them).  No legal cell is zero, so a row that comes back
    under another key, or not at all, shows up"""
    keys = np.asarray(keys, np.uint64).reshape(-1)
    a = np.arange(3, dtype=np.uint64)
    R = ((keys[:, None] >> (np.uint64(16) + np.uint64(8) * a[None, :])) & np.uint64(0xFF)).astype(np.float64) + 1.0 + np.arange(3) / 4.0
    legal = np.arange(3)[None, :] < np.array([key_actions(k) for k in keys]).reshape(-1, 1)
    R = np.where(legal, R, 0.0)
    return R, np.where(legal, 2.0 * R + 0.125, 0.0)


class Store:
    """Sequential model of the store with an UNBOUNDED linear probe: slots (slot -> key), probe (key -> slots looked at by its insertion, its own included).

    The occupied SET of linear probing does not depend on the insertion order; the length of one key's probe does (40 keys of home h and then 40 of home
    h + 20 look at 60 slots at the most, the other way round at 80).  What holds in every order: a probe for a key never looks past the first free slot
    after its home in the FINAL occupied set, because everything occupied on the way is occupied in the end.  reach(key) is that count of slots, home and
    free slot's predecessor included; while reach(key) <= MAX_PROBE for every key, the device holds every key whatever the arrival order."""

    def __init__(self, capacity_log2):
        self.c, self.mask, self.slots, self.probe = capacity_log2, (1 << capacity_log2) - 1, {}, {}

    def insert(self, keys):
        keys = np.asarray(keys, np.uint64).reshape(-1)
        for k, i in zip(keys.tolist(), home_slot(keys, self.c).tolist()):
            assert k not in self.probe and len(self.slots) <= self.mask
            n = 1
            while i in self.slots:
                i, n = (i + 1) & self.mask, n + 1
            self.slots[i], self.probe[k] = k, n
        return self

    def longest_probe(self):
        return max(self.probe.values())

    def reach(self, key):
        """slots from the home of `key` up to (not including) the first free one in the occupied set as it stands; capacity if the store is full"""
        i, n = home_slot(np.uint64(key), self.c), 0
        while i in self.slots and n <= self.mask:
            i, n = (i + 1) & self.mask, n + 1
        return n

    def longest_reach(self):
        return max(self.reach(k) for k in self.probe)


def isolated(key, others, capacity_log2):
    """no key of `others` (but `key` itself) has its home in [h - 64, h + 128) mod capacity, h the home of `key`: 64 keys of home h then fill exactly
    h .. h + 63 and every other key probes as it would without them"""
    others = np.array([k for k in others if int(k) != int(key)], np.uint64)
    if not others.size:
        return True
    d = (home_slot(others, capacity_log2) - home_slot(np.uint64(key), capacity_log2) + 64) & ((1 << capacity_log2) - 1)
    return not bool((d < 192).any())
