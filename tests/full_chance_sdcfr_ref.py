"""CPU restatement of Deep CFR on FullScopa over a set of decks (scopa_amd/csrc/scopa_full_chance_sdcfr.hip; the contract is the
scopa_full_chance_sdcfr_* block of include/scopa.h): the 96 features of a key pair, the 96-128-64-40 advantage net in float64 with propagated error
sums, regret matching over the held cards, the sampling thresholds, the external-sampling walk over full_chance_exploit_ref.tree_of's forest, the
rows' ranks and ring positions, and the FIFO average policy.

TEST INFRASTRUCTURE, written from the definitions.  The forward pass and its tolerance rule are oracle/sdcfr_policy_ref.py's (`forward`,
`positive_regret_policy`: tol = K * 2^-24 * S with K = 4 and S the propagated sum of |terms|), which are shape-free.

The walk is compared GIVEN the device's own policy table and thresholds, so no draw is ambiguous; its float32 arithmetic has one pinned order
(v = 0; v = v + p[s] * cfv[s], every operation rounded; d = cfv - v; d / (max|d| + float32(1e-8))), restated here in numpy float32, so regrets and
root values are compared on BITS: the largest deviation from this restatement measured on an MI355X is 0 (tests/test_gpu_full_chance_sdcfr.py).
Measured there against the float64 forward pass (K = 4), the largest |float32 - float64| / tolerance: the policy table 0.012 (Xavier, shifted and
all-negative nets; exact-arithmetic nets are bit-exact), the average-policy table 0.008 (1, 3 and 40 snapshots, training and held-out decks)."""
import numpy as np

import sdcfr_policy_ref as P

K, U24, EPS32 = P.K, P.U24, P.EPS32
FEATURES, ACTIONS = 96, 40
SHAPES = ((128, 96), (128,), (64, 128), (64,), (40, 64), (40,))
PHILOX_TAG = 224
ZERO_SUM = np.uint64(0xFFFFFFFFFFFFFFFF)
TWO53 = np.uint64(1 << 53)
CARDS = (3, 3, 2, 2)                       # held cards at choice level k & 3


def rows_per_traversal(R):
    return 4 * (6 ** R - 1) // 5


def visits_per_traversal(R, traverser):
    return (13, 8)[traverser] * (6 ** R - 1) // 5


# ---- features ------------------------------------------------------------------------------------------------------------------------------------
def features_of(a, b):
    a, b = int(a), int(b)
    f = np.zeros(FEATURES, np.float32)
    for c in range(40):
        f[c] = (b >> c) & 1
        f[40 + c] = (a >> (16 + c)) & 1
    player = (a >> 62) & 1
    f[80 + ((a >> 59) & 7)] = 1.0          # (the round is 0..5)
    f[86] = ((a >> 10) & 63) / 64.0
    s = ((a >> 5) & 31, a & 31)
    f[87], f[88] = s[player] / 32.0, s[1 - player] / 32.0
    f[89] = float(player)
    return f


def features(keys2):
    """float32 [n][96], vectorised; features_of is the one-key statement it is held to"""
    keys2 = np.asarray(keys2, np.uint64).reshape(-1, 2)
    a, b = keys2[:, 0:1], keys2[:, 1:2]
    c = np.arange(40, dtype=np.uint64)[None, :]
    one = np.uint64(1)
    f = np.zeros((len(keys2), FEATURES), np.float32)
    f[:, :40] = (b >> c) & one
    f[:, 40:80] = (a >> (c + np.uint64(16))) & one
    player = ((a >> np.uint64(62)) & one)[:, 0].astype(np.int64)
    rnd = ((a >> np.uint64(59)) & np.uint64(7))[:, 0].astype(np.int64)
    f[np.arange(len(keys2)), 80 + rnd] = 1.0
    f[:, 86] = ((a >> np.uint64(10)) & np.uint64(63))[:, 0].astype(np.float64) / 64.0
    s0, s1 = ((a >> np.uint64(5)) & np.uint64(31))[:, 0].astype(np.float64), (a & np.uint64(31))[:, 0].astype(np.float64)
    f[:, 87] = np.where(player == 1, s1, s0) / 32.0
    f[:, 88] = np.where(player == 1, s0, s1) / 32.0
    f[:, 89] = player
    return f


def slots_of(b):
    """the held cards in ascending card id = the action slots"""
    return [c for c in range(40) if (int(b) >> c) & 1]


# ---- nets ----------------------------------------------------------------------------------------------------------------------------------------
def xavier_net(seed, head_bias=0.1):
    rng = np.random.RandomState(seed)
    out = []
    for s in SHAPES:
        if len(s) == 2:
            a = np.sqrt(6.0 / (s[0] + s[1]))
            out.append(rng.uniform(-a, a, s).astype(np.float32))
        else:
            out.append(np.full(s, 0.1, np.float32))
    out[5] = np.full(SHAPES[5], head_bias, np.float32)
    return out


def negative_net(seed):
    """every advantage negative: the zero-sum branch at every node"""
    net = xavier_net(seed)
    net[4] = np.zeros(SHAPES[4], np.float32)
    net[5] = np.full(SHAPES[5], -1.0, np.float32)
    return net


def exact_net(seed):
    """weights in {-1, 0, 1} / 4, one in five non-zero, biases multiples of 1 / 4: every product and partial sum is a float32 value in any order"""
    rng = np.random.RandomState(seed)
    out = []
    for s in SHAPES:
        v = rng.randint(-1, 2, s) * (rng.rand(*s) < 0.2)
        out.append((v / 4.0).astype(np.float32))
    return out


def params64(net):
    return [np.asarray(a, np.float32).astype(np.float64).reshape(s) for a, s in zip(net, SHAPES)]


def node_policy(net, keys2, n_act, exact=False):
    """-> (policy [n][3], tolerance [n][3]) float64 in slot order, zeros beyond the count; evaluated once per distinct pair"""
    keys2 = np.asarray(keys2, np.uint64).reshape(-1, 2)
    n_act = np.asarray(n_act)
    uk, first, inv = np.unique(keys2, axis=0, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    feat = features(uk).astype(np.float64)
    adv, S = P.forward(params64(net), feat)
    if exact:
        assert (S < 4096.0).all() and np.array_equal(adv, adv.astype(np.float32).astype(np.float64)), "not an exact-arithmetic net"
        S = np.zeros_like(S)
    mask = feat[:, :ACTIONS]
    p, tol, z, _ = P.positive_regret_policy(adv, mask, S)
    if exact:
        p = p.astype(np.float32).astype(np.float64)
    cards = np.argsort(-mask, axis=1, kind="stable")[:, :3]            # the held cards in ascending card id, then cards not held
    live = np.arange(3)[None, :] < n_act[first][:, None]
    assert np.array_equal(mask.sum(1), n_act[first])
    out = np.take_along_axis(p, cards, 1) * live
    out_tol = np.take_along_axis(tol, cards, 1) * live
    return out[inv], out_tol[inv]


def thresholds(p3, n):
    """thr[2] uint64 of one node's float32 policy: scopa_sdcfr's definition on at most 3 slots"""
    pv = np.asarray(p3, np.float32)
    s = np.float32(pv[0] + pv[1])
    if n > 2:
        s = np.float32(s + pv[2])
    thr = [TWO53, TWO53]
    if s == np.float32(0.0):
        thr[0] = ZERO_SUM
        return np.array(thr, np.uint64)
    cdf, cs = [], 0.0
    for k in range(3):
        pq = float(np.float32(pv[k] / s))
        cs = cs + pq if k else pq
        cdf.append(cs)
    last = cdf[n - 1]
    for k in range(n - 1):
        thr[k] = np.uint64(int(np.ceil((cdf[k] / last) * 9007199254740992.0)))
    return np.array(thr, np.uint64)


def thresholds_all(pol, n_act):
    """`thresholds` of every row of pol [T][3] float32, vectorised -> [T][2] uint64"""
    pv, n = np.asarray(pol, np.float32), np.asarray(n_act)
    s = (pv[:, 0] + pv[:, 1]).astype(np.float32)
    s = np.where(n > 2, (s + pv[:, 2]).astype(np.float32), s)
    zero = s == np.float32(0.0)
    pq = (pv / np.where(zero, np.float32(1.0), s)[:, None]).astype(np.float32).astype(np.float64)
    c0 = pq[:, 0]
    c1 = c0 + pq[:, 1]
    c2 = c1 + pq[:, 2]
    last = np.where(n > 2, c2, c1)
    last = np.where(zero, 1.0, last)
    thr = np.full((len(pv), 2), TWO53, np.uint64)
    thr[:, 0] = np.ceil((c0 / last) * 9007199254740992.0).astype(np.uint64)
    thr[:, 1] = np.where(n > 2, np.ceil((c1 / last) * 9007199254740992.0).astype(np.uint64), TWO53)
    thr[zero, 0], thr[zero, 1] = ZERO_SUM, TWO53
    return thr


# ---- the forest ----------------------------------------------------------------------------------------------------------------------------------
class Forest:
    """the choice levels of full_chance_exploit_ref.tree_of's forest: keys [T][2] level-major and deck-major within a level, the leaves"""

    def __init__(self, tree, R):
        levels, leaf, n = tree
        self.R, self.L, self.n = R, 4 * R, n
        self.choice = [d for d, (_, k, _) in enumerate(levels) if k >= 2]
        assert len(self.choice) == self.L
        self.size = [len(levels[d][2]) for d in self.choice]
        self.off = np.concatenate([[0], np.cumsum(self.size)]).astype(np.int64)
        self.keys = np.array([k for d in self.choice for k in levels[d][2]], np.uint64).reshape(-1, 2)
        self.n_act = np.array([CARDS[k & 3] for k in range(self.L) for _ in range(self.size[k])], np.int32)
        self.leaf = np.array(leaf, np.float32)
        for k in range(self.L):
            assert levels[self.choice[k]][0] == (k & 1) and levels[self.choice[k]][1] == CARDS[k & 3]

    def level_nodes(self, player):
        """forest indices of the player's choice nodes, level-major: the order of average_policy's rows"""
        return np.concatenate([np.arange(self.off[k], self.off[k + 1]) for k in range(player, self.L, 2)])


def draw_N(level, g, trav_id, iteration, traverser, seed):
    o = P.philox4x32_10(np.uint64((level << 24) | int(g)), np.uint64(trav_id & 0xFFFFFFFF), np.uint64(iteration), np.uint64(PHILOX_TAG + traverser), int(seed))
    return (int(o[0]) >> 5 << 26) | (int(o[1]) >> 6)


def action_of(thr2, N, n):
    if thr2[0] == ZERO_SUM:
        a = int((N * 2.0 ** -53) * n)
    else:
        a = int(int(thr2[0]) <= N) + int(int(thr2[1]) <= N)
    return min(a, n - 1)


def row_of(pl, av, n):
    """(value, regret of the cards not held, regrets of the slots [3]) in float32, the pinned order"""
    f = np.float32
    v = f(0.0)
    for k in range(n):
        v = f(v + f(f(pl[k]) * f(av[k])))
    ri = f(f(0.0) - v)
    d = [f(f(av[k]) - v) if k < n else f(f(0.0) - v) for k in range(3)]
    mx = max([abs(ri)] + [abs(d[k]) for k in range(n)])
    if mx > 0:
        den = f(f(mx) + f(1e-8))
        ri = f(ri / den)
        d = [f(x / den) for x in d]
    return v, ri, d


def regret_row(b, ri, d):
    out = np.full(ACTIONS, ri, np.float32)
    for s, c in enumerate(slots_of(b)):
        out[c] = d[s]
    return out


def walk(forest, pol, thr, traverser, deck, trav_id, iteration, seed):
    """One traversal level by level, driven by the tables pol [T][3] float32 and thr [T][2] uint64
    -> dict(rows={rank: (forest node, regret [40] float32)}, value float32, visits, path={(level, g): slot drawn})"""
    L = forest.L
    frontier, fronts, path, visits = [deck], [], {}, 0
    for k in range(L):
        n = CARDS[k & 3]
        fronts.append(frontier)
        visits += len(frontier)
        if (k & 1) == traverser:
            frontier = [g * n + a for g in frontier for a in range(n)]
        else:
            nxt = []
            for g in frontier:
                a = action_of(thr[forest.off[k] + g], draw_N(k, g, trav_id, iteration, traverser, seed), n)
                path[(k, g)] = a
                nxt.append(g * n + a)
            frontier = nxt
    val = [np.float32(forest.leaf[g]) if traverser == 0 else np.float32(-forest.leaf[g]) for g in frontier]
    rank0, r = {}, 0
    for k in range(L):
        if (k & 1) == traverser:
            rank0[k] = r
            r += len(fronts[k])
    assert r == rows_per_traversal(forest.R)
    rows = {}
    for k in reversed(range(L)):
        if (k & 1) != traverser:
            continue
        n = CARDS[k & 3]
        up = []
        for f, g in enumerate(fronts[k]):
            idx = int(forest.off[k] + g)
            v, ri, d = row_of(pol[idx], val[f * n:f * n + n], n)
            rows[rank0[k] + f] = (idx, regret_row(forest.keys[idx, 1], ri, d))
            up.append(v)
        val = up
    return dict(rows=rows, value=val[0], visits=visits, path=path)


def ring_row(write_base, rows, slot, batch, i, rank, capacity):
    return (write_base + rows * (slot * batch + i) + rank) % capacity


# ---- the average policy ----------------------------------------------------------------------------------------------------------------------------
def average_policy(snapshots, coefs, keys2, n_act):
    """FIFO average of the snapshots' policies with float32 coefficients, normalised over the legal slots in float64
    -> (policy [n][3], tolerance [n][3], ambiguous [n]: the sum lies within tolerance of 0, uniform or not)"""
    keys2 = np.asarray(keys2, np.uint64).reshape(-1, 2)
    n = len(keys2)
    acc, tol, run = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
    for net, c in zip(snapshots, coefs):
        c = float(np.float32(c))
        p, tp = node_policy(net, keys2, n_act)
        acc += c * p
        run += np.abs(acc)
        tol += c * (tp + K * U24 * p)
    tol += K * U24 * run
    live = np.arange(3)[None, :] < np.asarray(n_act)[:, None]
    s = acc.sum(1, keepdims=True)
    ts = tol.sum(1, keepdims=True)
    ok = (s > 0) & np.isfinite(s)
    safe = np.where(ok, s, 1.0)
    q = np.where(ok, acc / safe, live / np.asarray(n_act)[:, None].astype(np.float64))
    tq = np.where(ok, (tol + q * ts) / safe + K * U24 * q, 0.0)
    return q * live, tq * live, (s <= ts)[:, 0] & (ts[:, 0] > 0)
