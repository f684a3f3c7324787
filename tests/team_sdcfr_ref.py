"""Numpy restatement of Single Deep CFR's traversal and average policy on Team MiniScopa over a set of deals (scopa_team_chance_sdcfr.hip).

TEST INFRASTRUCTURE, written for this repository's tests.  The rules come from the oracle's TeamState (oracle/oracle.py); the advantage net is the
reference's 34-128-64-16 MLP (torch layout W[out][in]).  Three parts:

  forward      the float64 forward pass of a net on feature bits (hand one-hot | table multi-hot << 16, then [1, 0]) and positive_regret_policy
               (nets.py:93-101): relu(adv) * mask / max(sum, 1e-8)
  thresholds   the sampling thresholds of a float32 policy row, bit for bit the rule sd_thresholds (scopa_sdcfr_tile.h): float32 p / sum, float64
               cdf left to right, thr[k] = ceil(cdf_k / cdf_last * 2^53) for k < nl - 1, 2^53 beyond, thr[0] = 2^64 - 1 where the float32 sum is 0
  traverse     DeepCFR._external_sampling_cfr (deep_cfr.py:284-365) as a recursion over TeamState in the reference's visit and append order:
               the traverser's team recurses into every legal card in hand order, value = sum policy[a] * child value in float32, regrets = cfv - value
               over all 16 slots, the row (features, regrets / (max|.| + 1e-8), mask) appended AFTER the children -- at the forced plies 12..15 too,
               where the policy of the one legal card is relu(adv) / max(relu(adv), 1e-8) --; the other team's plies take one action from a
               caller-supplied chooser.  The policy at a node comes from a caller-supplied function as well, so the traversal runs (a) on a scripted
               action sequence, (b) on a given policy / threshold table with the library's Philox keying, (c) on its own float64 policies.

and the average policy over keys (StrategyBuffer.get_average_policy, deep_cfr.py:137-160, per distinct key).
"""
import ctypes as C
import os

import numpy as np

import oracle as O
import team_chance_ref as TC
from team_cfr_ref import N_CHOICE, N_LEAVES, OFFSET, WIDTH, branch, team_of

ROWS = 1653                       # memory rows of one traversal: 501 choice + 2 x 576 forced (NOT MiniScopa's 1 653 decision nodes)
VISITS = (4277, 3127)             # non-terminal visits of one traversal, per traverser
CHOICE_VISITS = (1973, 823)       # ... of which at choice nodes (depths 0..11)
ARRIVALS = 576                    # depth-12 arrivals
PHILOX_TAG = 96                   # counter word 3 = 96 + traverser
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---- nets ---------------------------------------------------------------------------------------------------------------------------------
def golden_nets():
    """the two advantage nets of tests/golden/sdcfr.npz as [dict(w1, b1, w2, b2, w3, b3)] float32 (net p = team p)"""
    z = np.load(os.path.join(GOLDEN, "sdcfr.npz"))
    names = ("_backbone.0.fc.weight", "_backbone.0.fc.bias", "_backbone.1.fc.weight", "_backbone.1.fc.bias", "_head.weight", "_head.bias")
    return [dict(zip(("w1", "b1", "w2", "b2", "w3", "b3"), (z[f"net{p}_{n}"].astype(np.float32) for n in names))) for p in range(2)]


def with_head_bias(net, value):
    out = dict(net)
    out["b3"] = np.full(16, value, np.float32)
    return out


def random_net(seed, head_bias=0.0):
    r = np.random.default_rng(seed)
    u = lambda n_out, n_in: r.uniform(-1, 1, (n_out, n_in)).astype(np.float32) / np.float32(np.sqrt(n_in))
    return dict(w1=u(128, 34), b1=r.uniform(-.1, .1, 128).astype(np.float32), w2=u(64, 128), b2=r.uniform(-.1, .1, 64).astype(np.float32),
                w3=u(16, 64), b3=(r.uniform(-.1, .1, 16) + head_bias).astype(np.float32))


def net_flat(net):
    """the six tensors in state_dict order, flattened (DeepCFR's parameter order)"""
    return np.concatenate([net[k].reshape(-1) for k in ("w1", "b1", "w2", "b2", "w3", "b3")]).astype(np.float32)


def features_of_bits(xbits):
    """[N] uint32 -> [N][34] float32: hand one-hot, table multi-hot, [1, 0]"""
    xbits = np.asarray(xbits, np.uint32).reshape(-1)
    f = np.zeros((xbits.shape[0], 34), np.float32)
    f[:, :32] = ((xbits[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1).astype(np.float32)
    f[:, 32] = 1.0
    return f


def forward64(net, xbits):
    """raw advantages [N][16] float64"""
    x = features_of_bits(xbits).astype(np.float64)
    h1 = np.maximum(x @ net["w1"].astype(np.float64).T + net["b1"].astype(np.float64), 0.0)
    h2 = np.maximum(h1 @ net["w2"].astype(np.float64).T + net["b2"].astype(np.float64), 0.0)
    return h2 @ net["w3"].astype(np.float64).T + net["b3"].astype(np.float64)


def policy64(net, xbits):
    """positive_regret_policy in float64 -> (policy [N][16], z [N] the positive-advantage sum over the legal slots)"""
    xbits = np.asarray(xbits, np.uint32).reshape(-1)
    mask = ((xbits[:, None] >> np.arange(16, dtype=np.uint32)[None, :]) & 1).astype(np.float64)
    pos = np.maximum(forward64(net, xbits), 0.0) * mask
    z = pos.sum(1)
    return pos / np.maximum(z, 1e-8)[:, None], z


def hand_order(p16, hand, nl):
    """[N][16] by card id -> [N][4] in hand order (nibble k of hand = the card of slot k), zeros beyond nl"""
    hand = np.asarray(hand, np.int64).reshape(-1)
    out = np.zeros((hand.shape[0], 4), p16.dtype)
    for k in range(4):
        card = (hand >> (4 * k)) & 15
        out[:, k] = np.where(k < np.asarray(nl), p16[np.arange(hand.shape[0]), card], 0)
    return out


# ---- thresholds -----------------------------------------------------------------------------------------------------------------------------
TWO53 = np.uint64(1 << 53)
ZERO_SUM = np.uint64(0xFFFFFFFFFFFFFFFF)


def thresholds(p4, nl):
    """[N][4] float32 policy rows (hand order) with nl [N] legal slots -> [N][3] uint64, the rule of sd_thresholds<4> (scopa_sdcfr_tile.h) bit for bit"""
    p4 = np.asarray(p4, np.float32).reshape(-1, 4)
    nl = np.broadcast_to(np.asarray(nl, np.int64), (p4.shape[0],))
    s = p4[:, 0].copy()
    for k in range(1, 4):
        s = np.where(k < nl, (s + p4[:, k]).astype(np.float32), s)                 # action_probs.sum(), float32, left to right
    thr = np.full((p4.shape[0], 3), TWO53, np.uint64)
    zero = s == np.float32(0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = (p4 / s[:, None]).astype(np.float32).astype(np.float64)               # float32 p, float64 cdf
    cdf = np.zeros((p4.shape[0], 4))
    c = q[:, 0].copy()
    cdf[:, 0] = c
    for k in range(1, 4):
        c = c + q[:, k]
        cdf[:, k] = c
    last = cdf[np.arange(p4.shape[0]), nl - 1]
    for k in range(3):
        m = (k < nl - 1) & ~zero
        with np.errstate(divide="ignore", invalid="ignore"):
            v = np.ceil((cdf[:, k] / last) * 9007199254740992.0)
        thr[m, k] = v[m].astype(np.uint64)
    thr[zero, 0] = ZERO_SUM
    return thr


def action_of(thr3, N, nl):
    """the walk's compare: #{k : thr[k] <= N}; a zero sum keeps numpy's uniform arithmetic (int)(u * nl)"""
    if int(thr3[0]) == int(ZERO_SUM):
        a = int((float(N) * 2.0 ** -53) * float(nl))
    else:
        a = sum(1 for k in range(3) if int(thr3[k]) <= int(N))
    return min(a, nl - 1)


# ---- Philox (the library's keying) ------------------------------------------------------------------------------------------------------------
def philox4x32_10(c, k):
    c, k = [int(x) for x in c], [int(x) for x in k]
    M = 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & M, (p0 >> 32) ^ c[3] ^ k[1], p0 & M]
        k = [(k[0] + 0x9E3779B9) & M, (k[1] + 0xBB67AE85) & M]
    return c


def draw_N(row, trav_id, iteration, traverser, seed):
    """the 53-bit integer N of the draw at local row `row`: u = N * 2^-53"""
    x = philox4x32_10((row, trav_id & 0xFFFFFFFF, iteration & 0xFFFFFFFF, PHILOX_TAG + traverser), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return ((x[0] >> 5) << 26) | (x[1] >> 6)


# ---- a deal's node info ---------------------------------------------------------------------------------------------------------------------------
_INFO = {}


def node_info(perm):
    """(xbits uint32 [321365], hand uint16 [321365], forced xbits uint32 [4][331776], r2 int8 [331776]) of a deal: feature bits and the mover's
    remaining hand nibbles (hand order) of every choice row, feature bits of the four forced nodes below every depth-12 node -- a level-wise walk
    over the oracle's transitions (team_chance_ref.walk's)"""
    kb = bytes(np.ascontiguousarray(perm, np.uint8))
    if kb in _INFO:
        return _INFO[kb]
    u = np.uint64
    p = np.frombuffer(kb, np.uint8).astype(np.uint64)
    hands = [np.array([p[4 * s] | p[4 * s + 1] << u(4) | p[4 * s + 2] << u(8) | p[4 * s + 3] << u(12)], np.uint64) for s in range(4)]
    tab, nt = np.zeros(1, np.uint64), np.zeros(1, np.int64)
    xbits, hand_out, fx = np.zeros(N_CHOICE, np.uint32), np.zeros(N_CHOICE, np.uint16), np.zeros((4, N_LEAVES), np.uint32)

    def bits(words, counts, width):
        b = np.zeros(words.shape[0], np.uint64)
        for i in range(width):
            b |= np.where(i < counts, u(1) << ((words >> u(4 * i)) & u(15)), u(0))
        return b

    for d in range(16):
        seat, b = d & 3, branch(d) if d < 12 else 1
        h = hands[seat]
        xb = (bits(h, np.full(h.shape[0], b), 4) | bits(tab, nt, 8) << u(16)).astype(np.uint32)
        if d < 12:
            xbits[OFFSET[d]:OFFSET[d] + WIDTH[d]] = xb
            hand_out[OFFSET[d]:OFFSET[d] + WIDTH[d]] = h.astype(np.uint16)
        else:
            fx[d - 12] = xb
        c = np.arange(b, dtype=np.uint64)[None, :]
        card = (h[:, None] >> (u(4) * c)) & u(15)
        left = (h[:, None] & ((u(1) << (u(4) * c)) - u(1))) | ((h[:, None] >> (u(4) * c + u(4))) << (u(4) * c))
        rep = lambda a: np.repeat(a, b)
        combo = rep(tab) | rep(nt).astype(np.uint64) << u(32) | card.reshape(-1) << u(36)
        uq, inv = np.unique(combo, return_inverse=True)
        for x in uq.tolist():
            if x not in TC._TRANSITIONS:
                TC._TRANSITIONS[x] = TC._transition(x & 0xFFFFFFFF, (x >> 32) & 15, x >> 36)
        r = np.array([TC._TRANSITIONS[x] for x in uq.tolist()], np.int64).reshape(-1, 4)[inv]
        hands = [left.reshape(-1) if s == seat else rep(hands[s]) for s in range(4)]
        tab, nt = r[:, 0].astype(np.uint64), r[:, 1]
    out = (xbits, hand_out, fx, TC.walk(perm)[1])
    for a in out[:3]:
        a.setflags(write=False)
    _INFO[kb] = out
    return out


def float64_tables(perm, nets, traverser=None):
    """a deal's policy tables under `nets` in float64: (policy [321365][4] hand order, z [321365], forced policy [4][331776], forced z) -- every choice
    row under the net of the row's team, the forced nodes of depth 12 + f under the net of team f >> 1 for the two depths of `traverser` (None: none)"""
    xbits, hand, fx, _ = node_info(perm)
    pol, z = np.zeros((N_CHOICE, 4)), np.zeros(N_CHOICE)
    for d in range(12):
        rows = slice(OFFSET[d], OFFSET[d] + WIDTH[d])
        p16, zz = policy64(nets[team_of(d)], xbits[rows])
        pol[rows], z[rows] = hand_order(p16, hand[rows], branch(d)), zz
    fpol, fz = np.zeros((4, N_LEAVES)), np.zeros((4, N_LEAVES))
    for f in range(4):
        if traverser is None or (f >> 1) != traverser:
            continue
        p16, zz = policy64(nets[f >> 1], fx[f])
        card = np.log2((fx[f] & 0xFFFF).astype(np.float64)).astype(np.int64)
        fpol[f], fz[f] = p16[np.arange(N_LEAVES), card], zz
    return pol, z, fpol, fz


def forced64(perm, nets, traverser, stride=1):
    """(policy [2][n], z [2][n]) in float64 of the one legal card at every stride-th node of the traverser's two forced depths"""
    fx = node_info(perm)[2]
    p, z = [], []
    for f in (2 * traverser, 2 * traverser + 1):
        xb = fx[f][::stride]
        p16, zz = policy64(nets[traverser], xb)
        p.append(p16[np.arange(xb.shape[0]), np.log2((xb & 0xFFFF).astype(np.float64)).astype(np.int64)])
        z.append(zz)
    return np.array(p), np.array(z)


def legal_count_of_rows():
    nl = np.zeros(N_CHOICE, np.int64)
    for d in range(12):
        nl[OFFSET[d]:OFFSET[d] + WIDTH[d]] = branch(d)
    return nl


# ---- the traversal ------------------------------------------------------------------------------------------------------------------------------
def _clone(st):
    c = O.TeamState.__new__(O.TeamState)
    c.perm = st.perm
    c.s = O._TeamState.from_buffer_copy(st.s)
    return c


def state_bits(st):
    """(feature bits, hand cards in hand order) of the seat to move, read off the oracle's state"""
    s = st.s
    seat = int(s.step) & 3
    cards = [int(s.hand[seat][i]) for i in range(s.nh[seat])]
    xb = 0
    for c in cards:
        xb |= 1 << c
    for i in range(s.nt):
        xb |= 1 << (16 + int(s.table[i]))
    return xb, cards


class Traversal:
    """one traversal; rows = [(feature bits, regrets float32 [16], mask bits)] in append order, value float32, visits per depth"""

    def __init__(self, perm, traverser, policy_fn, choose_fn):
        """policy_fn(depth, node index within the level, feature bits, cards) -> float32 [len(cards)] policy of the legal cards, hand order;
        choose_fn(depth, node, cards, policy) -> slot of the sampled card (the other team's plies with more than one card)"""
        self.traverser, self.policy_fn, self.choose_fn = traverser, policy_fn, choose_fn
        self.rows, self.visits, self.sampled = [], np.zeros(16, np.int64), []
        self.value = self._walk(O.TeamState(perm=perm), 0, 0)

    def _walk(self, st, depth, node):
        if st.is_terminal():
            return np.float32(st.rewards()[self.traverser])
        self.visits[depth] += 1
        xb, cards = state_bits(st)
        assert st.legal() == cards and st.current_player() == ((depth & 3) >> 1)
        pol = np.asarray(self.policy_fn(depth, node, xb, cards), np.float32)
        nl = len(cards)
        if ((depth & 3) >> 1) == self.traverser:
            value, cfv = np.float32(0.0), np.zeros(16, np.float32)
            for k, card in enumerate(cards):
                ch = _clone(st)
                ch.step(card)
                av = self._walk(ch, depth + 1, node * nl + k if depth < 12 else node)
                value = np.float32(value + np.float32(pol[k] * av))
                cfv[card] = av
            reg = (cfv - value).astype(np.float32)
            mx = np.float32(np.max(np.abs(reg)))
            if mx > 0:
                reg = (reg / np.float32(mx + np.float32(1e-8))).astype(np.float32)   # add_experience (:73-74)
            self.rows.append((xb, reg, xb & 0xFFFF))
            return value
        k = 0
        if nl > 1:
            k = int(self.choose_fn(depth, node, cards, pol))
            self.sampled.append(cards[k])
        ch = _clone(st)
        ch.step(cards[k])
        return self._walk(ch, depth + 1, node * nl + k if depth < 12 else node)

    def arrays(self):
        return (np.array([r[0] for r in self.rows], np.uint32), np.array([r[1] for r in self.rows], np.float32).reshape(-1, 16),
                np.array([r[2] for r in self.rows], np.uint16))


def scripted(actions):
    """mode (a): the other team's cards in visit order"""
    it = iter(actions)
    return lambda depth, node, cards, pol: cards.index(int(next(it)))


def table_policy(pol4, fpol2, traverser):
    """policy_fn over a deal's table: float32 [321365][4] for the choice rows, [2][331776] for the traverser's forced depths (None: the other team's
    forced plies, whose policy nothing reads)"""
    def fn(depth, node, xb, cards):
        if depth < 12:
            return pol4[OFFSET[depth] + node, :len(cards)]
        if ((depth & 3) >> 1) != traverser:
            return np.ones(1, np.float32)
        return fpol2[depth - 12 - 2 * traverser, node:node + 1]
    return fn


def philox_chooser(thr, traverser, trav_id, iteration, seed):
    """mode (b): the library's draw at the node's local row against the table's thresholds [321365][3]"""
    def fn(depth, node, cards, pol):
        row = OFFSET[depth] + node
        return action_of(thr[row], draw_N(row, trav_id, iteration, traverser, seed), len(cards))
    return fn


def own_policy(nets):
    """mode (c): the float64 forward at every visit, rounded to float32"""
    def fn(depth, node, xb, cards):
        p16, _ = policy64(nets[(depth & 3) >> 1], np.array([xb], np.uint32))
        return p16[0, cards].astype(np.float32)
    return fn


def numpy_chooser(rng):
    """the reference's np.random.choice on float32 probabilities with the uniform fall-back"""
    def fn(depth, node, cards, pol):
        s = pol.sum()
        return int(rng.choice(len(cards))) if s == 0 else int(rng.choice(len(cards), p=pol / s))
    return fn


# ---- the words of the GPU walk test (tests/philox_words.py's conventions): ids are b0 + deal * batch + i, accepted up to b0 = 2^32 - n * batch ---------
TSD_SEED = 0x7EA4D33C


def last_b0(n, batch):
    return (1 << 32) - n * batch


def word_cases(n, batch):
    """(seed, iteration, b0) with one word wide at a time, then all at once"""
    import philox_words as W
    return W.word_cases(TSD_SEED, batch, last_b0(n, batch), small_iteration=3, small_b0=0)


def ring_rows(write_base, slot, batch, i, capacity):
    return (write_base + ROWS * (slot * batch + i) + np.arange(ROWS)) % capacity


# ---- the average policy over keys -----------------------------------------------------------------------------------------------------------------
def average_policy(cr, perms, team, snapshots, coefs):
    """cr = team_chance_ref.ChanceRef: per distinct key of `team`, x from the key's first occurrence: the FIFO float32 sum of
    positive_regret_policy(net_s(x)) * coef[s] (here from float64 policies), normalised over the legal slots in float64, uniform where the sum is 0 or
    not finite (a NaN coefficient gives that), zeros beyond the legal count -> (rows of the team [K], table [K][4] float64, z [S][K])"""
    rows = np.nonzero(cr.team == team)[0]
    first = cr.occ[cr.occ_off[rows]]
    deal, local = first // N_CHOICE, first % N_CHOICE
    xb, hand = np.zeros(len(rows), np.uint32), np.zeros(len(rows), np.uint16)
    for d in range(cr.n):
        info = node_info(perms[d])
        m = deal == d
        xb[m], hand[m] = info[0][local[m]], info[1][local[m]]
    nl = cr.nleg[rows]
    acc = np.zeros((len(rows), 4), np.float32)
    zs = np.zeros((len(snapshots), len(rows)))
    for s, (net, coef) in enumerate(zip(snapshots, coefs)):
        p16, z = policy64(net, xb)
        zs[s] = z
        with np.errstate(invalid="ignore"):
            acc = (acc + (hand_order(p16, hand, nl).astype(np.float32) * np.float32(coef)).astype(np.float32)).astype(np.float32)
    live = np.arange(4)[None, :] < nl[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        total = np.where(live, acc.astype(np.float64), 0.0).sum(1)
        uniform = ~(total > 0.0) | np.isinf(total)
        out = np.where(live, np.where(uniform[:, None], 1.0 / nl[:, None], acc.astype(np.float64) / total[:, None]), 0.0)
    return rows, out, zs
