"""Float64 numpy restatement of Team MiniScopa over a set of deals (scopa_team_chance.hip), on tests/team_cfr_ref.py's Ref: the keys and the index
of shared rows, the alternating weighted sweep with the fixed-order reduce, the level-wise best response across deals.

TEST INFRASTRUCTURE, written for this repository's tests.  The rules come from the oracle (oracle/oracle.py): a level-wise walk asks it for every
distinct (table, card) transition once, which gives a deal's keys and payoffs in a fraction of a second (checked against team_cfr_ref.leaves).
Every float64 operation is one numpy elementwise operation (one rounding, no fused multiply-add), in the kernels' documented order:

  key       depth << 60 | acting seat's initial hand (nibble i = hand position i) << 44 | cards played so far (nibble i = ply i)
  index     distinct keys ascending; map[n][321365] local row -> global id; occurrences deal * 321365 + row ascending per global id
  sweep     per deal Ref's traversal arithmetic against the sigma rows gathered through map; a traverser's row yields {opp * (u - v), reach * ls}
  reduce    a row's increments added over its occurrences in ascending order STARTING FROM THE FIRST one's value; then R <- R + dR;
            R <- !(R <= 0) ? R * pos : R * neg; S <- (S + dS) * strat (weights None = no multiplication); sigma by regret matching
  root      (v_deal0 + v_deal1 + ...) / n in deal order
  best response   per responder, depth 11 up: q = opp_reach * val(child) per node, added per global row in the same fixed order, first slot best by a
            strict `>`; the other team's levels v = 0.0; v += row[c] * val(child c)
"""
import ctypes as C

import numpy as np

import oracle as O
import team_cfr_ref as T
from team_cfr_ref import N_CHOICE, N_LEAVES, OFFSET, WIDTH, branch, team_of

_WALKS, _TRANSITIONS = {}, {}


def _transition(table, nt, card):
    """the oracle's step of a seat that plays `card` onto `table` -> (new table word, new nt, cards captured incl. the played one, scopa)"""
    s = O._TeamState()
    s.hand[0][0], s.nh[0] = card, 1
    s.hand[1][0], s.nh[1] = (card + 1) & 15, 1   # someone still holds a card: the step does not end the game
    for i in range(nt):
        s.table[i] = (table >> (4 * i)) & 15
    s.nt, s.last_capture_team = nt, -1
    O.lib().ogt_step(C.byref(s), int(card))
    new = 0
    for i in range(s.nt):
        new |= int(s.table[i]) << (4 * i)
    return new, int(s.nt), int(s.ncap[0]), int(s.scopas[0])


def walk(perm):
    """(keys uint64 [321365], r2 int8 [331776]) of a deal: every choice node's key in row order, reward x2 of team 0 at every depth-12 node"""
    kb = bytes(np.ascontiguousarray(perm, np.uint8))
    if kb in _WALKS:
        return _WALKS[kb]
    perm = np.frombuffer(kb, np.uint8).astype(np.uint64)
    init = [perm[4 * s] | perm[4 * s + 1] << np.uint64(4) | perm[4 * s + 2] << np.uint64(8) | perm[4 * s + 3] << np.uint64(12) for s in range(4)]
    hands = [np.array([h], np.uint64) for h in init]
    tab, nt, score, lct, hist = np.zeros(1, np.uint64), np.zeros(1, np.int64), np.zeros(1, np.int64), np.full(1, -1, np.int64), np.zeros(1, np.uint64)
    keys = np.zeros(N_CHOICE, np.uint64)
    u = np.uint64
    for d in range(16):
        seat, b = d & 3, branch(d) if d < 12 else 1
        if d < 12:
            keys[OFFSET[d]:OFFSET[d] + WIDTH[d]] = u(d << 60) | init[seat] << u(44) | hist
        c = np.arange(b, dtype=np.uint64)[None, :]
        h = hands[seat][:, None]
        card = (h >> (u(4) * c)) & u(15)
        left = (h & ((u(1) << (u(4) * c)) - u(1))) | ((h >> (u(4) * c + u(4))) << (u(4) * c))
        rep = lambda a: np.repeat(a, b)
        combo = (rep(tab) | rep(nt).astype(np.uint64) << u(32) | card.reshape(-1) << u(36))
        uq, inv = np.unique(combo, return_inverse=True)
        for x in uq.tolist():
            if x not in _TRANSITIONS:
                _TRANSITIONS[x] = _transition(x & 0xFFFFFFFF, (x >> 32) & 15, x >> 36)
        res = np.array([_TRANSITIONS[x] for x in uq.tolist()], np.int64).reshape(-1, 4)
        r = res[inv]
        sign = 1 if seat < 2 else -1
        hist = rep(hist) | card.reshape(-1) << u(4 * d)
        hands = [left.reshape(-1) if s == seat else rep(hands[s]) for s in range(4)]
        tab, nt = r[:, 0].astype(np.uint64), r[:, 1]
        score = rep(score) + sign * (r[:, 2] + 2 * r[:, 3])
        lct = np.where(r[:, 2] > 0, seat >> 1, rep(lct))
    score = score + np.where((nt > 0) & (lct >= 0), np.where(lct == 0, nt, -nt), 0)   # the leftovers go to the last capturing team
    assert score.shape == (N_LEAVES,)
    out = (keys, score.astype(np.int8))
    for a in out:
        a.setflags(write=False)
    _WALKS[kb] = out
    return out


def ref_of(perm):
    """team_cfr_ref.Ref of a deal with the walk's payoffs in place of its slower enumeration (test_team_chance_ref.py holds the two equal)"""
    T._LEAVES.setdefault(bytes(np.ascontiguousarray(perm, np.uint8)), walk(perm)[1])
    return T.Ref(perm)


def make_key(depth, hand, history):
    key = int(depth) << 60
    for i, c in enumerate(hand):
        key |= int(c) << (44 + 4 * i)
    for i, c in enumerate(history):
        key |= int(c) << (4 * i)
    return key


def key_depth(keys):
    return (np.asarray(keys, np.uint64) >> np.uint64(60)).astype(np.int64)


def _sum_left(x):
    """x[:, 0] + x[:, 1] + ... left to right"""
    s = x[..., 0].copy()
    for c in range(1, x.shape[-1]):
        s = s + x[..., c]
    return s


class ChanceRef:
    def __init__(self, perms):
        self.perms = np.ascontiguousarray(perms, np.uint8).reshape(-1, 16)
        self.n = n = self.perms.shape[0]
        walks = [walk(p) for p in self.perms]
        keys = np.stack([w[0] for w in walks])
        self.r2 = np.stack([w[1] for w in walks]).astype(np.int64)                  # [n][331776]
        self.gkey, inv = np.unique(keys.reshape(-1), return_inverse=True)
        self.G = self.gkey.shape[0]
        self.map = inv.reshape(n, N_CHOICE).astype(np.int32)
        flat = self.map.reshape(-1).astype(np.int64)
        self.occ = np.argsort(flat, kind="stable").astype(np.int64)                 # deal * 321365 + row, ascending per global id
        counts = np.bincount(flat, minlength=self.G)
        self.occ_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self.depth = key_depth(self.gkey)
        self.nleg = 4 - (self.depth >> 2)
        self.team = (self.depth & 3) >> 1
        self.depth_off = np.searchsorted(self.depth, np.arange(13))

    # ---- tables -------------------------------------------------------------------------------------------------------------------------
    def sigma(self, R):
        out = np.zeros((self.G, 4))
        for b in (2, 3, 4):
            m = self.nleg == b
            out[m] = T.Ref.sigma(R[m], b)
        return out

    def tables(self):
        R = np.zeros((self.G, 4))
        return R, np.zeros((self.G, 4)), self.sigma(R)

    def reduce_rows(self, img, rows):
        """img [n * 321365][k] summed over the occurrences of the global rows `rows`, in occurrence order from the first -> [len(rows)][k]"""
        o, cnt = self.occ_off[rows], self.occ_off[rows + 1] - self.occ_off[rows]
        acc = img[self.occ[o]].copy()
        for k in range(1, int(cnt.max()) if len(rows) else 0):
            m = cnt > k
            acc[m] = acc[m] + img[self.occ[o[m] + k]]
        return acc

    # ---- the sweep ------------------------------------------------------------------------------------------------------------------------
    def sweep(self, sig, p):
        """all deals against the sigma table `sig` [G][4] for traverser p -> (increment image [n * 321365][8], per-deal root values [n])"""
        n = self.n
        L = sig[self.map]                                                            # [n][321365][4]
        img = np.zeros((n, N_CHOICE, 8))
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            r = {0: (np.ones((n, 1)), np.ones((n, 1)))}
            for d in range(11):
                b, sg = branch(d), L[:, OFFSET[d]:OFFSET[d] + WIDTH[d], :branch(d)]
                r0, r1 = r[d]
                c0 = (r0[:, :, None] * sg) if team_of(d) == 0 else np.repeat(r0[:, :, None], b, 2)
                c1 = (r1[:, :, None] * sg) if team_of(d) == 1 else np.repeat(r1[:, :, None], b, 2)
                r[d + 1] = (c0.reshape(n, -1), c1.reshape(n, -1))
            val = 0.5 * (self.r2 if p == 0 else -self.r2).astype(np.float64)
            for d in range(11, -1, -1):
                b, rows = branch(d), slice(OFFSET[d], OFFSET[d] + WIDTH[d])
                u, ls = val.reshape(n, -1, b), L[:, rows, :b]
                prod = ls * u
                v = _sum_left(prod)
                if team_of(d) == p:
                    reach, opp = r[d][p], r[d][1 - p]
                    img[:, rows, :b] = opp[:, :, None] * (u - v[:, :, None])
                    img[:, rows, 4:4 + b] = reach[:, :, None] * ls
                val = v
        return img.reshape(n * N_CHOICE, 8), val[:, 0].copy()

    def mean(self, per_deal):
        s = per_deal[0]
        for k in range(1, self.n):
            s = s + per_deal[k]
        return s / float(self.n)

    def traverse(self, R, S, sig, p, w=None):
        """one traversal of team p on the shared tables in place (sig refreshed for the updated rows) -> root value"""
        img, roots = self.sweep(sig, p)
        rows = np.nonzero(self.team == p)[0]
        acc = self.reduce_rows(img, rows)
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            for b in (2, 3, 4):
                m = self.nleg[rows] == b
                g = rows[m]
                Rn = R[g, :b] + acc[m, :b]
                Sn = S[g, :b] + acc[m, 4:4 + b]
                if w is not None:
                    Rn = np.where(~(Rn <= 0.0), Rn * float(w[0]), Rn * float(w[1]))
                    Sn = Sn * float(w[2])
                R[g, :b], S[g, :b] = Rn, Sn
                sig[g] = T.Ref.sigma(R[g], b)
            return float(self.mean(roots))

    def iterate(self, R, S, sig, n_iters=None, weights=None):
        ws = [None] * n_iters if weights is None else list(np.asarray(weights, np.float64).reshape(-1, 3))
        out = np.zeros((len(ws), 2))
        for t, w in enumerate(ws):
            for p in (0, 1):
                out[t, p] = self.traverse(R, S, sig, p, w)
        return out

    # ---- best response across deals ---------------------------------------------------------------------------------------------------------
    def average_policy(self, S):
        out = np.zeros((self.G, 4))
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            for b in (2, 3, 4):
                m = self.nleg == b
                s = _sum_left(S[m, :b])
                out[m, :b] = np.where((s > 0.0)[:, None], S[m, :b] / s[:, None], 1.0 / b)
        return out

    def value_pass(self, pol, responder):
        """one pass; responder 0 / 1: that team best-responds across deals, valued for itself; None: both follow, valued for team 0.
        -> (per-deal root values [n], choice int [G] or None)"""
        n = self.n
        persp = 1 if responder == 1 else 0
        P = pol[self.map]                                                            # [n][321365][4]
        choice = np.zeros(self.G, np.int64) if responder is not None else None
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            reach = {0: np.ones((n, 1))}
            if responder is not None:
                for d in range(11):
                    b = branch(d)
                    a = reach[d][:, :, None]
                    ch = a * P[:, OFFSET[d]:OFFSET[d] + WIDTH[d], :b] if team_of(d) != responder else np.repeat(a, b, 2)
                    reach[d + 1] = ch.reshape(n, -1)
            val = 0.5 * (self.r2 if persp == 0 else -self.r2).astype(np.float64)
            for d in range(11, -1, -1):
                b, rows = branch(d), slice(OFFSET[d], OFFSET[d] + WIDTH[d])
                u = val.reshape(n, -1, b)
                if responder is not None and team_of(d) == responder:
                    q = np.zeros((n, N_CHOICE, 4))
                    q[:, rows, :b] = reach[d][:, :, None] * u
                    g = np.arange(self.depth_off[d], self.depth_off[d + 1])
                    acc = self.reduce_rows(q.reshape(n * N_CHOICE, 4), g)
                    best, vb = np.zeros(len(g), np.int64), acc[:, 0].copy()
                    for c in range(1, b):
                        better = acc[:, c] > vb
                        best, vb = np.where(better, c, best), np.where(better, acc[:, c], vb)
                    choice[g] = best
                    val = np.take_along_axis(u, choice[self.map[:, rows]][:, :, None], 2)[:, :, 0]
                else:
                    row = P[:, rows, :b]
                    v = np.zeros((n, u.shape[1]))
                    for c in range(b):
                        v = v + row[:, :, c] * u[:, :, c]
                    val = v
        return val[:, 0].copy(), choice

    def exploitability(self, pol):
        """-> (out4, [br table of team 0, of team 1] as complete [G][4] tables)"""
        v0, c0 = self.value_pass(pol, 0)
        v1, c1 = self.value_pass(pol, 1)
        v, _ = self.value_pass(pol, None)
        brs = []
        for p, ch in ((0, c0), (1, c1)):
            t = pol.copy()
            m = self.team == p
            t[m] = (np.arange(4)[None, :] == ch[m][:, None]).astype(np.float64)
            brs.append(t)
        b0, b1 = self.mean(v0), self.mean(v1)
        return np.array([(b0 + b1) / 2.0, b0, b1, self.mean(v)]), brs, v

    def policy_for_deal(self, pol, deal):
        return pol[self.map[deal]]
