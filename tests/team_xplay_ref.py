"""Float64 numpy restatement of policy against policy on Team MiniScopa (scopa_team_xplay.hip): the leaf scopas, the exact four-quantity cross-play
per deal and its deal-order mean, the sampled seat-swapped match.  Built on tests/team_chance_ref.py's ChanceRef (its map and r2) and
tests/team_cfr_ref.py.

TEST INFRASTRUCTURE, written for this repository's tests.  Every float64 operation is one numpy elementwise operation (one rounding, no fused
multiply-add), in the kernels' documented order:

  leaves      per depth-12 node, after its four forced plies: 0.5 * r2, 0.25 * r2 * r2, scopas of team 0's two seats, of team 1's two seats
  follow      per (deal, a, b), depth 11 up: table a's rows at team 0's depths and table b's at team 1's, through the deal's map row (or the local row
              itself on one deal); per node and quantity v = 0.0; v += row[c] * child[c], c = 0 .. b - 1 -- rows as given, the padding never read
  mean        s = img[0]; s += img[1]; ... in deal order, then s / float(n)
  match       episode i: deal = (x0 * n) >> 32 of Philox counter (i, i >> 32, 44, stream) (the chance form only); ply d at counter
              (i, i >> 32, 32 + d, stream); N = (x0 >> 5) << 26 | x1 >> 6; thr[k] = ceil(cdf_k / cdf_last * 2^53), 0 where the quotient is <= 0, 2^53
              where it is >= 1 or NaN; action = #{k < b - 1 : thr[k] <= N}; episodes i < n_team0 have a as team 0
"""
import ctypes as C

import numpy as np

import oracle as O
import philox_words as W
import team_chance_ref as TC
import team_chance_sets as TS
from team_cfr_ref import N_CHOICE, N_LEAVES, OFFSET, WIDTH, branch, team_of
from team_mccfr_ref import philox4x32_10

PLY_TAG, DEAL_TAG = 32, 44
_SCOPAS = {}


# ---- leaf scopas --------------------------------------------------------------------------------------------------------------------------
def leaf_scopas_enum(perm, first=0, count=N_LEAVES):
    """uint8 [count]: the scopa byte (team 0 low nibble, team 1 high nibble) of the depth-12 nodes first .. first + count - 1, enumerated through the
    oracle's TeamState as team_cfr_ref.leaves enumerates r2: the path's legal-action indices, then the four forced plies"""
    L = O.lib()
    buf = (C.c_int * 4)()
    out = np.zeros(count, np.uint8)
    for k in range(count):
        idx, digits = first + k, []
        for d in range(11, -1, -1):
            digits.append(idx % branch(d))
            idx //= branch(d)
        s = O.TeamState(perm=np.ascontiguousarray(perm, np.uint8)).s
        for c in reversed(digits):
            L.ogt_legal(C.byref(s), buf)
            L.ogt_step(C.byref(s), buf[c])
        for _ in range(4):
            L.ogt_legal(C.byref(s), buf)
            L.ogt_step(C.byref(s), buf[0])
        assert s.terminal
        out[k] = (int(s.scopas[0]) + int(s.scopas[1])) | ((int(s.scopas[2]) + int(s.scopas[3])) << 4)
    return out


def leaf_scopas(perm):
    """uint8 [331776]: the scopa byte of every depth-12 node, by team_chance_ref.walk's level-wise walk -- every distinct (table, card) transition is
    the oracle's step, asked once (held equal to leaf_scopas_enum by tests/test_team_xplay_ref.py)"""
    kb = bytes(np.ascontiguousarray(perm, np.uint8))
    if kb in _SCOPAS:
        return _SCOPAS[kb]
    u = np.uint64
    p = np.frombuffer(kb, np.uint8).astype(np.uint64)
    hands = [np.array([p[4 * s] | p[4 * s + 1] << u(4) | p[4 * s + 2] << u(8) | p[4 * s + 3] << u(12)], np.uint64) for s in range(4)]
    tab, nt, sc = np.zeros(1, np.uint64), np.zeros(1, np.int64), [np.zeros(1, np.int64), np.zeros(1, np.int64)]
    for d in range(16):
        seat, b = d & 3, branch(d) if d < 12 else 1
        c = np.arange(b, dtype=np.uint64)[None, :]
        h = hands[seat][:, None]
        card = (h >> (u(4) * c)) & u(15)
        left = (h & ((u(1) << (u(4) * c)) - u(1))) | ((h >> (u(4) * c + u(4))) << (u(4) * c))
        rep = lambda a: np.repeat(a, b)
        combo = rep(tab) | rep(nt).astype(np.uint64) << u(32) | card.reshape(-1) << u(36)
        uq, inv = np.unique(combo, return_inverse=True)
        for x in uq.tolist():
            if x not in TC._TRANSITIONS:
                TC._TRANSITIONS[x] = TC._transition(x & 0xFFFFFFFF, (x >> 32) & 15, x >> 36)
        r = np.array([TC._TRANSITIONS[x] for x in uq.tolist()], np.int64).reshape(-1, 4)[inv.reshape(-1)]
        hands = [left.reshape(-1) if s == seat else rep(hands[s]) for s in range(4)]
        tab, nt = r[:, 0].astype(np.uint64), r[:, 1]
        sc = [rep(sc[t]) + (r[:, 3] if t == seat >> 1 else 0) for t in (0, 1)]
    assert sc[0].shape == (N_LEAVES,) and int(sc[0].max()) < 16 and int(sc[1].max()) < 16
    out = (sc[0] | (sc[1] << 4)).astype(np.uint8)
    out.setflags(write=False)
    _SCOPAS[kb] = out
    return out


def leaf_quads(r2, sc):
    """[leaves][4] float64 from the int payoffs and the scopa bytes"""
    r2 = np.asarray(r2, np.int64)
    sc = np.asarray(sc, np.int64)
    return np.stack([0.5 * r2.astype(np.float64), 0.25 * (r2 * r2).astype(np.float64), (sc & 15).astype(np.float64), (sc >> 4).astype(np.float64)], 1)


# ---- the follow pass ---------------------------------------------------------------------------------------------------------------------------
def follow(quads, rows_a, rows_b, read_padding=False):
    """the root's four quantities: quads [331776][4]; rows_a / rows_b [321365][4] the two tables in the deal's LOCAL row order.
    read_padding: the wrong pass that adds all four slots of every row (the guard that the padding of the test tables matters)"""
    val = quads
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for d in range(11, -1, -1):
            b = branch(d)
            row = (rows_a if team_of(d) == 0 else rows_b)[OFFSET[d]:OFFSET[d] + WIDTH[d]]
            u = val.reshape(-1, b, 4)
            v = np.zeros((u.shape[0], 4))
            for c in range(b):
                v = v + row[:, c, None] * u[:, c, :]
            if read_padding:
                for c in range(b, 4):
                    v = v + row[:, c, None] * u[:, 0, :]
            val = v
    return val[0].copy()


def deal_mean(img, order=None):
    """s = img[0]; s += img[1]; ...; s / n over the leading axis (order: another summation order, for the guard)"""
    order = range(img.shape[0]) if order is None else order
    with np.errstate(invalid="ignore", over="ignore"):
        s = None
        for k in order:
            s = img[k].copy() if s is None else s + img[k]
        return s / float(img.shape[0])


# ---- thresholds and the match ------------------------------------------------------------------------------------------------------------------
TWO53 = 9007199254740992.0


def thresholds(rows, b):
    """uint64 [m][b - 1] of rows [m][>= b]: scopa_tree_passes.h's policy_thresholds"""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        c = rows[:, 0].copy()
        cdf = [c]
        for q in range(1, b):
            c = c + rows[:, q]
            cdf.append(c)
        out = np.zeros((rows.shape[0], b - 1), np.uint64)
        for k in range(b - 1):
            x = cdf[k] / cdf[b - 1]
            mid = (x > 0.0) & (x < 1.0)
            t = np.full(rows.shape[0], 1 << 53, np.uint64)
            t[x <= 0.0] = 0
            t[mid] = np.ceil(x[mid] * TWO53).astype(np.uint64)
            out[:, k] = t
    return out


class Match:
    """what a match over deals leaves: per-episode deal and leaf, the ten sums"""

    def __init__(self, deal, leaf, stats):
        self.deal, self.leaf, self.stats = deal, leaf, stats


def sums_of(leaf_r2, leaf_sc, n_team0):
    """int64 [2][5] from every episode's r2 of team 0 and scopa byte"""
    st = np.zeros((2, 5), np.int64)
    r2, sc = np.asarray(leaf_r2, np.int64), np.asarray(leaf_sc, np.int64)
    for half, sl in ((0, slice(0, n_team0)), (1, slice(n_team0, None))):
        mine = r2[sl] if half == 0 else -r2[sl]
        s0, s1 = sc[sl] & 15, sc[sl] >> 4
        st[half] = [mine.shape[0], mine.sum(), (mine * mine).sum(), (s0 if half == 0 else s1).sum(), (s1 if half == 0 else s0).sum()]
    return st


def match(maps, r2, sc, pol_a, pol_b, n, n_team0, seed, stream, draw_deal=True):
    """maps int [n_deals][321365] (None: one deal, local rows are table rows), r2 / sc [n_deals][331776] -> Match"""
    n_deals = r2.shape[0]
    i = np.arange(n, dtype=np.uint64)
    lo, hi = i & np.uint64(W.M32), i >> np.uint64(32)
    if draw_deal:
        x = philox4x32_10(lo, hi, np.uint64(DEAL_TAG), np.uint64(stream), int(seed))
        deal = ((x[0] * np.uint64(n_deals)) >> np.uint64(32)).astype(np.int64)
    else:
        deal = np.zeros(n, np.int64)
    a_team = (np.arange(n) >= n_team0).astype(np.int64)
    idx = np.zeros(n, np.int64)
    for d in range(12):
        b = branch(d)
        x = philox4x32_10(lo, hi, np.uint64(PLY_TAG + d), np.uint64(stream), int(seed))
        N = ((x[0] >> np.uint64(5)) << np.uint64(26)) | (x[1] >> np.uint64(6))
        local = OFFSET[d] + idx
        at = local if maps is None else maps[deal, local].astype(np.int64)
        rows = np.where((a_team == team_of(d))[:, None], pol_a[at], pol_b[at])
        thr = thresholds(rows, b)
        idx = idx * b + (thr <= N[:, None]).sum(1)
    return Match(deal, idx, sums_of(r2[deal, idx], sc[deal, idx], n_team0))


# ---- a set of deals ----------------------------------------------------------------------------------------------------------------------------
class XRef:
    """cross-play and matches on the deals of a ChanceRef (tables [G][4]); XRef.one(perm) is one deal with tables in its local row order"""

    def __init__(self, cr, own_rows=False):
        self.cr, self.n = cr, cr.n
        self.maps = None if own_rows else cr.map
        self.r2 = np.asarray(cr.r2, np.int64).reshape(cr.n, N_LEAVES)
        self.sc = np.stack([leaf_scopas(p) for p in cr.perms])
        self.quads = [leaf_quads(self.r2[k], self.sc[k]) for k in range(cr.n)]

    @classmethod
    def one(cls, perm):
        assert np.asarray(perm).size == 16
        return TS.cached(("xone", bytes(np.ascontiguousarray(perm, np.uint8))), lambda: cls(_OneDeal(perm), own_rows=True))

    def local(self, pol, deal):
        return pol if self.maps is None else pol[self.maps[deal]]

    def per_deal(self, policies, read_padding=False):
        """[n][K][K][4]"""
        K = len(policies)
        out = np.zeros((self.n, K, K, 4))
        for k in range(self.n):
            loc = [self.local(np.asarray(p, np.float64), k) for p in policies]
            for a in range(K):
                for b in range(K):
                    out[k, a, b] = follow(self.quads[k], loc[a], loc[b], read_padding)
        return out

    def cross_play(self, policies):
        """-> (out [K][K][4], per_deal [n][K][K][4])"""
        img = self.per_deal(policies)
        return (deal_mean(img) if self.maps is not None else img[0]), img

    def match(self, pol_a, pol_b, n, n_team0, seed, stream):
        return match(self.maps, self.r2, self.sc, np.asarray(pol_a, np.float64), np.asarray(pol_b, np.float64), n, n_team0, seed, stream, draw_deal=self.maps is not None)


class _OneDeal:
    """the parts of a ChanceRef an XRef with own rows reads, for one deal"""

    def __init__(self, perm):
        self.perms = np.ascontiguousarray(perm, np.uint8).reshape(1, 16)
        self.n = 1
        self.r2 = TC.walk(self.perms[0])[1].astype(np.int64).reshape(1, N_LEAVES)


def xref(name):
    return TS.cached(("xref", name), lambda: XRef(TS.chance_ref(name)))


# ---- the test tables -----------------------------------------------------------------------------------------------------------------------------
def adversarial(cr, seed=7):
    """[G][4]: positive unnormalised rows, non-zero garbage in the padding slots, every 11th row all-zero in its legal slots"""
    rng = np.random.default_rng(seed)
    t = rng.uniform(0.05, 3.0, (cr.G, 4))
    pad = np.arange(4)[None, :] >= cr.nleg[:, None]
    t[pad] = rng.uniform(-9.0, 9.0, int(pad.sum())) + 20.0
    zero = (np.arange(cr.G) % 11 == 3)[:, None] & ~pad
    t[zero] = 0.0
    return t


def tables(name):
    """{"uniform", "cfr", "br0", "adv"} of a deal set, read-only: (i) uniform, (ii) the average policy after 3 CFR+ iterations, (iii) team 0's best
    response table to (ii) with the BR0 value and the per-deal values ChanceRef.exploitability reports, (iv) the adversarial table"""
    def make():
        cr = TS.chance_ref(name)
        uni = np.where(np.arange(4)[None, :] < cr.nleg[:, None], 1.0 / cr.nleg[:, None], 0.0)
        cfr = cr.average_policy(TS.ref_run(name, "cfr+")[1])
        out4, brs, per_deal_value = cr.exploitability(cfr)
        out = {"uniform": uni, "cfr": cfr, "br0": brs[0], "adv": adversarial(cr), "cfr_out4": out4, "cfr_value_per_deal": per_deal_value}
        for a in out.values():
            a.setflags(write=False)
        return out
    return TS.cached(("xtables", name), make)


def normalised(cr, table):
    """the rows a match plays from `table`: legal slots / their left-to-right sum, slot 0 where that sum is not > 0; padding 0"""
    legal = np.arange(4)[None, :] < cr.nleg[:, None]
    x = np.where(legal, table, 0.0)
    s = x[:, 0] + x[:, 1] + x[:, 2] + x[:, 3]
    out = np.where(s[:, None] > 0, x / np.where(s > 0, s, 1.0)[:, None], 0.0)
    out[~(s > 0), 0] = 1.0
    return out


STACK = ("cfr", "br0", "adv")          # the K = 3 of the bit-for-bit tests


def stack(name):
    t = tables(name)
    return [t[k] for k in STACK]


def reference(name):
    """(out [3][3][4], per_deal [n][3][3][4]) of STACK on a deal set, computed once"""
    return TS.cached(("xcross", name), lambda: xref(name).cross_play(stack(name)))


# the match cases of tests/test_gpu_team_xplay.py, guarded by tests/test_team_xplay_ref.py: (seed, stream id)
MATCH_N, MATCH_TEAM0 = 4099, 1501
MATCH_CASES = [(0x5C09A, 16), (W.WIDE_SEED, 16), (0x5C09A, W.ITER_B31), (0x5C09A, W.ITER_HI), (W.WIDE_SEED, W.ITER_HI)]
LONG_N, LONG_SEED, LONG_STREAM = 65536, 0x5C09A, 21


def standard_error_check(stats, exact, n_team0, n):
    """per seat half: (mean reward of a, its exact target, the standard error from the exact second moment); exact = cross-play [2][2][4] of (a, b)"""
    out = []
    for half, (cell, sign, m) in enumerate((((0, 1), 1.0, n_team0), ((1, 0), -1.0, n - n_team0))):
        mean = 0.5 * float(stats[half, 1]) / m
        target = sign * float(exact[cell][0])
        var = float(exact[cell][1]) - float(exact[cell][0]) ** 2
        out.append((mean, target, (max(var, 0.0) / m) ** 0.5))
    return out
