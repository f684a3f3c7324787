"""Float64 restatement of policy against policy on the chance game (scopa_amd/csrc/scopa_chance_xplay.hip), composed from what exists: per deal
xplay_ref.Ref's cross, thresholds, episodes and match_stats; across deals chance_ref.ChanceRef's map, reduce and exploitability passes.

TEST INFRASTRUCTURE, written for this repository's tests: the GPU kernels are held to it bit for bit (tests/test_gpu_chance_xplay.py) and it is
itself anchored to ChanceRef.exploitability (tests/test_chance_xplay_ref.py).  Every float64 operation is one numpy operation (one rounding):
  cross-play     per deal Ref.cross of the two tables in the deal's local order; the mean s = v[0]; s = s + v[1]; ... in deal order, then s / n
  best response  ChanceRef.exploitability's passes statement for statement, keeping `best` of every responder ply and scattering it into tables:
                 player p's rows one-hot at the chosen action, the other player's rows the policy's
  match          episode i draws deal = (x0 * n) >> 32 from the first Philox word of counter (i, i >> 32, 8, stream) -- eval_ref's Philox -- and then
                 is Ref.episodes' walk on that deal under the deal's local thresholds
"""
import numpy as np

import eval_ref
from chance_ref import ChanceRef
from xplay_ref import Ref as XRef

DEAL_TAG = 8


def _perm(h0, h1):
    return h0 + h1 + [c for c in range(16) if c not in h0 + h1]


# the six-deal set of tests/test_gpu_chance.py (copied: test files are not imported)
SIX = np.array([_perm([0, 5, 10, 15], h) for h in ([1, 2, 3, 4], [1, 2, 3, 6], [1, 2, 7, 6], [9, 8, 7, 6])] +
               [_perm([0, 5, 10, 14], h) for h in ([1, 2, 3, 4], [9, 8, 7, 6])], np.uint8)


class ChanceXRef:
    def __init__(self, chance_ref):
        self.c = chance_ref
        self.n, self.G = chance_ref.n, chance_ref.G
        self.x = [XRef(t) for t in chance_ref.trees]

    def local(self, P, d):
        """the global table P [G][4] in deal d's local order: what scopa_chance_policy_for_deal scatters"""
        return np.asarray(P, np.float64)[self.c.map[d, :self.c.I[d]]]

    # ---- cross-play -----------------------------------------------------------------------------------------------------------------
    def cross_per_deal(self, pols):
        """-> [n][K][K][4]: Ref.cross per deal and ordered pair"""
        loc = [[self.local(P, d) for P in pols] for d in range(self.n)]
        return np.array([[[self.x[d].cross(a, b) for b in loc[d]] for a in loc[d]] for d in range(self.n)])

    def mean(self, per_deal):
        with np.errstate(invalid="ignore", over="ignore"):
            s = per_deal[0].copy()
            for d in range(1, self.n):
                s = s + per_deal[d]
            return s / float(self.n)

    def cross(self, pols):
        """-> (per_deal [n][K][K][4], out [K][K][4])"""
        per = self.cross_per_deal(pols)
        return per, self.mean(per)

    # ---- best response --------------------------------------------------------------------------------------------------------------
    def best_response(self, P):
        """ChanceRef.exploitability(P) with the choices kept -> (out4, (br0, br1))"""
        c = self.c
        P = np.ascontiguousarray(P, np.float64)
        out, tables = np.zeros(4), []
        with np.errstate(invalid="ignore", over="ignore"):
            for br in range(3):
                choice = np.zeros(c.G, np.int64)
                reach = [np.zeros(t.n_nodes) for t in c.trees]
                val = [np.zeros(t.n_nodes) for t in c.trees]
                for d, ref in enumerate(c.refs):
                    reach[d][0] = 1.0
                    for lv in ref.levels:
                        g = c.map[d, lv["inf"]]
                        for a in range(lv["n"]):
                            ch = lv["child"][:, a]
                            reach[d][ch] = reach[d][lv["nodes"]] if lv["p"] == br else reach[d][lv["nodes"]] * P[g, a]
                    val[d][ref.term_nodes] = -ref.term_val if br == 1 else ref.term_val
                for depth in range(7, -1, -1):
                    n, p = 4 - depth // 2, depth & 1
                    if p == br:
                        qs = []
                        for d, ref in enumerate(c.refs):
                            lv = ref.levels[depth]
                            q = np.zeros((ref.I, 4))
                            for a in range(n):
                                term = reach[d][lv["nodes"]] * val[d][lv["child"][:, a]]
                                for grp in lv["groups"]:
                                    q[lv["inf"][grp], a] = q[lv["inf"][grp], a] + term[grp]
                            qs.append(q)
                        Q = c.reduce(qs)
                        best = np.zeros(c.G, np.int64)
                        rows = np.arange(c.G)
                        for a in range(1, n):
                            best = np.where(Q[rows, a] > Q[rows, best], a, best)
                        mine = c.ply == depth
                        choice[mine] = best[mine]
                        for d, ref in enumerate(c.refs):
                            lv = ref.levels[depth]
                            val[d][lv["nodes"]] = val[d][lv["child"][np.arange(lv["nodes"].size), best[c.map[d, lv["inf"]]]]]
                    else:
                        for d, ref in enumerate(c.refs):
                            lv = ref.levels[depth]
                            g = c.map[d, lv["inf"]]
                            v = np.zeros(lv["nodes"].size)
                            for a in range(n):
                                v = v + P[g, a] * val[d][lv["child"][:, a]]
                            val[d][lv["nodes"]] = v
                s = val[0][0]
                for d in range(1, c.n):
                    s = s + val[d][0]
                out[1 + br] = s / float(c.n)
                if br < 2:
                    onehot = (np.arange(4)[None, :] == choice[:, None]).astype(np.float64)
                    tables.append(np.where((c.player == br)[:, None], onehot, P))
        out[0] = 0.5 * (out[1] + out[2])
        return out, tuple(tables)

    # ---- the match ------------------------------------------------------------------------------------------------------------------
    def deals(self, episodes, stream_id, seed):
        """the deal every episode draws: (x0 * n) >> 32 of Philox (i, i >> 32, 8, stream_id; seed)"""
        out = np.zeros(len(episodes), np.int64)
        for e, i in enumerate(episodes):
            eval_ref.draw(int(i), DEAL_TAG, stream_id, seed)
            out[e] = (int(eval_ref._out[0]) * self.n) >> 32
        return out

    def thresholds(self, P):
        """per deal the local threshold rows of the global table P"""
        return [self.x[d].thresholds(self.local(P, d)) for d in range(self.n)]

    def match(self, oracle, A, B, n, n_seat0, stream_id, seed):
        """-> (deal [n], terminal index [n], stats int64 [2][5] from A's point of view)"""
        ta, tb = self.thresholds(A), self.thresholds(B)
        deal = self.deals(range(n), stream_id, seed)
        idx = np.zeros(n, np.int64)
        stats = np.zeros((2, 5), np.int64)
        eps = np.arange(n)
        for d in range(self.n):
            for half, sel in enumerate((eps < n_seat0, eps >= n_seat0)):
                mine = np.flatnonzero((deal == d) & sel)
                seats = (ta[d], tb[d]) if half == 0 else (tb[d], ta[d])
                idx[mine] = self.x[d].episodes(oracle, seats[0], seats[1], [int(i) for i in mine], stream_id, seed)
                stats[half] += np.array(self.x[d].match_stats(idx[mine], half), np.int64)
        return deal, idx, stats


# ---- the six-deal case shared by the CPU and the GPU tests: built once per process, never modified ------------------------------------------
MATCH_N, MATCH_SEAT0, MATCH_STREAM, MATCH_SEED = 20001, 10001, 16, 0x5C09A


def six(oracle, _cache={}):
    """-> dict(cref, xref, pols [4][G][4] = uniform, solved (20 DCFR iterations), Dirichlet (fixed seed), one-hot; names)"""
    if not _cache:
        from scopa_amd.algorithms import schedule
        c = ChanceRef([oracle.Tree(perm=p) for p in SIX])
        x = ChanceXRef(c)
        rng = np.random.default_rng(2025)
        uniform = np.where(c.legal, 1.0 / c.nlegal[:, None].astype(np.float64), 0.0)
        R, S = c.tables()
        c.run(R, S, schedule("dcfr", 0, 20, 1.5, 0.0, 2.0))
        solved = c.average_policy(S)
        gam = np.where(c.legal, rng.gamma(0.7, size=(c.G, 4)), 0.0)
        dirichlet = gam / gam.sum(1, keepdims=True)
        onehot = (np.arange(4)[None, :] == rng.integers(0, c.nlegal)[:, None]).astype(np.float64)
        pols = np.stack([uniform, solved, dirichlet, onehot])
        pols.setflags(write=False)
        _cache.update(cref=c, xref=x, pols=pols, names=("uniform", "solved", "dirichlet", "onehot"))
    return _cache


def six_cross(oracle, _cache={}):
    """the reference's (per_deal [6][4][4][4], out [4][4][4]) of the four policies"""
    if not _cache:
        s = six(oracle)
        per, out = s["xref"].cross(s["pols"])
        for a in (per, out):
            a.setflags(write=False)
        _cache.update(per=per, out=out)
    return _cache["per"], _cache["out"]


def six_best(oracle, k, _cache={}):
    if k not in _cache:
        s = six(oracle)
        _cache[k] = s["xref"].best_response(s["pols"][k])
    return _cache[k]


def six_match(oracle, ia, ib, n=MATCH_N, n_seat0=MATCH_SEAT0, stream_id=MATCH_STREAM, seed=MATCH_SEED, _cache={}):
    key = (ia, ib, n, n_seat0, stream_id, seed)
    if key not in _cache:
        s = six(oracle)
        _cache[key] = s["xref"].match(oracle, s["pols"][ia], s["pols"][ib], n, n_seat0, stream_id, seed)
    return _cache[key]
