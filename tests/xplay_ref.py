"""Float64 restatement of the policy-against-policy kernels (scopa_amd/csrc/scopa_xplay.hip) over oracle.Tree's exported arrays.

TEST INFRASTRUCTURE, written for this repository's tests: the GPU kernels are held to it bit for bit, and it is itself anchored to the C oracle
(tests/test_xplay_ref.py: Tree.policy_value, Tree.exploitability).  Every float64 operation is one numpy elementwise operation (one rounding, no
fused multiply-add), in the kernels' order:
  cross          terminals 0.5 * p0, 0.25 * p0 * p0 and the two scopa counts; eight levels bottom up, `v = 0.0; v += row[c] * child[c]`, children
                 left to right; the row is P0's at player-0 infosets and P1's at player-1 infosets, used as given
  best_response  k_exploitability's procedure: reach of everyone but the responder top down; per (infoset, action) cell the ply's nodes added in
                 ascending order from 0.0; argmax by a strict `>` (ties to the lowest action); the other player's plies as in cross
  sampling       thresholds ceil(cdf_k / cdf_last * 2^53) and the draw N = (x0 >> 5) << 26 | (x1 >> 6) of Philox (episode, ply, stream; seed):
                 action = #{k : thr[k] <= N}, clamped to the last legal one; an episode is a walk over the tree's level-order node indices
Tree nodes are in DFS preorder: ascending index within a ply is the device's level order (children of node j of a ply are j * n + c).
"""
import numpy as np

N_PLIES = 8
TWO53 = 9007199254740992


class Ref:
    def __init__(self, tree):
        t = self.tree = tree
        self.I = t.n_infosets
        self.nlegal = t.infoset_nlegal.astype(np.int64)
        self.player = t.infoset_player.astype(np.int64)
        self.levels = []
        for d in range(N_PLIES):
            nodes = np.flatnonzero((t.depth == d) & (t.term == 0))
            n, p = int(t.nlegal[nodes[0]]), int(t.player[nodes[0]])
            assert (t.nlegal[nodes] == n).all() and (t.player[nodes] == p).all() and p == d % 2 and n == 4 - d // 2
            inf = t.infoset[nodes].astype(np.int64)
            assert (self.nlegal[inf] == n).all() and (self.player[inf] == p).all()
            seen, rank = {}, np.zeros(nodes.size, np.int64)
            for j, i in enumerate(inf):                  # rank of a node among its infoset's nodes, in ply order
                rank[j] = seen.get(i, 0)
                seen[i] = rank[j] + 1
            groups = [np.flatnonzero(rank == k) for k in range(rank.max() + 1)]      # within a group every infoset appears once
            self.levels.append(dict(nodes=nodes, n=n, p=p, inf=inf, child=t.child[nodes, :n].astype(np.int64), groups=groups,
                                    rows=np.array(sorted(seen), np.int64)))
        self.term_nodes = np.flatnonzero(t.term != 0)
        assert (t.depth[self.term_nodes] == N_PLIES).all() and self.term_nodes.size == 576
        for d, lv in enumerate(self.levels):             # level order: the children of node j are nodes j * n + c of the next level
            nxt = self.levels[d + 1]["nodes"] if d + 1 < N_PLIES else self.term_nodes
            assert np.array_equal(lv["child"].reshape(-1), nxt)
        assert sorted(np.concatenate([lv["rows"] for lv in self.levels]).tolist()) == list(range(self.I))   # an infoset lives in one ply
        p0 = t.r2[self.term_nodes, 0].astype(np.float64)
        self.term_p0 = p0
        self.term_r2 = t.r2[self.term_nodes].astype(np.int64)                                  # rewards x2 of either seat
        self.term_scopas = t.states()["scopas"][self.term_nodes].astype(np.int64)              # [576][2]
        self.term_q = np.stack([0.5 * p0, 0.25 * p0 * p0, self.term_scopas[:, 0].astype(np.float64), self.term_scopas[:, 1].astype(np.float64)])

    # ---- cross-play -----------------------------------------------------------------------------------------------------------------
    def combined(self, P0, P1):
        return np.where((self.player == 0)[:, None], np.asarray(P0, np.float64), np.asarray(P1, np.float64))

    def cross(self, P0, P1):
        """-> float64 [4]: E[reward of seat 0], E[its square], E[scopas of seat 0], E[scopas of seat 1] of P0 in seat 0 against P1 in seat 1"""
        pol = self.combined(P0, P1)
        val = np.zeros((4, self.tree.n_nodes))
        val[:, self.term_nodes] = self.term_q
        with np.errstate(invalid="ignore", over="ignore"):
            for lv in reversed(self.levels):
                v = np.zeros((4, lv["nodes"].size))
                for c in range(lv["n"]):
                    v = v + pol[lv["inf"], c][None, :] * val[:, lv["child"][:, c]]
                val[:, lv["nodes"]] = v
        return val[:, 0].copy()

    # ---- best response --------------------------------------------------------------------------------------------------------------
    def _br_pass(self, P, br):
        """pass `br` of k_exploitability (2 = nobody responds) -> (root value for the responder / for player 0, choice [I] int64)"""
        t = self.tree
        reach, val = np.zeros(t.n_nodes), np.zeros(t.n_nodes)
        choice = np.zeros(self.I, np.int64)
        reach[0] = 1.0
        with np.errstate(invalid="ignore", over="ignore"):
            for lv in self.levels:
                for c in range(lv["n"]):
                    r = reach[lv["nodes"]]
                    reach[lv["child"][:, c]] = r if lv["p"] == br else r * P[lv["inf"], c]
            p0 = self.term_r2[:, 0]
            val[self.term_nodes] = 0.5 * (-p0 if br == 1 else p0).astype(np.float64)      # negated as an integer: a drawn terminal is +0.0 for both
            for lv in reversed(self.levels):
                nodes, inf, n = lv["nodes"], lv["inf"], lv["n"]
                if lv["p"] == br:
                    q = np.zeros((self.I, 4))
                    for c in range(n):
                        term = reach[nodes] * val[lv["child"][:, c]]
                        for g in lv["groups"]:
                            q[inf[g], c] = q[inf[g], c] + term[g]
                    rows = lv["rows"]
                    best = np.zeros(rows.size, np.int64)
                    for c in range(1, n):
                        best = np.where(q[rows, c] > q[rows, best], c, best)
                    choice[rows] = best
                    val[nodes] = val[lv["child"][np.arange(nodes.size), choice[inf]]]
                else:
                    v = np.zeros(nodes.size)
                    for c in range(n):
                        v = v + P[inf, c] * val[lv["child"][:, c]]
                    val[nodes] = v
        return val[0], choice

    def best_response(self, P):
        """-> (out4 = [(BR0 + BR1) / 2, BR0, BR1, value], (br0, br1)): br_p is P with player p's rows one-hot at the chosen action"""
        P = np.ascontiguousarray(P, np.float64)
        out4, tables = np.zeros(4), []
        for br in (0, 1):
            out4[1 + br], choice = self._br_pass(P, br)
            onehot = (np.arange(4)[None, :] == choice[:, None]).astype(np.float64)
            tables.append(np.where((self.player == br)[:, None], onehot, P))
        out4[3], _ = self._br_pass(P, 2)
        out4[0] = 0.5 * (out4[1] + out4[2])
        return out4, tuple(tables)

    # ---- sampling -------------------------------------------------------------------------------------------------------------------
    def thresholds(self, P):
        """uint64 [I][3]: k_eval_thresholds' rows -- 2^53 (never counted) beyond n - 2 and where the quotient is >= 1 or NaN, 0 where it is <= 0"""
        P = np.asarray(P, np.float64)
        thr = np.full((self.I, 3), TWO53, np.uint64)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            for r in range(self.I):
                n = int(self.nlegal[r])
                cdf, c = [], 0.0
                for k in range(n):
                    c = P[r, k] if k == 0 else c + P[r, k]
                    cdf.append(c)
                for k in range(n - 1):
                    x = np.float64(cdf[k]) / np.float64(cdf[n - 1])
                    if x <= 0.0:
                        thr[r, k] = 0
                    elif x < 1.0:
                        thr[r, k] = int(np.ceil(x * np.float64(TWO53)))
        return thr

    def episodes(self, oracle, thr_seat0, thr_seat1, episodes, stream_id, seed):
        """terminal index (level order within ply 8) of each episode in `episodes`: seat s samples by thr_seat{s}"""
        key = [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF]
        thr = (thr_seat0, thr_seat1)
        out = np.zeros(len(episodes), np.int64)
        for e, i in enumerate(episodes):
            idx = 0
            for ply in range(6):                         # plies 6 and 7 have one legal card and draw nothing
                lv = self.levels[ply]
                x = oracle.philox4x32_10([i & 0xFFFFFFFF, i >> 32, ply, stream_id], key)
                N = ((int(x[0]) >> 5) << 26) | (int(x[1]) >> 6)
                row = thr[ply & 1][lv["inf"][idx]]
                a = sum(int(row[k]) <= N for k in range(3))
                idx = idx * lv["n"] + min(a, lv["n"] - 1)
            out[e] = idx
        return out

    def match_stats(self, idx, seat):
        """the integer sums scopa_eval_pair_match reports for episodes with terminal indices idx, the policy of interest in `seat`"""
        r2 = self.term_r2[idx]
        mine = r2[:, seat]
        sc = self.term_scopas[idx]
        return [int(idx.size), int(mine.sum()), int((mine * mine).sum()), int(sc[:, seat].sum()), int(sc[:, 1 - seat].sum())]


def policy_set(tree, seed=2024):
    """The tests' tables for one deal, [n_infosets][4] float64 with zeros in the illegal slots: uniform; the average policy after five unit-weight
    synchronous sweeps; a seeded Dirichlet table; one with zero entries in legal slots (every second row loses its first legal action where it has
    two or more, renormalised); two random one-hot tables."""
    rng = np.random.default_rng(seed)
    n = tree.infoset_nlegal.astype(np.int64)
    legal = np.arange(4)[None, :] < n[:, None]
    uniform = np.where(legal, 1.0 / n[:, None].astype(np.float64), 0.0)
    R, S, _ = tree.tables()
    tree.cfr_sync(R, S, 5)
    average = tree.average_policy(S)
    g = np.where(legal, rng.gamma(0.7, size=(n.size, 4)), 0.0)
    dirichlet = g / g.sum(1, keepdims=True)
    z = np.where(legal, rng.gamma(1.0, size=(n.size, 4)), 0.0)
    z[(np.arange(n.size) % 2 == 0) & (n >= 2), 0] = 0.0
    zeros = z / z.sum(1, keepdims=True)
    onehots = [(np.arange(4)[None, :] == rng.integers(0, n)[:, None]).astype(np.float64) for _ in range(2)]
    return {"uniform": uniform, "average": average, "dirichlet": dirichlet, "zeros": zeros, "onehot_a": onehots[0], "onehot_b": onehots[1]}
