"""Float64 restatement of the chance game over a set of deals (scopa_chance_*: k_chance_sweep, k_chance_reduce and the cross-deal exploitability)
over oracle.Tree's exported arrays.

TEST INFRASTRUCTURE, written for this repository's tests: the GPU kernels are held to it with np.array_equal, and it is itself anchored to the C
oracle with one deal (tests/test_chance_ref.py).  Every float64 operation is one numpy elementwise operation (one rounding, no fused multiply-add),
in the kernels' order:
  index     global id = rank of the key among the distinct keys of all deals, ascending unsigned; map[n][1653] local -> global, -1 past a deal's
            count; per global id its occurrences in ascending (deal, local id) order
  sweep     per deal, cfr_variants_ref's sweep with the deal's sigma rows gathered through map: dR, dS per cell from 0.0, nodes ascending in a ply
  reduce    per cell the occurrences' increments in that order STARTING FROM THE FIRST occurrence's value, then R <- R + dR;
            R <- !(R <= 0) ? R * pos : R * neg;  S <- (S + dS) * strat; alternating: two sweeps, sweep p updates player p's rows, player 0 first
  exploitability   per responder: reach per deal; plies 7..0: on a responder ply q per deal (nodes ascending from 0.0), reduced over the occurrences
            from the first, argmax with ties to the lowest action, values selected; else sigma-weighted values (children left to right from 0.0);
            each figure (v_deal0 + v_deal1 + ...) / n in deal order
"""
import numpy as np

from cfr_variants_ref import Ref

N_DECISION = 1653


def tree_keys(t):
    """uint64 key per infoset of an oracle.Tree: bit 0 player | bits 1-3 hand size | bits 4-19 ordered hand | bits 20-23 table size | 24-55 table"""
    st = t.states()
    first = np.full(t.n_infosets, -1, np.int64)
    for node in np.flatnonzero(t.term == 0)[::-1]:
        first[t.infoset[node]] = node
    keys = np.zeros(t.n_infosets, np.uint64)
    for i, node in enumerate(first):
        p = int(t.infoset_player[i])
        nh, nt = int(st["nh"][node, p]), int(st["nt"][node])
        k = p | (nh << 1) | (nt << 20)
        for j in range(nh):
            k |= int(st["hands"][node, p, j]) << (4 + 4 * j)
        for j in range(nt):
            k |= int(st["table"][node, j]) << (24 + 4 * j)
        keys[i] = k
    return keys


class ChanceRef:
    def __init__(self, trees):
        self.trees, self.refs, self.n = list(trees), [Ref(t) for t in trees], len(trees)
        self.I = [t.n_infosets for t in self.trees]
        self.local_keys = [tree_keys(t) for t in self.trees]
        self.keys = np.unique(np.concatenate(self.local_keys))            # sorted ascending, unsigned
        self.G = self.keys.size
        self.n_occ = int(sum(self.I))
        self.map = np.full((self.n, N_DECISION), -1, np.int32)
        for d, k in enumerate(self.local_keys):
            self.map[d, :k.size] = np.searchsorted(self.keys, k)
        self.nlegal = ((self.keys >> np.uint64(1)) & np.uint64(7)).astype(np.int64)
        self.player = (self.keys & np.uint64(1)).astype(np.int64)
        self.ply = 2 * (4 - self.nlegal) + self.player
        self.legal = np.arange(4)[None, :] < self.nlegal[:, None]
        for d, ref in enumerate(self.refs):                              # every global row belongs to exactly one ply
            for depth, lv in enumerate(ref.levels):
                assert (self.ply[self.map[d, lv["rows"]]] == depth).all()
        # occurrences: flat id = start[deal] + local, ascending (deal, local) per global row; grouped by rank within the row
        self.start = np.concatenate([[0], np.cumsum(self.I)]).astype(np.int64)
        flat_g = np.concatenate([self.map[d, :self.I[d]] for d in range(self.n)]).astype(np.int64)
        self.count = np.bincount(flat_g, minlength=self.G)
        order = np.argsort(flat_g, kind="stable")                        # by global row, then ascending flat id = (deal, local)
        first = np.concatenate([[0], np.cumsum(self.count)])[:-1]
        rank = np.arange(flat_g.size) - np.repeat(first, self.count)
        self.occ_groups = [(flat_g[order[rank == k]], order[rank == k]) for k in range(int(self.count.max()))]   # (global rows, flat ids)

    def shared_hand_sizes(self, player):
        """hand sizes at which `player` has a row that occurs in more than one deal"""
        return sorted(set(self.nlegal[(self.count > 1) & (self.player == player)].tolist()))

    def tables(self):
        return np.zeros((self.G, 4)), np.zeros((self.G, 4))

    def sigma(self, R):
        with np.errstate(invalid="ignore", divide="ignore"):
            pos = np.where(self.legal, np.where(~(R <= 0.0), R, 0.0), 0.0)
            s = pos[:, 0].copy()
            for c in range(1, 4):
                s = np.where(c < self.nlegal, s + pos[:, c], s)
            uni = (1.0 / self.nlegal.astype(np.float64))[:, None]
            return np.where(self.legal, np.where((s > 0.0)[:, None], pos / s[:, None], uni), 0.0)

    def average_policy(self, S):
        with np.errstate(invalid="ignore", divide="ignore"):
            s = S[:, 0].copy()
            for c in range(1, 4):
                s = np.where(c < self.nlegal, s + S[:, c], s)
            uni = (1.0 / self.nlegal.astype(np.float64))[:, None]
            return np.where(self.legal, np.where((s > 0.0)[:, None], S / s[:, None], uni), 0.0)

    def reduce(self, per_deal):
        """[G][4] sums of the deals' [I_d][4] rows over each global row's occurrences, in order, from the first"""
        flat = np.concatenate(per_deal, 0)
        acc = np.zeros((self.G, 4))
        with np.errstate(invalid="ignore", over="ignore"):
            for k, (rows, ids) in enumerate(self.occ_groups):
                acc[rows] = flat[ids] if k == 0 else acc[rows] + flat[ids]
        return acc

    def deal_delta(self, d, sig, update):
        """the sweep of deal d under its local sigma rows -> dR, dS [I_d][4] (zero where nothing is summed)"""
        ref = self.refs[d]
        t = ref.tree
        r0, r1, val = np.zeros(t.n_nodes), np.zeros(t.n_nodes), np.zeros(t.n_nodes)
        r0[0] = r1[0] = 1.0
        dR, dS = np.zeros((ref.I, 4)), np.zeros((ref.I, 4))
        with np.errstate(invalid="ignore", over="ignore"):
            for lv in ref.levels:
                for a in range(lv["n"]):
                    c, sg = lv["child"][:, a], sig[lv["inf"], a]
                    r0[c] = r0[lv["nodes"]] * sg if lv["p"] == 0 else r0[lv["nodes"]]
                    r1[c] = r1[lv["nodes"]] * sg if lv["p"] == 1 else r1[lv["nodes"]]
            val[ref.term_nodes] = ref.term_val
            for lv in reversed(ref.levels):
                nodes, inf, p = lv["nodes"], lv["inf"], lv["p"]
                v = np.zeros(nodes.size)
                for a in range(lv["n"]):
                    v = v + sig[inf, a] * val[lv["child"][:, a]]
                val[nodes] = v
                if update is not None and update != p:
                    continue
                reach, opp, sgn = (r0[nodes], r1[nodes], 1.0) if p == 0 else (r1[nodes], r0[nodes], -1.0)
                for a in range(lv["n"]):
                    tR = opp * (sgn * (val[lv["child"][:, a]] - v))
                    tS = reach * sig[inf, a]
                    aR, aS = np.zeros(ref.I), np.zeros(ref.I)
                    for g in lv["groups"]:
                        aR[inf[g]] = aR[inf[g]] + tR[g]
                        aS[inf[g]] = aS[inf[g]] + tS[g]
                    dR[lv["rows"], a], dS[lv["rows"], a] = aR[lv["rows"]], aS[lv["rows"]]
        return dR, dS

    def sweep(self, R, S, w, update):
        w_pos, w_neg, w_strat = (float(x) for x in w)
        sig = self.sigma(R)
        deltas = [self.deal_delta(d, sig[self.map[d, :self.I[d]]], update) for d in range(self.n)]
        dR, dS = self.reduce([x[0] for x in deltas]), self.reduce([x[1] for x in deltas])
        cells = self.legal if update is None else self.legal & (self.player == update)[:, None]
        with np.errstate(invalid="ignore", over="ignore"):
            Rn = R + dR
            R[cells] = np.where(~(Rn <= 0.0), Rn * w_pos, Rn * w_neg)[cells]
            S[cells] = ((S + dS) * w_strat)[cells]

    def run(self, R, S, weights, alternating=False):
        """len(weights) iterations in place on R, S ([G][4] float64)"""
        for w in np.asarray(weights, np.float64).reshape(-1, 3):
            if alternating:
                self.sweep(R, S, w, 0)
                self.sweep(R, S, w, 1)
            else:
                self.sweep(R, S, w, None)
        return R, S

    def exploitability(self, P):
        """-> out4 = [(BR0 + BR1) / 2, BR0, BR1, value] of the global policy P [G][4]"""
        out = np.zeros(4)
        with np.errstate(invalid="ignore", over="ignore"):
            for br in range(3):
                reach = [np.zeros(t.n_nodes) for t in self.trees]
                val = [np.zeros(t.n_nodes) for t in self.trees]
                for d, ref in enumerate(self.refs):
                    reach[d][0] = 1.0
                    for lv in ref.levels:
                        g = self.map[d, lv["inf"]]
                        for a in range(lv["n"]):
                            c = lv["child"][:, a]
                            reach[d][c] = reach[d][lv["nodes"]] if lv["p"] == br else reach[d][lv["nodes"]] * P[g, a]
                    val[d][ref.term_nodes] = -ref.term_val if br == 1 else ref.term_val
                for depth in range(7, -1, -1):
                    n, p = 4 - depth // 2, depth & 1
                    if p == br:
                        qs = []
                        for d, ref in enumerate(self.refs):
                            lv = ref.levels[depth]
                            q = np.zeros((ref.I, 4))
                            for a in range(n):
                                term = reach[d][lv["nodes"]] * val[d][lv["child"][:, a]]
                                for g in lv["groups"]:
                                    q[lv["inf"][g], a] = q[lv["inf"][g], a] + term[g]
                            qs.append(q)
                        Q = self.reduce(qs)
                        best = np.zeros(self.G, np.int64)
                        rows = np.arange(self.G)
                        for a in range(1, n):
                            best = np.where(Q[rows, a] > Q[rows, best], a, best)
                        for d, ref in enumerate(self.refs):
                            lv = ref.levels[depth]
                            val[d][lv["nodes"]] = val[d][lv["child"][np.arange(lv["nodes"].size), best[self.map[d, lv["inf"]]]]]
                    else:
                        for d, ref in enumerate(self.refs):
                            lv = ref.levels[depth]
                            g = self.map[d, lv["inf"]]
                            v = np.zeros(lv["nodes"].size)
                            for a in range(n):
                                v = v + P[g, a] * val[d][lv["child"][:, a]]
                            val[d][lv["nodes"]] = v
                s = val[0][0]
                for d in range(1, self.n):
                    s = s + val[d][0]
                out[1 + br] = s / float(self.n)
        out[0] = 0.5 * (out[1] + out[2])
        return out
