"""Float64 restatement of the weighted synchronous CFR sweep (k_cfr_sync_weighted) over oracle.Tree's exported arrays.

TEST INFRASTRUCTURE, written for this repository's tests: the GPU kernel is held to it bit for bit, and it is itself anchored to the C oracle
(Tree.cfr_sync) with weights (1, 1, 1).  Every float64 operation is one numpy elementwise operation (one rounding, no fused multiply-add), in the
kernel's order:
  sigma     regret matching of the current regrets, `!(R <= 0) ? R : 0` summed left to right; a row whose sum is not > 0 (NaN included) is uniform
  reach     top down, the mover's reach times sigma
  value     bottom up, children left to right starting from 0.0
  dR, dS    per cell, starting from 0.0, the infoset's nodes in ply order (Tree nodes are in DFS preorder: ascending index within a ply)
  update    R <- R + dR;  R <- !(R <= 0) ? R * pos : R * neg;  S <- (S + dS) * strat       with the iteration's weights (pos, neg, strat)
Simultaneous form: one sweep per iteration, both players' rows updated.  Alternating form: two sweeps, sweep p recomputes sigma for every
infoset and updates player p's rows only, player 0 first.
"""
import numpy as np

N_PLIES = 8


class Ref:
    def __init__(self, tree):
        t = self.tree = tree
        self.I = t.n_infosets
        self.nlegal = t.infoset_nlegal.astype(np.int64)
        self.legal = np.arange(4)[None, :] < self.nlegal[:, None]
        self.term_nodes = np.flatnonzero(t.term != 0)
        self.term_val = 0.5 * t.r2[self.term_nodes, 0].astype(np.float64)
        self.levels = []
        for d in range(N_PLIES):
            nodes = np.flatnonzero((t.depth == d) & (t.term == 0))
            n, p = int(t.nlegal[nodes[0]]), int(t.player[nodes[0]])
            assert (t.nlegal[nodes] == n).all() and (t.player[nodes] == p).all()
            inf = t.infoset[nodes].astype(np.int64)
            assert (self.nlegal[inf] == n).all() and (t.infoset_player[inf] == p).all()
            seen, rank = {}, np.zeros(nodes.size, np.int64)
            for j, i in enumerate(inf):                  # rank of a node among its infoset's nodes, in ply order
                rank[j] = seen.get(i, 0)
                seen[i] = rank[j] + 1
            groups = [np.flatnonzero(rank == k) for k in range(rank.max() + 1)]      # within a group every infoset appears once
            self.levels.append(dict(nodes=nodes, n=n, p=p, inf=inf, child=t.child[nodes, :n].astype(np.int64), groups=groups,
                                    rows=np.array(sorted(seen), np.int64)))
        assert all(t.depth[k] == N_PLIES for k in self.term_nodes)

    def sigma(self, R):
        with np.errstate(invalid="ignore", divide="ignore"):
            pos = np.where(self.legal, np.where(~(R <= 0.0), R, 0.0), 0.0)
            s = pos[:, 0].copy()
            for c in range(1, 4):
                s = np.where(c < self.nlegal, s + pos[:, c], s)
            uni = (1.0 / self.nlegal.astype(np.float64))[:, None]
            return np.where(self.legal, np.where((s > 0.0)[:, None], pos / s[:, None], uni), 0.0)

    def sweep(self, R, S, w, update):
        """one sweep in place; update: None = both players, 0 / 1 = that player's rows only"""
        t, (w_pos, w_neg, w_strat) = self.tree, (float(x) for x in w)
        sig = self.sigma(R)
        r0, r1, val = np.zeros(t.n_nodes), np.zeros(t.n_nodes), np.zeros(t.n_nodes)
        r0[0] = r1[0] = 1.0
        with np.errstate(invalid="ignore", over="ignore"):
            for lv in self.levels:
                for a in range(lv["n"]):
                    c, sg = lv["child"][:, a], sig[lv["inf"], a]
                    r0[c] = r0[lv["nodes"]] * sg if lv["p"] == 0 else r0[lv["nodes"]]
                    r1[c] = r1[lv["nodes"]] * sg if lv["p"] == 1 else r1[lv["nodes"]]
            val[self.term_nodes] = self.term_val
            for lv in reversed(self.levels):
                nodes, inf, p = lv["nodes"], lv["inf"], lv["p"]
                v = np.zeros(nodes.size)
                for a in range(lv["n"]):
                    v = v + sig[inf, a] * val[lv["child"][:, a]]
                val[nodes] = v
                if update is not None and update != p:
                    continue
                reach, opp, sgn = (r0[nodes], r1[nodes], 1.0) if p == 0 else (r1[nodes], r0[nodes], -1.0)
                rows = lv["rows"]
                for a in range(lv["n"]):
                    tR = opp * (sgn * (val[lv["child"][:, a]] - v))
                    tS = reach * sig[inf, a]
                    dR, dS = np.zeros(self.I), np.zeros(self.I)
                    for g in lv["groups"]:
                        dR[inf[g]] = dR[inf[g]] + tR[g]
                        dS[inf[g]] = dS[inf[g]] + tS[g]
                    Rn = R[rows, a] + dR[rows]
                    R[rows, a] = np.where(~(Rn <= 0.0), Rn * w_pos, Rn * w_neg)
                    S[rows, a] = (S[rows, a] + dS[rows]) * w_strat

    def run(self, R, S, weights, alternating=False):
        """len(weights) iterations in place on R, S ([n_infosets][4] float64)"""
        for w in np.asarray(weights, np.float64).reshape(-1, 3):
            if alternating:
                self.sweep(R, S, w, 0)
                self.sweep(R, S, w, 1)
            else:
                self.sweep(R, S, w, None)
        return R, S

    def exploitability(self, S):
        return self.tree.exploitability(self.tree.average_policy(S))[0]
