"""Restatement of the chance game's MCCFR iteration (scopa_chance_mccfr_iterate: k_mccfr_chance, k_chance_reduce_mccfr) over ChanceRef's index and
the C oracle's per-deal batched-MCCFR deltas.

TEST INFRASTRUCTURE, written for this repository's tests.  One iteration on global tables Rg, Sg ([G][4] float64), deal list `deals` (None = all):
  per listed deal d, ascending   R_local = Rg[map[d, :I_d]];  dR, dS, dA = Tree.mccfr_batched_delta_abs(R_local, seed, iteration, d * batch, batch)
                                 -- the traversal ids follow the deal id, not its place in the list
  per global row                 dR and dA summed over its listed occurrences in ascending (deal, local id) order starting from the first one's
                                 value; visits = the integer sum of rint(dS.sum(1)) (the oracle adds sigma once per traverser visit and a sigma
                                 row sums to 1)
  touched rows only              Sg += visits * mccfr_edges.reference_sigma(Rg_old, nlegal) on the legal cells, one product and one sum each;
                                 Rg += dR on the legal cells.  A row with no listed occurrence keeps its bits
It is anchored to oracle.Tree.mccfr_batched with one deal (tests/test_chance_mccfr_ref.py)."""
import numpy as np

import mccfr_edges as E
from chance_ref import ChanceRef

PAIR_VISITS = (463, 240)   # decision and terminal visits of one traversal pair
# tests/test_gpu_chance_mccfr.py's iterations under tests/philox_words.py's wide seed on the six-deal set: the smallest batch, all deals at iteration 0,
# this list at iteration 1; guarded on the CPU by tests/test_chance_mccfr_ref.py
WORD_BATCH = 1
WORD_LIST = [4, 0, 3]


class ChanceMccfrRef:
    def __init__(self, trees):
        self.ref = trees if isinstance(trees, ChanceRef) else ChanceRef(trees)
        self.n, self.G, self.map, self.I, self.nlegal, self.legal = self.ref.n, self.ref.G, self.ref.map, self.ref.I, self.ref.nlegal, self.ref.legal

    def tables(self):
        return self.ref.tables()

    def listed_rows(self, deals=None):
        """bool [G]: rows with at least one occurrence in a listed deal"""
        hit = np.zeros(self.G, bool)
        for d in (range(self.n) if deals is None else deals):
            hit[self.map[int(d), :self.I[int(d)]]] = True
        return hit

    def deltas(self, Rg, batch, seed, iteration, deals=None):
        """-> dR [G][4], A [G][4] (sum of |increment| per cell), visits int64 [G], touched bool [G], (decision visits, terminal visits)"""
        deals = list(range(self.n)) if deals is None else sorted(int(d) for d in deals)
        assert len(set(deals)) == len(deals) and all(0 <= d < self.n for d in deals) and self.n * int(batch) <= 1 << 32
        dR, A = np.zeros((self.G, 4)), np.zeros((self.G, 4))
        visits, touched, dvis, tvis = np.zeros(self.G, np.int64), np.zeros(self.G, bool), 0, 0
        for d in deals:
            rows = self.map[d, :self.I[d]].astype(np.int64)          # a deal's keys are distinct: no row twice
            dr, ds, da, dv, tv = self.ref.trees[d].mccfr_batched_delta_abs(np.ascontiguousarray(Rg[rows]), seed, iteration, d * int(batch), int(batch))
            first = ~touched[rows]
            with np.errstate(invalid="ignore", over="ignore"):
                dR[rows] = np.where(first[:, None], dr, dR[rows] + dr)
                A[rows] = np.where(first[:, None], da, A[rows] + da)
            c = np.rint(ds.sum(1)).astype(np.int64)
            assert np.array_equal(c == 0, ~(ds != 0).any(1))
            visits[rows] += c
            touched[rows] = True
            dvis, tvis = dvis + dv, tvis + tv
        return dR, A, visits, touched, (dvis, tvis)

    def iterate(self, Rg, Sg, batch, seed, iteration, deals=None):
        """one iteration in place -> (A, visits, touched, (decision visits, terminal visits))"""
        dR, A, visits, touched, vis = self.deltas(Rg, batch, seed, iteration, deals)
        cells = self.legal & touched[:, None]
        sig = np.zeros((self.G, 4))
        sig[touched] = E.reference_sigma(Rg[touched], self.nlegal[touched])
        with np.errstate(invalid="ignore", over="ignore"):
            Sg[cells] = (Sg + visits.astype(np.float64)[:, None] * sig)[cells]
            Rg[cells] = (Rg + dR)[cells]
        return A, visits, touched, vis

    def run(self, Rg, Sg, batch, seed, iter0, n_iters, lists=None):
        """n_iters iterations from iteration number iter0 in place; lists: None or [n_iters][m] -> the per-row sum of A over the iterations"""
        A_sum = np.zeros(self.G)
        for t in range(n_iters):
            A, _, _, _ = self.iterate(Rg, Sg, batch, seed, iter0 + t, None if lists is None else lists[t])
            A_sum += A.sum(1)
        return A_sum
