"""Float64 restatement of the deal-sampled iterations of the chance game (scopa_chance_cfr_iterate_sampled: k_chance_sweep with a deal list,
k_chance_reduce_sampled) on top of chance_ref.ChanceRef.

TEST INFRASTRUCTURE, written for this repository's tests: the GPU kernels are held to it with np.array_equal (tests/test_gpu_chance_sampled.py), and
tests/test_chance_sampled_ref.py anchors it to ChanceRef, which is anchored to the C oracle.  An iteration sweeps only the listed deals:
  sweep     ChanceRef.deal_delta for every listed deal under the current sigma -- the same per-deal float64 operations as a full iteration
  reduce    per cell, the global row's occurrences are walked in ascending (deal, local id) order and the unsampled deals skipped: the sum STARTS
            FROM THE FIRST SAMPLED occurrence's value; a row without a sampled occurrence keeps the increment +0.0.  The order of a list plays no part
  update    ChanceRef.sweep's, on every row of the updated player(s), sampled or not: R <- R + dR; R <- !(R <= 0) ? R * pos : R * neg;
            S <- (S + dS) * strat.  Increments are not scaled by n / m
"""
import numpy as np

from chance_ref import ChanceRef


class SampledChanceRef(ChanceRef):
    def __init__(self, trees):
        super().__init__(trees)
        # the deal of every flat occurrence id (flat id = start[deal] + local)
        self.flat_deal = np.repeat(np.arange(self.n), self.I)

    def _check(self, deals):
        deals = [int(d) for d in np.asarray(deals).reshape(-1)]
        assert len(deals) >= 1 and len(set(deals)) == len(deals) and all(0 <= d < self.n for d in deals), deals
        return deals

    def sampled_mask(self, deals):
        mask = np.zeros(self.n, bool)
        mask[self._check(deals)] = True
        return mask

    def occurrence_stats(self, deals):
        """per global row: (occurrences, sampled occurrences, whether the row's FIRST occurrence is sampled) for the list `deals`"""
        mask = self.sampled_mask(deals)
        total, sampled = np.zeros(self.G, np.int64), np.zeros(self.G, np.int64)
        first_sampled = np.zeros(self.G, bool)
        for k, (rows, ids) in enumerate(self.occ_groups):
            on = mask[self.flat_deal[ids]]
            total[rows] += 1
            sampled[rows] += on
            if k == 0:
                first_sampled[rows] = on
        return total, sampled, first_sampled

    def reduce_sampled(self, per_deal, mask):
        """[G][4] sums over each global row's occurrences in order, skipping the deals not in `mask`, from the first sampled value; +0.0 where
        none is sampled.  per_deal[d] is read for the sampled deals only."""
        flat = np.concatenate([x if mask[d] else np.zeros((self.I[d], 4)) for d, x in enumerate(per_deal)], 0)
        acc = np.zeros((self.G, 4))
        started = np.zeros(self.G, bool)
        with np.errstate(invalid="ignore", over="ignore"):
            for rows, ids in self.occ_groups:                               # a row occurs at most once per group: plain fancy assignment
                on = mask[self.flat_deal[ids]]
                new, more = on & ~started[rows], on & started[rows]
                acc[rows[new]] = flat[ids[new]]
                acc[rows[more]] = acc[rows[more]] + flat[ids[more]]
                started[rows[new]] = True
        return acc

    def sweep_sampled(self, R, S, w, update, deals):
        w_pos, w_neg, w_strat = (float(x) for x in w)
        mask = self.sampled_mask(deals)
        sig = self.sigma(R)
        deltas = [self.deal_delta(d, sig[self.map[d, :self.I[d]]], update) if mask[d] else (None, None) for d in range(self.n)]
        dR, dS = self.reduce_sampled([x[0] for x in deltas], mask), self.reduce_sampled([x[1] for x in deltas], mask)
        cells = self.legal if update is None else self.legal & (self.player == update)[:, None]
        with np.errstate(invalid="ignore", over="ignore"):
            Rn = R + dR
            R[cells] = np.where(~(Rn <= 0.0), Rn * w_pos, Rn * w_neg)[cells]
            S[cells] = ((S + dS) * w_strat)[cells]

    def run_sampled(self, R, S, lists, weights=None, alternating=False):
        """len(lists) iterations in place on R, S ([G][4] float64): iteration t sweeps the deals lists[t]; weights None = all ones"""
        lists = [self._check(row) for row in lists]
        weights = np.ones((len(lists), 3)) if weights is None else np.asarray(weights, np.float64).reshape(-1, 3)
        assert len(weights) == len(lists)
        for deals, w in zip(lists, weights):
            if alternating:
                self.sweep_sampled(R, S, w, 0, deals)
                self.sweep_sampled(R, S, w, 1, deals)
            else:
                self.sweep_sampled(R, S, w, None, deals)
        return R, S
