"""Float64 numpy restatement of the deal-sampled and simultaneous iterations of Team MiniScopa over a set of deals
(scopa_team_chance_cfr_iterate_sampled), on tests/team_chance_ref.py's ChanceRef.

TEST INFRASTRUCTURE, written for this repository's tests.  A list of deals is restated as ChanceRef's own sweep and fixed-order sum on the
SUB-INDEX of the listed deals: the listed deals in ascending id, their rows of the map with the GLOBAL ids kept, and the occurrences of every global
row among them in ascending (deal, row) order.  So

  sweep     only the listed deals, ChanceRef.sweep's arithmetic against the sigma rows gathered through their map rows
  reduce    a row's increments added over its LISTED occurrences in ascending (deal, row) order STARTING FROM THE FIRST listed one's value; a row of
            an updated team with no listed occurrence takes +0.0 for both sums (-0.0 + +0.0 is +0.0); then on EVERY row of the updated team
            R <- R + dR; R <- !(R <= 0) ? R * pos : R * neg; S <- (S + dS) * strat (weights None = no multiplication); sigma by regret matching
  root      the listed deals' root values added in ascending deal id from the first, divided by m
  alternating 1   traverser 0's sweep and reduce, then traverser 1's against the refreshed sigma; 0: both sweeps against the sigma of the
            iteration's start, then both teams' rows reduced
The order of the ids within a list cannot matter: the list is sorted first.
"""
import copy

import numpy as np

import team_cfr_ref as T


class SampledRef:
    def __init__(self, cr):
        self.cr = cr
        self._subs = {}

    def sub(self, deals):
        """ChanceRef restricted to the deals `deals` (any order, distinct): n = m, the map rows and payoffs of the listed deals in ascending id, the
        occurrence lists over them; global ids, keys, teams and legal counts are the full game's"""
        ids = tuple(sorted(int(d) for d in deals))
        assert len(set(ids)) == len(ids) >= 1 and 0 <= ids[0] and ids[-1] < self.cr.n
        if ids not in self._subs:
            cr, s = self.cr, copy.copy(self.cr)
            s.n = len(ids)
            s.map, s.r2 = cr.map[list(ids)], cr.r2[list(ids)]
            flat = s.map.reshape(-1).astype(np.int64)
            s.occ = np.argsort(flat, kind="stable").astype(np.int64)             # (position among the listed, row) ascending = (deal, row) ascending
            s.occ_off = np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=cr.G))]).astype(np.int64)
            self._subs[ids] = s
        return self._subs[ids]

    def increments(self, s, sig, p):
        """traverser p's sweep of the sub-game `s` -> (rows of team p, their summed increments [rows][8], the listed deals' mean root value)"""
        cr = self.cr
        img, roots = s.sweep(sig, p)
        rows = np.nonzero(cr.team == p)[0]
        acc = np.zeros((len(rows), 8))                                            # +0.0 where no occurrence is listed
        listed = (s.occ_off[rows + 1] - s.occ_off[rows]) > 0
        acc[listed] = s.reduce_rows(img, rows[listed])
        return rows, acc, float(s.mean(roots))

    def apply(self, R, S, sig, rows, acc, w):
        cr = self.cr
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            for b in (2, 3, 4):
                m = cr.nleg[rows] == b
                g = rows[m]
                Rn = R[g, :b] + acc[m, :b]
                Sn = S[g, :b] + acc[m, 4:4 + b]
                if w is not None:
                    Rn = np.where(~(Rn <= 0.0), Rn * float(w[0]), Rn * float(w[1]))
                    Sn = Sn * float(w[2])
                R[g, :b], S[g, :b] = Rn, Sn
                sig[g] = T.Ref.sigma(R[g], b)

    def iterate(self, R, S, sig, deals, weights=None, alternating=True):
        """one iteration per row of `deals` ([n_iters][m]; a row None = all deals) on the tables in place -> root values [n_iters][2]"""
        deals = list(deals)
        ws = [None] * len(deals) if weights is None else list(np.asarray(weights, np.float64).reshape(-1, 3))
        assert len(ws) == len(deals)
        out = np.zeros((len(deals), 2))
        for t, (lst, w) in enumerate(zip(deals, ws)):
            s = self.sub(range(self.cr.n) if lst is None else lst)
            if alternating:
                for p in (0, 1):
                    rows, acc, out[t, p] = self.increments(s, sig, p)
                    self.apply(R, S, sig, rows, acc, w)
            else:
                both = [self.increments(s, sig, p) for p in (0, 1)]              # both against the sigma of the iteration's start
                for p, (rows, acc, v) in enumerate(both):
                    out[t, p] = v
                    self.apply(R, S, sig, rows, acc, w)
        return out

