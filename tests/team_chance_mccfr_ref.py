"""Float64 numpy restatement of the sampling solver on Team MiniScopa over a set of deals (scopa_team_chance_mccfr.hip), built from the two
restatements it joins: tests/team_chance_ref.py's ChanceRef for the keys and the map, tests/team_mccfr_ref.py's MCRef(perm).walk for a deal's traversals.

TEST INFRASTRUCTURE, written for this repository's tests.

  walk      per listed deal, MCRef.walk against R0 = R_G[map[deal]] with the global traversal ids deal * batch + i (iterate) or b0 + i (traverse): the
            one-deal walk with every row read through the deal's map row.  Within a deal the map is injective, so the deal's increments land on distinct
            global rows
  scatter   dR, |inc| (the reorder budget's A) and the traverser-visit counts are added into [G] arrays deal after deal, in ascending deal order whatever the list's
  apply     rows with count > 0: R += dR; S[c] += count * sigma(R before the add)[c] over the legal slots; the row's sigma by ChanceRef's regret matching
            (what the CFR reduce leaves).  Other rows are not touched.  No discount, no n / m scaling
  NaN       the kernels' mc_sigma takes the positive part with `R > 0`, which is false for a NaN: a NaN regret cell counts as not positive and the other
            cells of its row keep their weights (the reference's np.maximum would make the whole row NaN and np.random.choice would raise there:
            tests/test_gpu_mccfr_edges.py).  MCRef._sigma uses np.maximum, so the walk and the apply read the regrets with every NaN replaced by 0.0 --
            the same positive part, cell for cell.  +inf and -inf need nothing: both sides compute inf / inf = NaN and max(-inf, 0) = 0
"""
import numpy as np

import philox_words as W
import team_cfr_ref as T
import team_chance_ref as TC
import team_mccfr_ref as M

PER_TRAVERSAL = 1731      # traverser instances of one traversal, either traverser
DRAWS, TERMINALS = 69964, 28800          # decision and terminal visits per pair of traversals

# the wide Philox words of tests/test_gpu_team_chance_mccfr.py, guarded on the CPU by tests/test_team_chance_mccfr_ref.py: nb traversals of the last deal
# of the two-deal set `swap`; b0 <= 0xFFFFFFFF - nb is the entry point's limit.  WORD_BATCH: the batch of the iterations under the wide seed, over
# all deals and then over WORD_LIST, whose order is not ascending (a slot is not its deal's id)
WORD_NB = WORD_BATCH = 2
WORD_CASES = W.word_cases(0x5C09A, WORD_NB, W.M32 - WORD_NB)
WORD_LIST = [1, 0]

_MC = {}


def mc_of(perm):
    """MCRef of a deal, with team_chance_ref's fast payoffs in place of team_cfr_ref's enumeration; one per deal and session"""
    key = bytes(np.ascontiguousarray(perm, np.uint8))
    if key not in _MC:
        T._LEAVES.setdefault(key, TC.walk(perm)[1])
        _MC[key] = M.MCRef(np.frombuffer(key, np.uint8))
    return _MC[key]


def positive_part_source(R):
    """the regrets as mc_sigma reads them: a NaN is not positive"""
    return np.where(np.isnan(R), 0.0, R)


class _Marks:
    """what MCRef.walk marks beside its increments; the chance game keeps neither"""

    def __init__(self, ref):
        self.seen = np.zeros(ref.n_rows, np.uint8)
        self.lv = np.zeros((2, ref.n_leaves), np.uint64)


class ChanceMCRef:
    def __init__(self, perms, cr=None):
        self.cr = TC.ChanceRef(perms) if cr is None else cr
        self.n, self.G = self.cr.n, self.cr.G
        self.mc = [mc_of(p) for p in self.cr.perms]

    def tables(self):
        return self.cr.tables()

    def deal_delta(self, R, seed, iteration, deal, first, nb, ids=None):
        """traversals first .. first + nb - 1 (or the global ids `ids`) of both traversers on `deal` against the shared regrets R
        -> (dR [321365][4], count [321365], A) over the deal's LOCAL rows"""
        mc, mp = self.mc[deal], self.cr.map[deal]
        R0 = positive_part_source(R[mp])
        dR, A, cnt = np.zeros_like(R0), np.zeros_like(R0), np.zeros(R0.shape[0])
        ids = np.arange(first, first + nb, dtype=np.uint64) if ids is None else np.asarray(ids, np.uint64)
        st = _Marks(mc.ref)
        for p in (0, 1):
            mc.walk(R0, st, p, ids, seed, iteration, dR, A, cnt)
        return dR, cnt, A

    def scatter(self, parts):
        """[(deal, dR, count, A)], added in the order given -> (dR [G][4], count [G], A [G][4])"""
        dR, A, cnt = np.zeros((self.G, 4)), np.zeros((self.G, 4)), np.zeros(self.G)
        with np.errstate(invalid="ignore", over="ignore"):
            for deal, d, c, a in parts:
                mp = self.cr.map[deal]          # injective within a deal: a plain indexed add
                dR[mp] = dR[mp] + d
                A[mp] = A[mp] + a
                cnt[mp] = cnt[mp] + c
        return dR, cnt, A

    def traverse(self, R, seed, iteration, deal, b0, nb, ids=None):
        """scopa_team_chance_mccfr_traverse -> (dR, count, A) over the global rows"""
        return self.scatter([(deal,) + self.deal_delta(R, seed, iteration, deal, b0, nb, ids)])

    def delta(self, R, seed, iteration, batch, deals=None):
        """the walk launch of one iteration: every listed deal d (None = all) walks the ids d * batch + i -> (dR, count, A) over the global rows"""
        deals = range(self.n) if deals is None else sorted(int(d) for d in deals)
        return self.scatter([(d,) + self.deal_delta(R, seed, iteration, d, d * batch, batch) for d in deals])

    def apply(self, R, S, sig, dR, cnt):
        cr = self.cr
        with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
            for b in (2, 3, 4):
                ch = np.nonzero((cnt > 0) & (cr.nleg == b))[0]
                if ch.size == 0:
                    continue
                sg = M.MCRef._sigma(positive_part_source(R[ch, :b]))
                R[ch, :b] = R[ch, :b] + dR[ch, :b]
                S[ch, :b] = S[ch, :b] + cnt[ch, None] * sg
                sig[ch] = T.Ref.sigma(R[ch], b)

    def iterate(self, R, S, sig, batch, seed, iteration, deals=None):
        """one iteration in place -> (A, count)"""
        dR, cnt, A = self.delta(R.copy(), seed, iteration, batch, deals)
        self.apply(R, S, sig, dR, cnt)
        return A, cnt
