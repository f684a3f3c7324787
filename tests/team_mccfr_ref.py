"""Float64 Python / numpy restatement of the Team MiniScopa sampling solver (scopa_team_mccfr.hip): the reference's MCCFRTrainer._sample
(src/algorithms/mc_cfr.py:37-86) on TPIMiniScopaGame in its own visit order, and the batched definition, level-vectorised over the batch.

TEST INFRASTRUCTURE, written for this repository's tests.  Shape, rows and payoffs come from tests/team_cfr_ref.py; the sequential form is anchored to
the reference's own recursion by tests/golden/team_mccfr.npz (tests/test_team_mccfr_ref.py) and the GPU kernels are held to this module.

  sigma     InfoNode.current_strategy (:20-24): np.maximum(R, 0), summed left to right, divided; uniform where the sum is 0
  choice    np.random.choice(legal, p=sigma) (:55): cdf = cumsum(p); cdf /= cdf[-1]; searchsorted(cdf, u, side="right"); ONE uniform per decision visit,
            forced plies included
  shape     a visit instance of a traverser ply with b cards has b + 1 child instances (slot 0 the sampled child :67, slot 1 + c child c :72-78), any
            other ply one.  Instance j of depth d has index IOFF[p][d] + j in the traversal; its children are j * m + slot.  Fixed, whatever is drawn
  value     the reward of the leaf the sampled descent ends in (:86, :38-39); cfv_all[c] = that of loop child c
  update    traverser's rows: regret_sum += weight * (cfv_all - v), v = np.dot(sigma, cfv_all), weight = reach[opp] / sampling[trav] or 0 where the
            sampling probability is 0 (:79-83); strategy_sum += sigma (reach_probs[traverser] is never updated, :61-65)
  forced    below a depth-12 node: 11 (traverser 0) or 5 (traverser 1) more draws, four terminals; the team's first forced ply is visited once per
            arrival and its second twice, regret stays [0.], strategy_sum = the visit count.  Kept as leaf_visits[p][depth-12 node]

np.dot of two short float64 vectors is the chain v = fma(sigma[i], cfv[i], v) from 0.0, and that is what both kernels compute.  `dot_fma` does it
exactly with rationals for the sequential form, `dot_fma_vec` with an error-free float64 emulation for the batched one: a v that is one rounding off
would be multiplied by importance weights of 1e50 and more on tables with tiny sigmas.  `replay(..., frozen=R0)` is the sequential form on a frozen
table: what ties the two forms together (tests/test_team_mccfr_ref.py).
"""
from fractions import Fraction

import numpy as np

import philox_words as W
import team_cfr_ref as T

PHILOX_TAG = 64
# the wide Philox words of tests/test_gpu_team_mccfr.py's traverse tests, guarded on the CPU by tests/test_team_mccfr_ref.py: nb traversals of the
# seed-42 deal from each start table; b0 <= 0xFFFFFFFF - nb is the entry point's limit.  ITERATE_WORDS: the one batched iteration under the wide seed
WORD_NB = 3
WORD_CASES = W.word_cases(0x5C09A, WORD_NB, W.M32 - WORD_NB)
ITERATE_WORDS = (W.WIDE_SEED, 0, 0)
WORD_TABLES = ("zero", "small_large")
FORCED_DRAWS = (11, 5)      # draws of the forced tail below a depth-12 node, per traverser
TERMINALS_PER_ARRIVAL = 4


def word_start(name):
    """the regret table a wide-word case starts from: reset tables (uniform sigma at every row), or oracle/mccfr_edges.py's small_large table, on
    which the sampled action depends on the draw through a non-uniform sigma at every depth"""
    import mccfr_edges as E
    n_legal = np.repeat([T.branch(d) for d in range(12)], T.WIDTH[:12])
    return np.zeros((n_legal.size, 4)) if name == "zero" else E.edge_table(name, n_legal)


def mult(p, d):
    return T.branch(d) + 1 if T.team_of(d) == p else 1


def shape(p, d0=0):
    """(IW, IOFF): instances per depth d0..12 and instances above each depth, of one traversal of team p from a depth-d0 root"""
    iw, ioff, w, o = {}, {}, 1, 0
    for d in range(d0, 13):
        iw[d], ioff[d] = w, o
        o += w
        if d < 12:
            w *= mult(p, d)
    return iw, ioff


def draws_per_traversal(p, d0=0):
    iw, ioff = shape(p, d0)
    return ioff[12] + iw[12] * FORCED_DRAWS[p]


def closed_form_visits(p, d0=0):
    """V(d) = 1 + (b + 1) V(d + 1) at the traverser's plies, 1 + V(d + 1) elsewhere, V(16) = 0: the reference's recursion, forced plies included"""
    v = 0
    for d in range(15, d0 - 1, -1):
        b = T.branch(d) if d < 12 else 1
        v = 1 + ((b + 1) * v if T.team_of(d) == p else v)
    return v


def dot_fma(sigma, cfv):
    v = 0.0
    for s, c in zip(sigma, cfv):
        s, c = float(s), float(c)
        if np.isfinite(s) and np.isfinite(c) and np.isfinite(v):
            v = float(Fraction(s) * Fraction(c) + Fraction(v))   # one rounding, as fma
        else:
            v = s * c + v
    return v


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def fma_vec(a, b, c):
    """fma(a, b, c) elementwise with one rounding, from float64 operations alone (Boldo and Melquiond, "Emulation of FMA and correctly rounded sums:
    proved algorithms using rounding to odd", 2008): a * b = uh + ul exactly (Dekker), c + uh = th + tl exactly, v = tl + ul rounded to odd, th + v rounded
    to nearest.  For finite operands whose product neither overflows nor falls below 2^-969: sigma in [0, 1] times a reward here.  Checked against the
    rational arithmetic of dot_fma in tests/test_team_mccfr_ref.py."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    uh = a * b
    sa, sb = 134217729.0 * a, 134217729.0 * b
    ah, bh = sa - (sa - a), sb - (sb - b)
    al, bl = a - ah, b - bh
    ul = ((ah * bh - uh) + ah * bl + al * bh) + al * bl
    th, tl = _two_sum(c, uh)
    v, err = _two_sum(tl, ul)
    even = (v.view(np.int64) & 1) == 0
    toward = np.where(err > 0, np.inf, -np.inf)
    v = np.where((err != 0) & even, np.nextafter(v, toward), v)
    return th + v


def dot_fma_vec(sigma, cfv):
    """v = fma(sigma[..., i], cfv[..., i], v) from 0.0 along the last axis"""
    v = np.zeros(sigma.shape[:-1])
    for i in range(sigma.shape[-1]):
        v = fma_vec(sigma[..., i], cfv[..., i], v)
    return v


def sigma_row(R):
    pos = np.maximum(R, 0)
    s = pos.sum()
    if s == 0:
        return np.ones_like(pos) / len(pos)
    return pos / s


def choose(sigma, u):
    cdf = sigma.cumsum()
    cdf /= cdf[-1]
    return int(cdf.searchsorted(u, side="right"))


class State:
    """tables of T.Ref plus the sampling solver's: seen [n_rows] uint8, leaf_visits [2][n_leaves] uint64"""

    def __init__(self, ref):
        self.R, self.S, self.L, self.Q = ref.tables()
        self.seen = np.zeros(ref.n_rows, np.uint8)
        self.lv = np.zeros((2, ref.n_leaves), np.uint64)

    def copy(self):
        o = State.__new__(State)
        o.R, o.S, o.L, o.Q, o.seen, o.lv = self.R.copy(), self.S.copy(), self.L.copy(), self.Q.copy(), self.seen.copy(), self.lv.copy()
        return o


class MCRef:
    def __init__(self, perm, path=()):
        self.ref = T.Ref(perm, path)
        self.d0 = self.ref.d0
        self.draws = tuple(draws_per_traversal(p, self.d0) for p in (0, 1))

    def state(self):
        return State(self.ref)

    # ---- the sequential form ------------------------------------------------------------------------------------------------------------------
    def replay(self, st, p, uniforms, upos=0, frozen=None):
        """one traversal of team p in the reference's visit order, uniforms[upos:] -> the next position.  frozen=None: live tables, updated in place
        (and local_strategy of the updated rows refreshed).  frozen=R0: regrets read from R0, the increments returned as (dR, count) besides."""
        ref, r2 = self.ref, self.ref.r2
        pos = [upos]
        dR = np.zeros_like(st.R) if frozen is not None else None
        cnt = np.zeros(ref.n_rows) if frozen is not None else None
        Rsrc = st.R if frozen is None else frozen

        def rec(d, idx, reach, samp):
            if d == 12:
                st.lv[p, idx] += np.uint64(1)
                pos[0] += FORCED_DRAWS[p]
                return 0.5 * float(r2[idx] if p == 0 else -r2[idx])
            b, row = T.branch(d), ref.off[d] + idx
            st.seen[row] = 1
            sigma = sigma_row(Rsrc[row, :b])
            a = choose(sigma, uniforms[pos[0]])
            pos[0] += 1
            if T.team_of(d) != p:
                return rec(d + 1, idx * b + a, reach * sigma[a], samp)
            util = rec(d + 1, idx * b + a, reach, samp * sigma[a])
            cfv = np.zeros(b)
            for c in range(b):
                cfv[c] = rec(d + 1, idx * b + c, reach, samp * sigma[c])
            v = dot_fma(sigma, cfv)
            weight = reach / samp if samp > 0 else 0
            if frozen is None:
                st.R[row, :b] += weight * (cfv - v)
                st.S[row, :b] += 1.0 * sigma
                st.L[row] = T.Ref.sigma(st.R[row:row + 1], b)[0]
            else:
                dR[row, :b] += weight * (cfv - v)
                cnt[row] += 1.0
            return util

        with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
            rec(self.d0, 0, 1.0, 1.0)
        return pos[0] if frozen is None else (pos[0], dR, cnt)

    def iteration(self, st, uniforms, upos=0):
        """MCCFRTrainer.iteration() (:88-92) -> the next stream position"""
        for p in (0, 1):
            upos = self.replay(st, p, uniforms, upos)
        return upos

    def stream_order(self, p):
        """the (depth, instance) of every draw of one traversal in the reference's visit order; (-1, -1) for a forced tail's draws"""
        out = []

        def rec(d, inst):
            if d == 12:
                out.extend([(-1, -1)] * FORCED_DRAWS[p])
                return
            out.append((d, inst))
            m = mult(p, d)
            for slot in range(m):
                rec(d + 1, inst * m + slot)

        rec(self.d0, 0)
        return out

    # ---- the batched definition -----------------------------------------------------------------------------------------------------------------
    def uniforms(self, p, ids, seed, iteration):
        """{depth: u [len(ids)][instances of that depth]}: u53(x0, x1) of Philox counter (instance index, traversal id, iteration, 64 + p)"""
        iw, ioff = shape(p, self.d0)
        ids = np.asarray(ids, np.uint64).reshape(-1, 1)
        out = {}
        for d in range(self.d0, 12):
            q = (np.arange(iw[d], dtype=np.uint64) + np.uint64(ioff[d])).reshape(1, -1)
            o = philox4x32_10(q, ids, np.uint64(iteration), np.uint64(PHILOX_TAG + p), int(seed))
            out[d] = ((o[0] >> np.uint64(5)).astype(np.float64) * 67108864.0 + (o[1] >> np.uint64(6)).astype(np.float64)) / 9007199254740992.0
        return out

    @staticmethod
    def _sigma(Rr):
        pos = np.maximum(Rr, 0)
        s = pos[..., 0].copy()
        for c in range(1, Rr.shape[-1]):
            s = s + pos[..., c]
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where((s == 0)[..., None], 1.0 / Rr.shape[-1], pos / s[..., None])

    def walk(self, R0, st, p, ids, seed, iteration, dR, A, cnt):
        """traversals `ids` of team p against the frozen regrets R0: increments added into dR, their absolute values into A, traverser visits into cnt,
        st.seen and st.lv updated"""
        ref = self.ref
        B = len(ids)
        if B == 0:
            return
        U = self.uniforms(p, ids, seed, iteration)
        node, reach, samp = np.zeros((B, 1), np.int64), np.ones((B, 1)), np.ones((B, 1))
        kept = {}
        with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
            for d in range(self.d0, 12):
                b, rows = T.branch(d), ref.off[d] + node
                st.seen[rows.reshape(-1)] = 1
                sg = self._sigma(R0[rows, :b])
                cdf = np.cumsum(sg, axis=-1)          # sequential adds along the short axis
                cdf = cdf / cdf[..., -1:]
                a = np.minimum((cdf <= U[d][..., None]).sum(-1), b - 1)
                sa = np.take_along_axis(sg, a[..., None], -1)[..., 0]
                if T.team_of(d) != p:
                    reach, node = reach * sa, node * b + a
                    continue
                kept[d] = (rows, sg, reach, samp)
                c = np.concatenate([a[..., None], np.broadcast_to(np.arange(b), a.shape + (b,))], -1)      # [B][w][b + 1]
                node = (node[..., None] * b + c).reshape(B, -1)
                samp = (samp[..., None] * np.take_along_axis(sg, c, -1)).reshape(B, -1)
                reach = np.repeat(reach, b + 1, axis=1)
            np.add.at(st.lv[p], node.reshape(-1), np.uint64(1))
            val = 0.5 * (ref.r2[node] if p == 0 else -ref.r2[node]).astype(np.float64)
            for d in range(11, self.d0 - 1, -1):
                if d not in kept:
                    continue
                b = T.branch(d)
                rows, sg, reach, samp = kept[d]
                val = val.reshape(B, -1, b + 1)
                cfv = val[..., 1:]
                v = dot_fma_vec(sg, cfv)
                wt = np.where(samp > 0, reach / np.where(samp > 0, samp, 1.0), 0.0)
                inc = wt[..., None] * (cfv - v[..., None])
                flat = rows.reshape(-1)
                for c in range(b):
                    np.add.at(dR[:, c], flat, inc[..., c].reshape(-1))
                    np.add.at(A[:, c], flat, np.abs(inc[..., c]).reshape(-1))
                np.add.at(cnt, flat, 1.0)
                val = val[..., 0]

    def delta(self, R0, st, seed, iteration, b0, nb):
        """the delta of traversals [b0, b0 + nb) of both teams against R0 -> (dR [n][4], count [n], A [n][4])"""
        return self.delta_ids(R0, st, seed, iteration, np.arange(b0, b0 + nb, dtype=np.uint64))

    def delta_ids(self, R0, st, seed, iteration, ids):
        """delta for any list of global traversal ids (tests/philox_words.py: the ids a kernel that narrowed b0 would walk)"""
        dR, A, cnt = np.zeros_like(R0), np.zeros_like(R0), np.zeros(R0.shape[0])
        ids = np.asarray(ids, np.uint64)
        for p in (0, 1):
            self.walk(R0, st, p, ids, seed, iteration, dR, A, cnt)
        return dR, cnt, A

    def apply(self, st, dR, cnt):
        """regret += dR; strategy += count * sigma of the regrets before the add; local_strategy of the changed rows refreshed"""
        ref = self.ref
        with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
            for d in range(self.d0, 12):
                b, rows = T.branch(d), ref.rows(d)
                ch = np.nonzero(cnt[rows] > 0)[0] + rows.start
                if ch.size == 0:
                    continue
                sg = self._sigma(st.R[ch, :b])
                st.R[ch, :b] = st.R[ch, :b] + dR[ch, :b]
                st.S[ch, :b] = st.S[ch, :b] + cnt[ch, None] * sg
                st.L[ch] = T.Ref.sigma(st.R[ch], b)

    def iterate(self, st, batch, seed, iteration):
        """one batched iteration in place -> (A, count)"""
        dR, cnt, A = self.delta(st.R.copy(), st, seed, iteration, 0, batch)
        self.apply(st, dR, cnt)
        return A, cnt

    # ---- what the reference's info_sets dict holds --------------------------------------------------------------------------------------------------
    def forced_strategy(self, st, leaf, d):
        """strategy_sum[0] of the forced node of depth d (12..15) below depth-12 node `leaf`: the CFR solver's leaf_reach_sum plus 1 x / 2 x the arrivals"""
        p = T.team_of(d)
        return float(st.Q[p, leaf]) + float(st.lv[p, leaf]) * (1.0 if (d & 1) == 0 else 2.0)

    def n_visited(self, st):
        return int(st.seen.sum()) + 4 * int(((st.lv[0] + st.lv[1]) > 0).sum())


def philox4x32_10(c0, c1, c2, c3, seed):
    """Philox4x32-10 vectorised over the counter words (broadcast uint64 arrays holding 32-bit values); key = (seed low, seed high)"""
    M = np.uint64(0xFFFFFFFF)
    c = [np.asarray(x, np.uint64) & M for x in (c0, c1, c2, c3)]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & M, p1 & M, ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & M, p0 & M]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M, (k1 + np.uint64(0xBB67AE85)) & M
    return c
