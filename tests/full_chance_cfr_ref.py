"""CPU restatement of the exact weighted CFR iteration of FullScopa ACROSS a set of decks (scopa_amd/csrc/scopa_full_chance_cfr.hip; the procedure is
stated under `cfr_iterate` of scopa_full_chance in include/scopa.h) on full_chance_exploit_ref's forest (tree_of, mix_up's value pass, mean_of) and
full_mccfr_ref's sigma_of, in float64 and in the procedure's own order of adds.

TEST INFRASTRUCTURE.  It follows steps 1-6 literally -- the deck-major forest, every pair of every choice level claimed as a zero row, sigma frozen
per sweep, two reaches top down, the value pass bottom up, per-pair sums in ascending forest index starting from 0.0, the weighted update per cell --
so the device's tables and sweep values are compared with it on bits; tests/test_full_chance_cfr_ref.py holds it in turn to a depth-first recursive
CFR per deck, to the exploitability restatement's value pass, to cfr_variants_ref's weighting rule and, with one round to go, to the best response.

  claim      every pair of the forest's choice levels gets a row in R and S ([0.0] * 3 where it has none)
  sweep      steps 3, 4: -> the sweep's value; updates the rows of player `update` (None: of both) in place
  iterate    step 5: -> (R, S, values [n][2]); the tables given are copied, not changed
  huge_rows  the edge table `huge` (cells near DBL_MAX, +inf, NaN and -inf cells in fixed rows) and `huge_finite` over a list of pairs

The pair has imperfect recall across rounds: with R > 1 this is CFR's arithmetic on rows that carry no convergence proof."""
import numpy as np

import full_chance_exploit_ref as X
import full_chance_ref as W
import full_exploit_ref as X1
import full_mccfr_ref as F


def claim(tree, R, S):
    for _, n, keys in tree[0]:
        if n > 1:
            for k in keys:
                if k not in R:
                    R[k] = [0.0] * 3
                if k not in S:
                    S[k] = [0.0] * 3


def weigh(r, w_pos, w_neg):
    """R <- !(R <= 0) ? R * pos : R * neg"""
    return r * w_pos if not (r <= 0.0) else r * w_neg


def sweep(tree, R, S, w, update):
    levels, leaf, n_decks = tree
    w_pos, w_neg, w_strat = (float(x) for x in w)
    prob = []
    for _, n, keys in levels:                    # sigma is frozen for the sweep: regret matching of the rows as the sweep finds them
        if n == 1:
            prob.append(None)
            continue
        row = {k: F.sigma_of(R[k], n) for k in set(keys)}
        prob.append([row[k] for k in keys])
    reach, w2 = [], ([1.0] * n_decks, [1.0] * n_decks)
    for d, (p, n, _) in enumerate(levels):       # w2[q] multiplies by prob at player q's choice levels only
        reach.append(w2)
        if n > 1:
            mine = [w2[p][g] * prob[d][g][a] for g in range(len(w2[p])) for a in range(n)]
            other = [w2[1 - p][g] for g in range(len(w2[p])) for a in range(n)]
            w2 = (mine, other) if p == 0 else (other, mine)
    V = leaf
    for d in reversed(range(len(levels))):
        p, n, keys = levels[d]
        if n == 1:                               # (a one-card node takes its child's value: same index, same list)
            continue
        Vc, V = V, X1.mix_up(prob[d], V, n)
        if update is not None and update != p:
            continue
        w_opp, w_own = reach[d][1 - p], reach[d][p]
        dR, dS = {}, {}
        for g, k in enumerate(keys):             # ascending forest index: deck by deck, within a deck in node order
            r, s = dR.get(k), dS.get(k)
            if r is None:
                r, s = dR[k], dS[k] = [0.0] * 3, [0.0] * 3
            xg = -V[g] if p else V[g]
            for a in range(n):
                xc = -Vc[g * n + a] if p else Vc[g * n + a]
                r[a] += w_opp[g] * (xc - xg)
                s[a] += w_own[g] * prob[d][g][a]
        for k, r in dR.items():
            for a in range(n):
                R[k][a] = weigh(R[k][a] + r[a], w_pos, w_neg)
                S[k][a] = (S[k][a] + dS[k][a]) * w_strat
    return X.mean_of(V[:n_decks], n_decks)


HUGE_SEED = 308
HUGE_MARKS = ((7, 1, np.inf), (11, 2, np.nan), (13, 3, -np.inf))   # (prime, residue, the regret cell of the rows with index % prime == residue)
HUGE_STRATEGY_MARK = (5, 4)                                        # rows with index % 5 == 4: one legal strategy cell is +inf


def huge_rows(keys, finite=False):
    """(pairs sorted by (A, B), n_act, regret [n][3], strategy [n][3]), as full_chance_ref.edge_rows: the table `huge` over the pairs, a fixed function
    of the pair list.  Row i is the i-th pair in (A, B) order; a fixed RandomState draws all three slots of every row, regret cells uniform in
    +-1.7e308 and strategy cells uniform in [0, 1.7e308); in the rows of HUGE_MARKS the legal regret cell i % n is +inf, NaN or -inf (a later mark
    wins), in those of HUGE_STRATEGY_MARK the legal strategy cell (i // 5) % n is +inf; cells beyond the action count are 0.0.  Sums of two cells
    overflow, inf / inf and inf * 0 make NaN.  finite: `huge_finite`, every non-finite cell replaced by 1e308"""
    keys = np.asarray(keys, np.uint64).reshape(-1, 2)
    keys = keys[np.lexsort((keys[:, 1], keys[:, 0]))]
    n_act = np.array([W.key_actions(k) for k in keys], np.int32)
    rs = np.random.RandomState(HUGE_SEED)
    m = keys.shape[0]
    rows = np.arange(m)
    R = (2.0 * rs.random_sample((m, 3)) - 1.0) * 1.7e308
    S = rs.random_sample((m, 3)) * 1.7e308
    for prime, res, cell in HUGE_MARKS:
        hit = rows % prime == res
        R[rows[hit], (rows % n_act)[hit]] = cell
    hit = rows % HUGE_STRATEGY_MARK[0] == HUGE_STRATEGY_MARK[1]
    S[rows[hit], ((rows // 5) % n_act)[hit]] = np.inf
    if finite:
        R[~np.isfinite(R)] = 1e308
        S[~np.isfinite(S)] = 1e308
    legal = np.arange(3)[None, :] < n_act[:, None]
    R[~legal] = 0.0
    S[~legal] = 0.0
    return keys, n_act, np.ascontiguousarray(R), np.ascontiguousarray(S)


def iterate(tree, R, S, weights, alternating=True):
    """weights [n][3] = (pos, neg, strat) per iteration -> (R, S, values [n][2]) from copies of the tables"""
    R, S = {k: list(v) for k, v in R.items()}, {k: list(v) for k, v in S.items()}
    weights = np.asarray(weights, np.float64).reshape(-1, 3)
    if weights.shape[0]:
        claim(tree, R, S)
    values = np.zeros((weights.shape[0], 2))
    for t, w in enumerate(weights):
        if alternating:
            values[t] = [sweep(tree, R, S, w, 0), sweep(tree, R, S, w, 1)]
        else:
            values[t] = sweep(tree, R, S, w, None)
    return R, S, values
