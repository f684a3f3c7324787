"""MiniScopa over a set of deals with the deal as a chance move (scopa_chance_* in include/scopa.h, _lib.ChanceGame).

A policy solved on one deal assumes the opponent's hand is known: that tree has no chance node.  Here chance picks one of a MultiDeal's deals
uniformly and infosets are shared across deals by key -- P{player}:H[own hand]_T[table], what a player who cannot see the other hand knows -- so
the solved policy is a table over KEYS and carries over to deals it never saw (table_for).  The iterations, the reduction across deals and the
exploitability run in the library's kernels; this module is the host loop, the deal sets and the key dictionaries.
"""
from itertools import combinations

import numpy as np

from .cfr_variants import schedule


def sample_deals(n, m, start, count, seed=0):
    """The deal samples of iterations start .. start + count - 1: int32 [count][m], row i holding m distinct deals of n, ascending, drawn with
    np.random.Generator(np.random.Philox(key=[seed, start + i])).choice(n, m, replace=False).  Keyed by the absolute iteration, so a continued
    run draws what one long run draws."""
    n, m, start, count = int(n), int(m), int(start), int(count)
    if not 1 <= m <= n or start < 0 or count < 0:
        raise ValueError("sample_deals: need 1 <= m <= n, start >= 0 and count >= 0")
    out = np.zeros((count, m), np.int32)
    for i in range(count):
        out[i] = np.sort(np.random.Generator(np.random.Philox(key=[int(seed), start + i])).choice(n, m, replace=False))
    return out


def solve(multi, variant="cfr+", eps=1e-3, max_iters=1000, check_every=10, alternating=False, sample=None, seed=0, **params):
    """Run `variant` ("vanilla", "cfr+", "linear", "dcfr"; params: alpha, beta, gamma) on the chance game over a built MultiDeal's deals from
    iteration 1 until its exploitability is below eps or max_iters is reached: chunks of check_every weighted iterations with the schedule
    continued, exploitability() after each.  sample=m: every iteration sweeps only m of the n deals, sample_deals(n, m, t, k, seed), through
    cfr_iterate_sampled; the exploitability stays the exact one over all deals.  -> (ChanceGame, iterations run, [(iteration, exploitability), ...])."""
    from .._lib import ChanceGame
    game, t, curve = ChanceGame(multi), 0, []
    while t < max_iters:
        k = min(int(check_every), int(max_iters) - t)
        if sample is None:
            game.cfr_iterate_weighted(schedule(variant, t, k, **params), alternating)
        else:
            game.cfr_iterate_sampled(sample_deals(game.n, sample, t, k, seed), schedule(variant, t, k, **params), alternating)
        t += k
        curve.append((t, float(game.exploitability()[0])))
        if curve[-1][1] < eps:
            break
    return game, t, curve


def solve_mccfr(multi, batch, eps=1e-3, max_iters=1000, check_every=10, sample=None, seed=0):
    """Run chance-sampled external-sampling MCCFR (ChanceGame.mccfr_iterate: `batch` traversal pairs per listed deal and iteration, Philox seed
    `seed`) on the chance game over a built MultiDeal's deals until its exploitability is below eps or max_iters is reached: chunks of check_every
    iterations, the exact exploitability() over all deals after each.  sample=m: every iteration walks only m of the n deals,
    sample_deals(n, m, t, k, seed).  -> (ChanceGame, iterations run, [(iteration, exploitability), ...])."""
    from .._lib import ChanceGame
    game, t, curve = ChanceGame(multi), 0, []
    while t < max_iters:
        k = min(int(check_every), int(max_iters) - t)
        game.mccfr_iterate(batch, k, seed, None if sample is None else sample_deals(game.n, sample, t, k, seed))
        t += k
        curve.append((t, float(game.exploitability()[0])))
        if curve[-1][1] < eps:
            break
    return game, t, curve


def hidden_hand_deals(hand0):
    """The 495 deals in which seat 0 holds `hand0` (4 cards, in this order) and seat 1 any 4 of the other 12 cards: uint8 [495][16] perms =
    seat-0 hand + seat-1 hand (ascending, the combinations in lexicographic order) + the remaining 8 cards ascending."""
    hand0 = [int(c) for c in hand0]
    if len(hand0) != 4 or len(set(hand0)) != 4 or not all(0 <= c < 16 for c in hand0):
        raise ValueError("hand0 must be 4 distinct cards in 0..15")
    rest = [c for c in range(16) if c not in hand0]
    perms = [hand0 + list(h1) + [c for c in rest if c not in h1] for h1 in combinations(rest, 4)]
    return np.array(perms, np.uint8)


def policy_by_key(game, policy=None):
    """{key: float64 [4] row} of `policy` ([G][4]; None = the game's average policy)"""
    keys, _ = game.index()
    if policy is None:
        _, policy = game.exploitability(return_policy=True)
    return {int(k): np.array(row, np.float64) for k, row in zip(keys, policy)}


def table_for(ctx, by_key):
    """A policy table [n_infosets][4] for the deal `ctx` holds -- any deal, held out or not: the row of every key in `by_key`, uniform over the
    legal actions (bits 1-3 of the key) for a key it does not have.  Host glue over the tree's exported keys."""
    keys = ctx.tree_export()["infoset_key"]
    P = np.zeros((len(keys), 4))
    for r, k in enumerate(keys):
        row = by_key.get(int(k))
        if row is None:
            n = (int(k) >> 1) & 7
            P[r, :n] = 1.0 / n
        else:
            P[r] = row
    return P
