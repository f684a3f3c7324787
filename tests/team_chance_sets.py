"""Deal sets of Team MiniScopa whose rows are shared BELOW depth 1, for the tests of the chance game over a set of deals.

TEST INFRASTRUCTURE, a plain helper module.  algorithms.team_chance.packet_deals hands four disjoint packets to the seats, so the first card played
names the deal and only rows of depths 0 and 1 have more than one occurrence.  Here the deals differ by cards that are played late or never seen by
the acting seat, so a key (depth, the acting seat's initial hand in hand order, the cards played so far) recurs in several deals at every depth.
Each set is uint8 [n][16], seat s at bytes 4 s .. 4 s + 3.

  both4      the base deal; cards 14 and 12 exchanged between seats 1 and 3; cards 15 and 13 exchanged between seats 0 and 2; both exchanges.  A team
             cannot tell the other team's exchange until one of its two cards is played: both teams own rows with 2 occurrences at every depth 0..11
  reordered  the base deal, and the base deal with seat 0's hand stored as 5 0 15 10.  The hand's order is part of the key, so no row of seat 0 is
             shared; seats 1, 2 and 3 see the same cards played in both deals, so each of their rows has 2 occurrences -- reached through a map that
             permutes the local rows (seat 0's slot c is another card in the second deal)
  hidden6    seats 0 and 2 keep their hands; seat 1 holds 1 4 and two of {11, 14, 9, 12}, seat 3 holds 3 6 and the other two, hands ascending, in the
             order of itertools.combinations([11, 14, 9, 12], 2).  The rows of seats 0 and 2 (the even depths) have 1, 2, 3 or 6 occurrences down to
             depth 10: a + b + c is not order-free, so this set holds the reduce to its summation order.  Seats 1 and 3 see their own hand, which
             names the deal: every row of an odd depth has one occurrence

The restatements of the sets are built once per process (chance_ref, ref_run) and handed out read-only.
"""
from itertools import combinations

import numpy as np

BASE = [[0, 5, 10, 15], [1, 4, 11, 14], [2, 7, 8, 13], [3, 6, 9, 12]]
NAMES = ("both4", "reordered", "hidden6")
ROWS = {"both4": 1217100, "reordered": 342358, "hidden6": 1760433}      # distinct keys, measured with team_chance_ref.ChanceRef
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def chance_ref(name):
    import team_chance_ref as TC
    return cached(("ref", name), lambda: TC.ChanceRef(deal_set(name)))


def chance_mc_ref(name):
    import team_chance_mccfr_ref as CM
    return cached(("mc", name), lambda: CM.ChanceMCRef(deal_set(name), chance_ref(name)))


def ref_run(name, variant, n_iters=3):
    """(R, S, sigma, root values) of the restatement after n_iters iterations of `variant` from reset, read-only"""
    def make():
        from scopa_amd.algorithms import schedule
        cr = chance_ref(name)
        R, S, sig = cr.tables()
        rv = cr.iterate(R, S, sig, weights=schedule(variant, 0, n_iters))
        for a in (R, S, sig, rv):
            a.setflags(write=False)
        return R, S, sig, rv
    return cached(("run", name, variant, n_iters), make)


def _deal(hands):
    return [c for h in hands for c in h]


def both4():
    h1, h3 = [1, 4, 11, 12], [3, 6, 9, 14]
    h0, h2 = [0, 5, 10, 13], [2, 7, 8, 15]
    return np.array([_deal(BASE), _deal([BASE[0], h1, BASE[2], h3]), _deal([h0, BASE[1], h2, BASE[3]]), _deal([h0, h1, h2, h3])], np.uint8)


def reordered():
    return np.array([_deal(BASE), _deal([[5, 0, 15, 10]] + BASE[1:])], np.uint8)


def hidden6():
    pool = [11, 14, 9, 12]
    out = []
    for pair in combinations(pool, 2):
        rest = [c for c in pool if c not in pair]
        out.append(_deal([BASE[0], sorted([1, 4] + list(pair)), BASE[2], sorted([3, 6] + rest)]))
    return np.array(out, np.uint8)


def deal_set(name):
    sets = {"both4": both4, "reordered": reordered, "hidden6": hidden6}
    out = sets[name]()
    assert out.shape[1] == 16 and all(sorted(d) == list(range(16)) for d in out.tolist())
    return out


def occurrence_table(cr):
    """{depth: {occurrences: rows}} of a team_chance_ref.ChanceRef"""
    cnt = np.diff(cr.occ_off)
    out = {}
    for d in range(12):
        c, k = np.unique(cnt[cr.depth == d], return_counts=True)
        out[d] = dict(zip(c.tolist(), k.tolist()))
    return out
