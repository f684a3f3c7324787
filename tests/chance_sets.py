"""Deal sets at which the chance game's rows are shared by many deals, their measured figures, and cached float64 references.

TEST INFRASTRUCTURE, shared by tests/test_chance_scale_ref.py (CPU) and tests/test_gpu_chance_scale.py (GPU).  The six-deal set of the other chance
tests has 3 522 keys for 3 860 occurrences and no key in more than six deals; here a row occurs in up to 8 (BOTH25), 70 (HIDDEN70) and 495
(HIDDEN495, the benchmarks' set) deals, and the deals' infoset counts differ by a factor of two and more, so a deal's LDS carving by its own count
runs under a max_infosets far above it.  FIGURES were measured with tests/chance_ref.py on the CPU; the tests assert them before anything else, so
that nothing passes vacuously.  A reference is built once per process and never modified.
"""
from itertools import combinations

import numpy as np

from chance_sampled_ref import SampledChanceRef


def _perm(h0, h1):
    h0, h1 = list(h0), list(h1)
    return h0 + h1 + [c for c in range(16) if c not in h0 + h1]


def _hidden_hand_deals(hand0):
    from scopa_amd.algorithms.chance import hidden_hand_deals
    return hidden_hand_deals(hand0)


# both hands hidden: seat 0 any 4 of five cards (outer loop), seat 1 any 4 of five others
BOTH25 = np.array([_perm(h0, h1) for h0 in combinations([0, 5, 10, 15, 3], 4) for h1 in combinations([1, 2, 6, 7, 9], 4)], np.uint8)
# seat 0's hand fixed, seat 1 any 4 of eight cards
HIDDEN70 = np.array([_perm([0, 5, 10, 15], h1) for h1 in combinations([1, 2, 3, 4, 6, 7, 8, 9], 4)], np.uint8)
SETS = {"BOTH25": lambda: BOTH25, "HIDDEN70": lambda: HIDDEN70, "HIDDEN495": lambda: _hidden_hand_deals([0, 5, 10, 15])}

# name -> n deals, G keys, occurrences, smallest and largest infoset count of a deal, largest multiplicity of a row of seat 0 / seat 1,
# rows in 100 or more deals
FIGURES = {
    "BOTH25": dict(n=25, G=8817, n_occ=17220, I_min=422, I_max=1008, max_mult=(8, 7)),
    "HIDDEN70": dict(n=70, G=23970, n_occ=48560, I_min=308, I_max=1142, max_mult=(70, 8)),
    "HIDDEN495": dict(n=495, G=159365, n_occ=384789, I_min=308, I_max=1142, max_mult=(495, 28), rows_100_or_more=90),
}
BOTH25_HISTOGRAM = [2703, 4405, 1255, 386, 20, 40, 6, 2]      # rows per multiplicity 1 .. 8

WEIGHTINGS = ("vanilla", "cfr+", "dcfr")
# the sampled lists of HIDDEN495 at the benchmark's sizes: sample_deals(495, m, 0, 3, SAMPLE_SEED[m]).  The seeds are the smallest for which
# the lists' preconditions (check_sampled_lists) hold, found on the CPU with the reference alone
SAMPLE_SIZES = (16, 64)
SAMPLE_ITERS = 3
SAMPLE_SEED = {16: 0, 64: 0}


def weights(name, n):
    from scopa_amd.algorithms import schedule
    return schedule(name, 0, n, 1.5, 0.0, 2.0)


def perms(name):
    return SETS[name]()


def ref(oracle, name, _cache={}):
    """The set's SampledChanceRef (a ChanceRef with the sampled iterations on top), built once"""
    if name not in _cache:
        _cache[name] = SampledChanceRef([oracle.Tree(perm=p) for p in perms(name)])
    return _cache[name]


def multi(ctx, sl, name_or_perms):
    p = perms(name_or_perms) if isinstance(name_or_perms, str) else np.asarray(name_or_perms, np.uint8).reshape(-1, 16)
    m = sl.MultiDeal(ctx, len(p))
    m.set_perms(p)
    m.build()
    return m


def histogram(r):
    """rows per multiplicity 1, 2, ..."""
    return np.bincount(r.count)[1:].tolist()


def max_multiplicity(r):
    return tuple(int(r.count[r.player == p].max()) for p in (0, 1))


def check_figures(r, name):
    """the set's measured figures, asserted on its reference"""
    f = FIGURES[name]
    assert (r.n, r.G, r.n_occ) == (f["n"], f["G"], f["n_occ"]), (name, r.n, r.G, r.n_occ)
    assert max_multiplicity(r) == f["max_mult"], (name, max_multiplicity(r))
    if "I_min" in f:
        assert (min(r.I), max(r.I)) == (f["I_min"], f["I_max"]), (name, min(r.I), max(r.I))
    if "rows_100_or_more" in f:
        assert int((r.count >= 100).sum()) == f["rows_100_or_more"], (name, int((r.count >= 100).sum()))
    assert int((r.count == r.n).sum()) >= (0 if name == "BOTH25" else 1)


def sampled_lists(m):
    from scopa_amd.algorithms.chance import sample_deals
    return sample_deals(495, m, 0, SAMPLE_ITERS, SAMPLE_SEED[m])


def check_sampled_lists(r, lists):
    """every iteration lists some but not all occurrences of the row every deal shares; some iteration leaves a shared row without any"""
    root = np.flatnonzero(r.count == r.n)
    assert root.size >= 1
    none = False
    for deals in lists:
        total, sampled, _ = r.occurrence_stats(deals)
        assert (0 < sampled[root]).all() and (sampled[root] < total[root]).all(), deals
        none = none or bool(((total > 1) & (sampled == 0)).any())
    assert none
    return True
