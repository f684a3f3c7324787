"""Deal-sampled iterations of the chance game (scopa_chance_cfr_iterate_sampled: k_chance_sweep with a deal list, k_chance_reduce_sampled;
ChanceGame.cfr_iterate_sampled; chance.solve(sample=m)) on the GPU.

Every comparison is np.array_equal.  The six-deal set of tests/test_gpu_chance.py with three deals per iteration is held to
tests/chance_sampled_ref.py, which tests/test_chance_sampled_ref.py anchors to ChanceRef; the lists' preconditions (rows with sampled and unsampled
occurrences, rows whose first occurrence is unsampled, rows of both players with no sampled occurrence) are asserted first, so that nothing passes
vacuously.  With every deal listed the tables are cfr_iterate_weighted's; with one of two deals on disjoint cards they are the per-deal solver's."""
import ctypes as C

import numpy as np
import pytest

from chance_sampled_ref import SampledChanceRef

pytestmark = pytest.mark.gpu


def _perm(h0, h1):
    return h0 + h1 + [c for c in range(16) if c not in h0 + h1]


# the six-deal set of tests/test_gpu_chance.py
SIX = np.array([_perm([0, 5, 10, 15], h) for h in ([1, 2, 3, 4], [1, 2, 3, 6], [1, 2, 7, 6], [9, 8, 7, 6])] +
               [_perm([0, 5, 10, 14], h) for h in ([1, 2, 3, 4], [9, 8, 7, 6])], np.uint8)
WEIGHTINGS = ("vanilla", "cfr+", "dcfr")
LISTS = np.array([[1, 3, 4], [5, 2, 0], [0, 2, 3], [2, 4, 5], [1, 4, 5], [0, 3, 5], [1, 2, 5]], np.int32)   # the second one descending


def _weights(name, n):
    from scopa_amd.algorithms import schedule
    return schedule(name, 0, n, 1.5, 0.0, 2.0)


def _multi(ctx, sl, perms):
    perms = np.asarray(perms, np.uint8).reshape(-1, 16)
    m = sl.MultiDeal(ctx, len(perms))
    m.set_perms(perms)
    m.build()
    return m


def _six_ref(oracle, _cache={}):
    if not _cache:
        _cache["ref"] = SampledChanceRef([oracle.Tree(perm=p) for p in SIX])
    return _cache["ref"]


def _assert_preconditions(ref, lists):
    for deals in lists:
        total, sampled, first_sampled = ref.occurrence_stats(deals)
        assert ((sampled > 0) & (sampled < total)).any(), deals                               # a shared row with both kinds of occurrence
        assert (~first_sampled & (sampled > 0)).any(), deals                                  # an unsampled first occurrence, a sampled later one
        assert all(((sampled == 0) & (ref.player == p)).any() for p in (0, 1)), deals         # rows of each player that nothing touches
    assert any((np.diff(np.asarray(deals)) < 0).all() for deals in lists)                     # a list in descending order


def _six_tables(oracle, weighting, alternating, _cache={}):
    """the restatement's tables after 1, 2 and 7 sampled iterations over LISTS (computed once per case, never modified)"""
    key = (weighting, alternating)
    if key not in _cache:
        ref, w = _six_ref(oracle), _weights(weighting, 7)
        R, S = ref.tables()
        out, t = {}, 0
        for upto in (1, 2, 7):
            ref.run_sampled(R, S, LISTS[t:upto], w[t:upto], alternating)
            t = upto
            out[upto] = (R.copy(), S.copy())
        _cache[key] = out
    return _cache[key]


def _same(g, R, S):
    Rg, Sg = g.tables_get()
    return np.array_equal(Rg, R) and np.array_equal(Sg, S)


# ---- the six-deal set, three deals per iteration, against the float64 restatement ----------------------------------------------------------
@pytest.mark.parametrize("alternating", [False, True])
@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_six_deals_sampled_tables_and_exploitability(ctx, sl, oracle, weighting, alternating):
    ref, want = _six_ref(oracle), _six_tables(oracle, weighting, alternating)
    assert (ref.G, ref.n_occ) == (3522, 3860)
    _assert_preconditions(ref, LISTS)
    w = _weights(weighting, 7)
    g = sl.ChanceGame(_multi(ctx, sl, SIX))
    t = 0
    for upto in (1, 2, 7):
        g.cfr_iterate_sampled(LISTS[t:upto], w[t:upto], alternating)
        t = upto
        assert _same(g, *want[upto]), (weighting, alternating, upto)
    assert np.abs(want[7][0]).max() > 0 and np.abs(want[7][1]).max() > 0
    P = ref.average_policy(want[7][1])
    out, pol = g.exploitability(return_policy=True)
    assert np.array_equal(pol, P) and np.array_equal(out, ref.exploitability(P))
    # repeatability: a reset and the same call again
    g.tables_reset()
    g.cfr_iterate_sampled(LISTS, w, alternating)
    assert _same(g, *want[7])
    # the order of the ids within a list has no effect on any bit
    g.tables_reset()
    g.cfr_iterate_sampled(LISTS[:, ::-1], w, alternating)
    assert _same(g, *want[7])
    # continuation: the state after 2 iterations + the remaining lists
    g.tables_set(*want[2])
    g.cfr_iterate_sampled(LISTS[2:], w[2:], alternating)
    assert _same(g, *want[7])


@pytest.mark.parametrize("alternating", [False, True])
def test_sampled_and_full_calls_interleave(ctx, sl, oracle, alternating):
    ref, w = _six_ref(oracle), _weights("dcfr", 7)
    R, S = ref.tables()
    ref.run_sampled(R, S, LISTS[:2], w[:2], alternating)
    ref.run(R, S, w[2:5], alternating)
    ref.run_sampled(R, S, LISTS[5:], w[5:], alternating)
    g = sl.ChanceGame(_multi(ctx, sl, SIX))
    g.cfr_iterate_sampled(LISTS[:2], w[:2], alternating)
    g.cfr_iterate_weighted(w[2:5], alternating)
    g.cfr_iterate_sampled(LISTS[5:], w[5:], alternating)
    assert _same(g, R, S)
    assert np.array_equal(g.exploitability(), ref.exploitability(ref.average_policy(S)))      # the q rows reuse the increment buffer


@pytest.mark.parametrize("alternating", [False, True])
@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_every_deal_listed_is_the_weighted_call(ctx, sl, weighting, alternating):
    w = _weights(weighting, 5)
    m = _multi(ctx, sl, SIX)
    full, g = sl.ChanceGame(m), sl.ChanceGame(m)
    full.cfr_iterate_weighted(w, alternating)
    R, S = full.tables_get()
    assert np.abs(R).max() > 0 and np.abs(S).max() > 0
    g.cfr_iterate_sampled(np.tile(np.arange(6, dtype=np.int32), (5, 1)), w, alternating)       # the identity list
    assert _same(g, R, S)
    g.tables_reset()
    rng = np.random.Generator(np.random.Philox(key=[11, 0]))
    shuffled = np.array([rng.permutation(6) for _ in range(5)], np.int32)
    assert (shuffled != np.arange(6)).any()
    g.cfr_iterate_sampled(shuffled, w, alternating)
    assert _same(g, R, S)


def test_default_weights_are_all_ones(ctx, sl):
    m = _multi(ctx, sl, SIX)
    a, b = sl.ChanceGame(m), sl.ChanceGame(m)
    a.cfr_iterate_sampled(LISTS[:3])
    b.cfr_iterate_sampled(LISTS[:3], np.ones((3, 3)))
    R, S = a.tables_get()
    assert np.abs(R).max() > 0 and _same(b, R, S)
    with pytest.raises(ValueError):
        a.cfr_iterate_sampled(LISTS[:3], np.ones((2, 3)))
    assert _same(a, R, S)


@pytest.mark.parametrize("alternating", [False, True])
def test_one_of_two_disjoint_deals_is_the_per_deal_solver(ctx, sl, alternating):
    perms = np.array([list(range(16)), list(range(8, 16)) + list(range(8))], np.uint8)      # deal A plays cards 0-7, deal B cards 8-15
    w = _weights("cfr+", 3)
    m = _multi(ctx, sl, perms)
    g = sl.ChanceGame(m)
    IA, IB = (int(x) for x in m.n_infosets)
    assert g.G == IA + IB == g.n_occurrences
    _, mp = g.index()
    g.cfr_iterate_sampled(np.zeros((3, 1), np.int32), w, alternating)                       # m = 1: deal A, three times
    alone = _multi(ctx, sl, perms[0])
    alone.cfr_sync_iterate_weighted(w, alternating)
    Ra, Sa, _, _ = alone.tables_get(0)
    R, S = g.tables_get()
    assert np.abs(Ra).max() > 0 and np.array_equal(R[mp[0, :IA]], Ra) and np.array_equal(S[mp[0, :IA]], Sa)
    assert not R[mp[1, :IB]].any() and not S[mp[1, :IB]].any()


# ---- errors ---------------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_tables_alone(ctx, sl):
    L = sl.lib()
    g = sl.ChanceGame(_multi(ctx, sl, SIX))
    g.cfr_iterate_sampled(LISTS[:2], _weights("dcfr", 2))
    R, S = g.tables_get()
    assert np.abs(R).max() > 0

    def call(deals, m=None, weights=None, alternating=0, n_iters=None, handle=g._h):
        d = None if deals is None else np.ascontiguousarray(deals, np.int32)
        w = None if weights is None else np.ascontiguousarray(weights, np.float64)
        n_iters = d.shape[0] if n_iters is None else n_iters
        m = d.shape[1] if m is None else m
        return L.scopa_chance_cfr_iterate_sampled(handle, n_iters, m, sl._ptr(d), sl._ptr(w), alternating)

    nan_w = np.ones((2, 3))
    nan_w[1, 0] = np.nan
    bad = {"duplicate id": call([[0, 1, 2], [3, 4, 3]]),
           "id -1": call([[0, 1, 2], [-1, 4, 3]]),
           "id n": call([[0, 1, 2], [6, 4, 3]]),
           "m = 0": call(np.zeros((1, 1), np.int32), m=0),
           "m = n + 1": call(np.arange(7, dtype=np.int32)[None, :]),
           "alternating = 2": call(LISTS[:1], alternating=2),
           "NaN weight": call(LISTS[:2], weights=nan_w),
           "NULL handle": call(LISTS[:1], handle=None),
           "NULL list": call(None, m=3, n_iters=1),
           "n_iters < 0": call(LISTS[:1], n_iters=-1)}
    for what, rc in bad.items():
        assert rc == sl.SCOPA_EINVAL, what
        assert _same(g, R, S), what
    for deals in ([[0, 1, 2], [3, 4, 3]], np.zeros((1, 0), np.int32)):
        with pytest.raises(sl.ScopaError) as e:
            g.cfr_iterate_sampled(deals)
        assert e.value.status == sl.SCOPA_EINVAL
    assert call(None, m=3, n_iters=0) == sl.SCOPA_OK                                          # n_iters = 0: SCOPA_OK and nothing moves
    g.cfr_iterate_sampled(np.zeros((0, 3), np.int32))
    g.cfr_iterate_sampled(np.zeros((0, 3), np.int32), np.zeros((0, 3)), True)
    assert _same(g, R, S)
    g.cfr_iterate_sampled(LISTS[2:3], _weights("dcfr", 3)[2:])                                # and the handle still works
    assert not _same(g, R, S)


# ---- more deals than a round of workgroups, slot != deal id -------------------------------------------------------------------------------
def test_hidden_hand_deals_sampled(ctx, sl):
    from scopa_amd.algorithms.chance import hidden_hand_deals, sample_deals
    g = sl.ChanceGame(_multi(ctx, sl, hidden_hand_deals(sl.deal_py_seed(42)[:4])))
    _, mp = g.index()
    root = int(mp[0, 0])
    assert g.n == 495 and (mp[:, 0] == root).all()                                            # seat 0's first decision: one row for all 495 deals
    lists, w = sample_deals(495, 32, 0, 3), _weights("cfr+", 3)
    assert lists.shape == (3, 32) and (lists != np.arange(32)).any()                          # slot != deal id
    g.cfr_iterate_sampled(lists, w)
    R, S = g.tables_get()
    out = g.exploitability()
    assert np.isfinite(R).all() and np.isfinite(S).all() and np.isfinite(out).all()
    assert S[root].sum() > 0 and np.abs(R).max() > 0
    g.tables_reset()
    g.cfr_iterate_sampled(lists, w)
    assert _same(g, R, S) and np.array_equal(g.exploitability(), out)


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------------
def test_solve_with_sampled_deals(ctx, sl, oracle):
    from scopa_amd.algorithms import chance
    g, t, curve = chance.solve(_multi(ctx, sl, SIX), variant="cfr+", sample=3, seed=7, eps=0.0, max_iters=60, check_every=20)
    assert t == 60 and [c[0] for c in curve] == [20, 40, 60]
    print("cfr+ with 3 of 6 deals per iteration: exploitability at 20, 40, 60 iterations:", [c[1] for c in curve])
    assert curve[-1][1] < curve[0][1]
    assert curve[-1][1] == g.exploitability()[0]
    ref = _six_ref(oracle)                                                                    # the chunks continue the samples and the schedule
    R, S = ref.run_sampled(*ref.tables(), chance.sample_deals(6, 3, 0, 60, seed=7), _weights("cfr+", 60))
    assert _same(g, R, S)
