"""CPU checks of the restatement of the sampling solver on Team MiniScopa over a set of deals (tests/team_chance_mccfr_ref.py) against the one-deal
restatement tests/team_mccfr_ref.py, and of the entry points' declaration, binding and export."""
import os
import re

import numpy as np
import pytest

import philox_words as W
import team_chance_mccfr_ref as CM
import team_chance_ref as TC
import team_chance_sets as TS
import team_mccfr_ref as M
from conftest import ROOT

PACKETS = [[0, 5, 10, 15], [1, 4, 11, 14], [2, 7, 8, 13], [3, 6, 9, 12]]
SEED = 0x5C09A


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def six(oracle):
    from scopa_amd.algorithms.team_chance import packet_deals
    return packet_deals(PACKETS, fix_seat0=True)


@pytest.fixture(scope="module")
def ref_six(six):
    return CM.ChanceMCRef(six)


def test_one_deal_is_the_one_deal_solver_through_the_map(six):
    cm, mc = CM.ChanceMCRef(six[:1]), CM.mc_of(six[0])
    mp = cm.cr.map[0]
    assert cm.G == mp.size and np.array_equal(np.sort(mp), np.arange(cm.G))
    R, S, sig = cm.tables()
    st = mc.state()
    for it in range(2):
        A, cnt = cm.iterate(R, S, sig, 3, SEED, it)
        A1, cnt1 = mc.iterate(st, 3, SEED, it)
        assert np.array_equal(cnt[mp], cnt1) and np.array_equal(bits(A[mp]), bits(A1))
        assert np.array_equal(bits(R[mp]), bits(st.R)) and np.array_equal(bits(S[mp]), bits(st.S)) and np.array_equal(bits(sig[mp]), bits(st.L))
    assert np.count_nonzero(st.R) > 1000


def test_two_copies_draw_independent_traversals(six):
    """deal 1 of the set walks the ids batch .. 2 batch - 1: with both copies the counts are those of 2 batch traversals of the one deal"""
    B = 4
    cm, mc = CM.ChanceMCRef(six[[0, 0]]), CM.mc_of(six[0])
    mp = cm.cr.map[0]
    assert cm.G == mp.size and np.array_equal(cm.cr.map[0], cm.cr.map[1])
    R, _, _ = cm.tables()
    dR, cnt, A = cm.delta(R, SEED, 7, B)
    st = mc.state()
    dR1, cnt1, A1 = mc.delta(st.R, st, SEED, 7, 0, 2 * B)
    assert np.array_equal(cnt[mp], cnt1) and cnt.sum() == 2 * B * 2 * CM.PER_TRAVERSAL
    half, _, _ = mc.delta(st.R, st, SEED, 7, B, B)                                    # the second copy alone: ids B .. 2 B - 1
    assert np.array_equal(bits(cm.deal_delta(R, SEED, 7, 1, B, B)[0]), bits(half))
    assert np.allclose(dR[mp], dR1, rtol=1e-12, atol=1e-12)                               # the same increments, added copy after copy


def test_list_order_and_unlisted_deals_do_not_change_a_listed_deals_increments(six, ref_six):
    cm, B = ref_six, 3
    rng = np.random.default_rng(5)
    R = np.where(np.arange(4)[None, :] < cm.cr.nleg[:, None], rng.standard_normal((cm.G, 4)), 0.0)
    a = cm.delta(R, SEED, 2, B, deals=[0, 3])
    b = cm.delta(R, SEED, 2, B, deals=[3, 0])
    for x, y in zip(a, b):
        assert np.array_equal(bits(x), bits(y))
    assert a[1].sum() == 2 * B * 2 * CM.PER_TRAVERSAL
    # the same two deals in the set without deals 4 and 5: other global ids, the same keys, the same increments per key
    small = CM.ChanceMCRef(six[:4])
    where = np.searchsorted(cm.cr.gkey, small.cr.gkey)
    assert np.array_equal(cm.cr.gkey[where], small.cr.gkey)
    c = small.delta(R[where], SEED, 2, B, deals=[0, 3])
    for x, y in zip(a, c):
        assert np.array_equal(bits(x[where]), bits(y))
    touched = np.zeros(cm.G, bool)
    touched[where] = True
    assert not a[1][~touched].any()
    # a deal's own increments are a function of (regrets, seed, iteration, deal id, batch) alone
    own = cm.deal_delta(R, SEED, 2, 3, 3 * B, B)
    only3 = cm.delta(R, SEED, 2, B, deals=[3])
    assert np.array_equal(bits(only3[0][cm.cr.map[3]]), bits(own[0])) and np.array_equal(only3[1][cm.cr.map[3]], own[1])


@pytest.mark.parametrize("deals,batch", [(None, 2), ([4, 1, 2], 5)])
def test_counts_of_an_iteration(ref_six, deals, batch):
    cm = ref_six
    R, S, sig = cm.tables()
    A, cnt = cm.iterate(R, S, sig, batch, SEED, 0, deals)
    m = cm.n if deals is None else len(deals)
    assert cnt.sum() == m * batch * 2 * CM.PER_TRAVERSAL
    idle = cnt == 0
    assert not R[idle].any() and not S[idle].any() and not A[idle].any()
    assert np.allclose(S.sum(1), cnt, rtol=1e-15 * 4, atol=0.0)                            # zero regrets: uniform sigma, count * (1 / b) summed over b slots
    assert np.array_equal(bits(sig), bits(cm.cr.sigma(R)))


# ---- the wide Philox words of tests/test_gpu_team_chance_mccfr.py ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ref_swap(six):
    return CM.ChanceMCRef(six[:2])


@pytest.mark.parametrize("seed,iteration,b0", CM.WORD_CASES + [(W.WIDE_SEED, 1, CM.WORD_BATCH)], ids=W.case_id)
def test_uniforms_at_wide_words_are_the_oracles(oracle, ref_swap, seed, iteration, b0):
    """the draws of the last deal's walks, at the traverse cases and at the ids deal * batch + i of the second iteration under the wide seed"""
    mc, ids = ref_swap.mc[-1], W.ids_of(b0, CM.WORD_NB)
    for p in (0, 1):
        iw, ioff = M.shape(p)
        U = mc.uniforms(p, ids, seed, iteration)
        for d in (0, 3, 7, 11):
            for j in sorted({0, iw[d] // 3, iw[d] - 1}):
                for i, b in enumerate(ids):
                    assert U[d][i, j] == oracle.philox_uniform(seed, ioff[d] + j, b, iteration, M.PHILOX_TAG + p), (p, d, j, b)


@pytest.mark.parametrize("seed,iteration,b0", CM.WORD_CASES, ids=W.case_id)
def test_wide_word_traversals_separate(ref_swap, seed, iteration, b0):
    """a condition on the GPU test's inputs: the count column it compares exactly differs from the one any narrowed word gives (tests/philox_words.py)"""
    cm, nb = ref_swap, CM.WORD_NB
    R, deal = cm.tables()[0], cm.n - 1
    want = cm.traverse(R, seed, iteration, deal, b0, nb)[1]
    assert want.sum() == nb * 2 * CM.PER_TRAVERSAL
    variants = W.narrowed(seed, iteration, b0, nb)
    assert variants
    for what, s, it, ids in variants:
        assert not np.array_equal(cm.traverse(R, s, it, deal, 0, nb, ids=ids)[1], want), what


@pytest.mark.parametrize("deals", [None, CM.WORD_LIST])
def test_wide_seed_iterations_separate(ref_swap, deals):
    """the same for the iterations under the wide seed, from reset tables: the count column, hence the strategy sums, is not the low key word's, and
    not the one of ids that follow the list slot instead of the deal"""
    cm, B = ref_swap, CM.WORD_BATCH
    R = cm.tables()[0]
    for it in (0, 1):
        want = cm.delta(R, W.WIDE_SEED, it, B, deals)[1]
        assert not np.array_equal(cm.delta(R, W.WIDE_SEED & W.M32, it, B, deals)[1], want)
        if deals is not None:
            assert deals != sorted(deals)
            by_slot = cm.scatter([(d,) + cm.deal_delta(R, W.WIDE_SEED, it, d, s * B, B) for s, d in enumerate(deals)])[1]
            assert not np.array_equal(by_slot, want)


def test_nan_regrets_count_as_not_positive():
    R = np.array([[np.nan, 2.0, 6.0, -1.0], [np.nan, np.nan, -3.0, 0.0], [np.inf, 1.0, 0.0, 0.0]])
    with np.errstate(invalid="ignore"):
        sg = M.MCRef._sigma(CM.positive_part_source(R))
    assert np.array_equal(sg[0], [0.0, 0.25, 0.75, 0.0]) and np.array_equal(sg[1], [0.25] * 4)
    assert np.isnan(sg[2, 0]) and np.array_equal(sg[2, 1:], [0.0, 0.0, 0.0])


def test_entry_points_are_declared_bound_and_exported(sl):
    names = ["traverse", "apply", "walk", "iterate", "counters", "delta_get"]
    hdr = open(os.path.join(ROOT, "include", "scopa.h")).read()
    assert set(re.findall(r"\bscopa_team_chance_mccfr_([a-z_]+)\s*\(", hdr)) == set(names)
    L = sl.lib()
    for n in names:
        sym = "scopa_team_chance_mccfr_" + n
        assert sym in sl.SYMBOLS and hasattr(L, sym) and getattr(L, sym).argtypes is not None, sym
    for m in ("mccfr_traverse", "mccfr_apply", "mccfr_iterate", "mccfr_counters", "mccfr_delta_get"):
        assert callable(getattr(sl.TeamChanceGame, m))
    import scopa_amd.algorithms as A
    assert callable(A.team_chance.solve_mccfr)


# ---- deal sets that share rows below depth 1 (tests/team_chance_sets.py) ------------------------------------------------------------------------
def rows_visited_from_several_deals(cm, batch, iteration, R=None, deals=None):
    """(global rows the iteration's walks visit from more than one deal, their depths), from the restatement"""
    R = cm.tables()[0] if R is None else R
    deals_seen = np.zeros(cm.G, np.int64)
    for d in (range(cm.n) if deals is None else deals):
        _, cnt, _ = cm.deal_delta(R, SEED, iteration, d, d * batch, batch)
        deals_seen[cm.cr.map[d][cnt > 0]] += 1
    rows = np.nonzero(deals_seen > 1)[0]
    return rows, cm.cr.depth[rows]


@pytest.mark.parametrize("name", ["both4", "reordered", "hidden6"])
def test_delta_on_deep_sharing_sets_is_the_one_deal_walks_scattered(oracle, name):
    """batch 3, iteration 0: the count column is the scatter-add of every deal's one-deal MCRef counts with the traversal ids deal * batch + i, and rows
    of depth 5 or more are visited from more than one deal (measured: 113 on both4, 192 on reordered, 209 on hidden6)"""
    cm, B = TS.chance_mc_ref(name), 3
    R, _, _ = cm.tables()
    dR, cnt, A = cm.delta(R, SEED, 0, B)
    want, want_dR = np.zeros(cm.G), np.zeros((cm.G, 4))
    for d, perm in enumerate(cm.cr.perms):
        mc = CM.mc_of(perm)
        dR1, cnt1, _ = mc.delta(R[cm.cr.map[d]], mc.state(), SEED, 0, d * B, B)
        np.add.at(want, cm.cr.map[d], cnt1)
        want_dR[cm.cr.map[d]] = want_dR[cm.cr.map[d]] + dR1
    assert np.array_equal(cnt, want) and cnt.sum() == cm.n * B * 2 * CM.PER_TRAVERSAL
    assert np.array_equal(bits(dR), bits(want_dR))
    rows, depth = rows_visited_from_several_deals(cm, B, 0)
    print(name, "rows visited from several deals:", rows.size, "of depth 5 or more:", int((depth >= 5).sum()), "of depths 2..4:", int(((depth >= 2) & (depth <= 4)).sum()))
    assert (depth >= 5).sum() > 0
    assert np.all(np.diff(cm.cr.occ_off)[rows] > 1) and np.all(cnt[rows] >= 2)
