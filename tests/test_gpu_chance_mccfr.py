"""Chance-sampled external-sampling MCCFR on the chance game (scopa_chance_mccfr_iterate: k_mccfr_chance, k_chance_reduce_mccfr;
ChanceGame.mccfr_iterate; chance.solve_mccfr) on the GPU.

The six-deal set of tests/test_gpu_chance.py -- its preconditions asserted first -- is held to tests/chance_mccfr_ref.py, which
tests/test_chance_mccfr_ref.py anchors to the C oracle.  Visit counts, strategy sums and counters are exact (np.array_equal); regret rows, whose
increments a workgroup adds in arrival order, are held per row to the oracle's own reorder budget, oracle/mccfr_edges.py:
|R_gpu - R_ref| <= K_REORDER * eps * A_row + 2 * eps * |R_ref|, A_row = the sum of |increment| the oracle added into the row (the second term: the
rounding of R + dR itself).  That budget was derived for up to 17 923 pairs per row; no row here receives more than 6 * 48.  Runs of several
iterations are held to rtol = atol = 1e-10, the bound tests/test_gpu_multi.py uses for this walk.

Two deals on disjoint cards: scopa_multi_mccfr_iterate gives every deal the ids [0, batch), the chance game gives deal d the ids
[d * batch, (d + 1) * batch), so only deal 0 can coincide with the per-deal solver.  Each deal is therefore compared with MultiDeal.mccfr_iterate
from the game in which it is deal 0 (the pair in both orders), and as deal 1 it is held to the restatement."""
import ctypes as C

import numpy as np
import pytest

import mccfr_edges as E
import philox_words as W
from chance_mccfr_ref import PAIR_VISITS, WORD_BATCH, WORD_LIST, ChanceMccfrRef

pytestmark = pytest.mark.gpu

SEED = 0xC4A9CE


def _perm(h0, h1):
    return h0 + h1 + [c for c in range(16) if c not in h0 + h1]


# the six-deal set and the held-out deal of tests/test_gpu_chance.py
SIX = np.array([_perm([0, 5, 10, 15], h) for h in ([1, 2, 3, 4], [1, 2, 3, 6], [1, 2, 7, 6], [9, 8, 7, 6])] +
               [_perm([0, 5, 10, 14], h) for h in ([1, 2, 3, 4], [9, 8, 7, 6])], np.uint8)
HELD_OUT = np.array(_perm([0, 5, 10, 15], [1, 2, 3, 7]), np.uint8)
DISJOINT = np.array([list(range(16)), list(range(8, 16)) + list(range(8))], np.uint8)       # deal A plays cards 0-7, deal B cards 8-15


def _multi(ctx, sl, perms):
    perms = np.asarray(perms, np.uint8).reshape(-1, 16)
    m = sl.MultiDeal(ctx, len(perms))
    m.set_perms(perms)
    m.build()
    return m


def _six_ref(oracle, _cache={}):
    if not _cache:
        _cache["ref"] = ChanceMccfrRef([oracle.Tree(perm=p) for p in SIX])
        ref = _cache["ref"].ref
        assert (ref.G, ref.n_occ) == (3522, 3860)
        assert len(ref.shared_hand_sizes(0)) >= 3 and len(ref.shared_hand_sizes(1)) >= 3
    return _cache["ref"]


def _six_game(ctx, sl):
    g = sl.ChanceGame(_multi(ctx, sl, SIX))
    assert (g.n, g.G, g.n_occurrences) == (6, 3522, 3860)
    return g


def _start_tables(ref, name):
    if name == "zero":
        return ref.tables()
    return E.edge_table(name, ref.nlegal), (1.0 + np.arange(ref.G * 4, dtype=np.float64).reshape(-1, 4)) * ref.legal


def _in_budget(R_gpu, R_ref, A):
    """per global row, printed before it is asserted: the largest error in units of its budget"""
    bound = (E.K_REORDER * E.EPS * A.sum(1))[:, None] + 2.0 * E.EPS * np.abs(R_ref)
    err = np.abs(R_gpu - R_ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = np.where(err == 0.0, 0.0, err / bound).max()
    print("largest regret error / budget:", worst)
    return bool((err <= bound).all())


def _one_iteration(ref, R0, S0, batch, it, deals=None, seed=SEED):
    R, S = R0.copy(), S0.copy()
    A, visits, touched, vis = ref.iterate(R, S, batch, seed, it, deals)
    return R, S, A, visits, touched, vis


# ---- one iteration from given tables ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", ["zero", "onehot", "small_large"])
def test_one_iteration_from_given_tables(ctx, sl, oracle, table):
    ref = _six_ref(oracle)
    g = _six_game(ctx, sl)
    R0, S0 = _start_tables(ref, table)
    seen = [0, 0]
    for batch in (1, 37, 48):
        g.tables_set(R0, S0)
        it = g.mccfr_counters()[2]
        R, S, A, visits, touched, vis = _one_iteration(ref, R0, S0, batch, it)
        assert touched.all() and vis == (PAIR_VISITS[0] * batch * 6, PAIR_VISITS[1] * batch * 6)
        g.mccfr_iterate(batch, 1, SEED)
        Rg, Sg = g.tables_get()
        seen = [seen[0] + vis[0], seen[1] + vis[1]]
        assert g.mccfr_counters() == (seen[0], seen[1], it + 1), (table, batch)
        want_S = np.where(ref.legal, S0 + visits.astype(np.float64)[:, None] * E.reference_sigma(R0, ref.nlegal), S0)
        assert np.array_equal(S, want_S) and np.array_equal(Sg, want_S), (table, batch)
        assert np.isfinite(R).all() and _in_budget(Rg, R, A), (table, batch)
        assert np.array_equal(Rg[~ref.legal], R0[~ref.legal])


def test_iterations_under_a_wide_seed(ctx, sl, oracle):
    """a seed whose high key word is not zero, at the smallest batch: iteration 0 over all deals and iteration 1 over a list, each from the device's OWN
    tables (counts, strategy sums and counters exact, regrets in the budget); then both in one call on a fresh handle, held as the file holds every run
    of several iterations.  tests/test_chance_mccfr_ref.py::test_wide_seed_iterations_separate: the low key word alone gives other visit counts"""
    ref, seed, batch = _six_ref(oracle), W.WIDE_SEED, WORD_BATCH
    g = _six_game(ctx, sl)
    seen = [0, 0]
    for it, deals in enumerate((None, WORD_LIST)):
        R0, S0 = g.tables_get()
        assert g.mccfr_counters()[2] == it
        R, S, A, visits, touched, vis = _one_iteration(ref, R0, S0, batch, it, deals, seed=seed)
        g.mccfr_iterate(batch, 1, seed, None if deals is None else [deals])
        Rg, Sg = g.tables_get()
        seen = [seen[0] + vis[0], seen[1] + vis[1]]
        assert g.mccfr_counters() == (seen[0], seen[1], it + 1)
        assert np.array_equal(Sg, S) and _in_budget(Rg, R, A), (it, deals)
        assert np.array_equal(Rg[~touched].view(np.uint64), R0[~touched].view(np.uint64))
    g2 = _six_game(ctx, sl)
    g2.mccfr_iterate(batch, 2, seed)
    R, S = ref.tables()
    ref.run(R, S, batch, seed, 0, 2)
    Rg, Sg = g2.tables_get()
    np.testing.assert_allclose(Rg, R, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(Sg, S, rtol=1e-10, atol=1e-10)
    assert g2.mccfr_counters() == (2 * 6 * batch * PAIR_VISITS[0], 2 * 6 * batch * PAIR_VISITS[1], 2) and np.abs(Rg).max() > 0


# ---- anchors ----------------------------------------------------------------------------------------------------------------------------------
def test_one_deal_is_the_single_deal_solver_and_the_oracle(ctx, sl, oracle):
    perm = sl.deal_py_seed(42)
    g = sl.ChanceGame(_multi(ctx, sl, perm))
    _, mp = g.index()
    g.mccfr_iterate(48, 5, 321)
    Rg, Sg = g.tables_get()
    t = oracle.Tree(seed=42)
    I = t.n_infosets
    R, S, _ = t.tables()
    t.mccfr_batched(R, S, 321, 0, 5, 48)
    np.testing.assert_allclose(Rg[mp[0, :I]], R, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(Sg[mp[0, :I]], S, rtol=1e-10, atol=1e-10)
    assert g.mccfr_counters() == (463 * 48 * 5, 240 * 48 * 5, 5)
    ctx.set_deal(perm)
    ctx.mccfr_seed(321)
    ctx.mccfr_iterate(48, 5)
    R1, S1, _ = ctx.tables_get()
    np.testing.assert_allclose(Rg[mp[0, :I]], R1, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(Sg[mp[0, :I]], S1, rtol=1e-10, atol=1e-10)


def test_the_same_deal_twice_matches_the_restatement(ctx, sl, oracle):
    perm = sl.deal_py_seed(42)
    t = oracle.Tree(seed=42)
    ref = ChanceMccfrRef([t, t])
    g = sl.ChanceGame(_multi(ctx, sl, [perm, perm]))
    assert g.G == ref.G == t.n_infosets and g.n_occurrences == 2 * g.G
    R0, S0 = ref.tables()
    R, S, A, visits, touched, vis = _one_iteration(ref, R0, S0, 48, 0)
    g.mccfr_iterate(48, 1, SEED)
    Rg, Sg = g.tables_get()
    assert np.array_equal(Sg, S) and _in_budget(Rg, R, A) and g.mccfr_counters() == (vis[0], vis[1], 1)
    # the two copies draw independent traversals: the visits are not twice one copy's
    _, _, _, v1, _, _ = _one_iteration(ChanceMccfrRef([t]), R0, S0, 48, 0)
    assert not np.array_equal(visits, 2 * v1)
    ref.run(R, S, 48, SEED, 1, 2)
    g.mccfr_iterate(48, 2, SEED)
    Rg, Sg = g.tables_get()
    np.testing.assert_allclose(Rg, R, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(Sg, S, rtol=1e-10, atol=1e-10)


@pytest.mark.parametrize("order", [(0, 1), (1, 0)])
def test_deals_on_disjoint_cards(ctx, sl, oracle, order):
    perms = DISJOINT[list(order)]
    m = _multi(ctx, sl, perms)
    g = sl.ChanceGame(m)
    I0, I1 = (int(x) for x in m.n_infosets)
    assert g.G == I0 + I1 == g.n_occurrences
    _, mp = g.index()
    g.mccfr_iterate(48, 5, 321)
    m.mccfr_iterate(48, 5, 321)                                                              # the multi's own tables: not touched by the game
    Rg, Sg = g.tables_get()
    Rd, Sd, _, _ = m.tables_get(0)                                                           # deal 0: the ids [0, 48) of the per-deal solver
    np.testing.assert_allclose(Rg[mp[0, :I0]], Rd, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(Sg[mp[0, :I0]], Sd, rtol=1e-10, atol=1e-10)
    ref = ChanceMccfrRef([oracle.Tree(perm=p) for p in perms])                               # deal 1: the ids [48, 96)
    R, S = ref.tables()
    ref.run(R, S, 48, 321, 0, 5)
    np.testing.assert_allclose(Rg, R, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(Sg, S, rtol=1e-10, atol=1e-10)
    R1, S1, _, _ = m.tables_get(1)
    assert not np.allclose(Rg[mp[1, :I1]], R1)                                               # other ids, other traversals


# ---- lists --------------------------------------------------------------------------------------------------------------------------------------
def test_every_deal_listed_in_any_order_is_the_call_without_a_list(ctx, sl, oracle):
    ref = _six_ref(oracle)
    R0, S0 = _start_tables(ref, "onehot")
    R, S, A, visits, touched, vis = _one_iteration(ref, R0, S0, 37, 0)
    for deals in (None, [[0, 1, 2, 3, 4, 5]], [[5, 4, 3, 2, 1, 0]]):
        g = _six_game(ctx, sl)
        g.tables_set(R0, S0)
        g.mccfr_iterate(37, 1, SEED, deals)
        Rg, Sg = g.tables_get()
        assert np.array_equal(Sg, S), deals                                                  # counts and strategy sums: bit equal
        assert _in_budget(Rg, R, A), deals
        assert g.mccfr_counters() == (vis[0], vis[1], 1)


def test_three_of_six_deals(ctx, sl, oracle):
    ref = _six_ref(oracle)
    R0, S0 = _start_tables(ref, "small_large")
    deals = [4, 0, 3]
    listed = ref.listed_rows(deals)
    assert listed.any() and (~listed).any() and (ref.ref.count[listed] > 1).any()
    g = _six_game(ctx, sl)
    g.mccfr_iterate(5, 2, SEED)                                                              # the stamps of an earlier call must not count
    g.tables_set(R0, S0)
    R, S, A, visits, touched, vis = _one_iteration(ref, R0, S0, 48, 2, deals)
    assert np.array_equal(touched, listed)
    before = g.mccfr_counters()
    g.mccfr_iterate(48, 1, SEED, [deals])
    Rg, Sg = g.tables_get()
    assert g.mccfr_counters() == (before[0] + vis[0], before[1] + vis[1], 3) and vis == (463 * 48 * 3, 240 * 48 * 3)
    assert np.array_equal(Rg[~listed].view(np.uint64), R0[~listed].view(np.uint64)) and np.array_equal(Sg[~listed].view(np.uint64), S0[~listed].view(np.uint64))
    assert np.array_equal(Sg, S) and _in_budget(Rg, R, A)
    assert (Rg[listed] != R0[listed]).any()


def test_more_deals_than_compute_units(ctx, sl):
    """495 deals: more workgroups than a round, and with a list slot != deal id"""
    from scopa_amd.algorithms.chance import hidden_hand_deals, sample_deals
    m = _multi(ctx, sl, hidden_hand_deals(sl.deal_py_seed(42)[:4]))
    g = sl.ChanceGame(m)
    _, mp = g.index()
    g.mccfr_iterate(8, 1, SEED)
    R, S = g.tables_get()
    assert g.mccfr_counters() == (463 * 8 * 495, 240 * 8 * 495, 1) and np.isfinite(R).all()
    assert S[int(mp[0, 0])].sum() == 8 * 495                                                 # seat 0's first decision: one row, one visit per pair, sigma = 1/4
    np.testing.assert_allclose(S.sum(), 2 * 86 * 8 * 495, rtol=1e-12)                        # a sigma row sums to 1: every traverser visit counted once
    lists = sample_deals(495, 32, 0, 2, seed=3)
    assert (lists != np.arange(32)).any()
    listed = np.zeros(g.G, bool)
    for d in lists.ravel():
        listed[mp[d, :int(m.n_infosets[d])]] = True
    g.mccfr_iterate(8, 2, SEED, lists)
    R2, S2 = g.tables_get()
    assert (~listed).any() and np.array_equal(R2[~listed], R[~listed]) and np.array_equal(S2[~listed], S[~listed])
    assert g.mccfr_counters() == (463 * 8 * (495 + 64), 240 * 8 * (495 + 64), 3)
    np.testing.assert_allclose(S2.sum(), 2 * 86 * 8 * (495 + 64), rtol=1e-12)


# ---- continuation and mixing ----------------------------------------------------------------------------------------------------------------
def test_two_calls_are_one_run(ctx, sl):
    a, b = _six_game(ctx, sl), _six_game(ctx, sl)
    lists = np.array([[0, 2, 4], [1, 3, 5], [5, 0, 1], [2, 3, 4], [0, 1, 2], [3, 4, 5], [4, 2, 0], [1, 5, 3]], np.int32)
    a.mccfr_iterate(48, 5, SEED, lists[:5])
    a.mccfr_iterate(48, 3, SEED, lists[5:])
    b.mccfr_iterate(48, 8, SEED, lists)
    (Ra, Sa), (Rb, Sb) = a.tables_get(), b.tables_get()
    assert np.abs(Ra).max() > 0
    np.testing.assert_allclose(Ra, Rb, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(Sa, Sb, rtol=1e-10, atol=1e-10)
    assert a.mccfr_counters() == b.mccfr_counters() == (463 * 48 * 3 * 8, 240 * 48 * 3 * 8, 8)


def test_mccfr_and_cfr_iterations_mix_on_one_handle(ctx, sl):
    g = _six_game(ctx, sl)
    g.mccfr_iterate(48, 4, SEED, [[0, 1, 2], [3, 4, 5], [0, 2, 4], [1, 3, 5]])
    R, S = g.tables_get()
    assert np.abs(R).max() > 0
    fresh = _six_game(ctx, sl)
    fresh.tables_set(R, S)                                                                   # computes every sigma row from R
    g.cfr_iterate_weighted(1)                                                                # reads the sigma rows the MCCFR reduce left
    fresh.cfr_iterate_weighted(1)
    (R1, S1), (R2, S2) = g.tables_get(), fresh.tables_get()
    assert np.array_equal(R1, R2) and np.array_equal(S1, S2) and not np.array_equal(R1, R)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_tables_alone(ctx, sl):
    L = sl.lib()
    g = _six_game(ctx, sl)
    g.mccfr_iterate(16, 2, SEED)
    R, S = g.tables_get()
    state = g.mccfr_counters()
    assert np.abs(R).max() > 0

    def call(batch, deals=None, n_iters=None, m=None):
        d = None if deals is None else np.ascontiguousarray(deals, np.int32)
        n_iters = (1 if d is None else d.shape[0]) if n_iters is None else n_iters
        m = (0 if d is None else d.shape[1]) if m is None else m
        return L.scopa_chance_mccfr_iterate(g._h, n_iters, batch, SEED, m, sl._ptr(d))

    bad = {"batch = 0": call(0),
           "batch > 2^24": call((1 << 24) + 1),
           "n * batch > 2^32": call(1 << 30),
           "duplicate id": call(16, [[0, 1, 2], [3, 4, 3]]),
           "id = n": call(16, [[0, 1, 6]]),
           "id = -1": call(16, [[0, -1, 2]]),
           "m = 0": call(16, np.zeros((1, 1), np.int32), m=0),
           "m = n + 1": call(16, np.arange(7, dtype=np.int32)[None, :]),
           "n_iters < 0": call(16, n_iters=-1)}
    for what, rc in bad.items():
        assert rc == sl.SCOPA_EINVAL, what
        assert np.array_equal(g.tables_get()[0], R) and np.array_equal(g.tables_get()[1], S) and g.mccfr_counters() == state, what
    for kw in (dict(batch=0), dict(batch=1 << 30), dict(batch=16, deals=[[0, 1, 1]]), dict(batch=16, deals=[[0, 1, 6]])):
        with pytest.raises(sl.ScopaError) as e:
            g.mccfr_iterate(n_iters=1, seed=SEED, **kw)
        assert e.value.status == sl.SCOPA_EINVAL
    with pytest.raises(ValueError):
        g.mccfr_iterate(16, 2, SEED, [[0, 1, 2]])                                             # one list for two iterations
    assert call(16, n_iters=0) == sl.SCOPA_OK                                                 # n_iters = 0: SCOPA_OK and nothing moves
    g.mccfr_iterate(16, 0, SEED)
    assert np.array_equal(g.tables_get()[0], R) and np.array_equal(g.tables_get()[1], S) and g.mccfr_counters() == state
    g.mccfr_iterate(16, 1, SEED)                                                              # and the handle still works
    assert not np.array_equal(g.tables_get()[0], R) and g.mccfr_counters()[2] == 3


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------------
def test_solve_mccfr_lowers_exploitability(ctx, sl):
    from scopa_amd.algorithms import chance
    g, t, curve = chance.solve_mccfr(_multi(ctx, sl, SIX), 256, eps=0.0, max_iters=40, check_every=10, seed=11)
    assert t == 40 and [c[0] for c in curve] == [10, 20, 30, 40] and g.mccfr_counters()[2] == 40
    print("chance MCCFR, batch 256: exploitability at 10, 20, 30, 40 iterations:", [c[1] for c in curve])
    assert curve[-1][1] < curve[0][1]
    assert curve[-1][1] == g.exploitability()[0]
    I = ctx.set_deal(HELD_OUT)
    P = chance.table_for(ctx, chance.policy_by_key(g))
    nl = (ctx.tree_export()["infoset_key"].astype(np.int64) >> 1) & 7
    assert P.shape == (I, 4) and (P >= 0).all() and not P[np.arange(4)[None, :] >= nl[:, None]].any()
    np.testing.assert_allclose(P.sum(1), 1.0, rtol=0, atol=1e-12)
    assert np.isfinite(ctx.exploitability(P)["exploitability"])


def test_solve_mccfr_with_sampled_deals(ctx, sl):
    from scopa_amd.algorithms import chance
    g, t, curve = chance.solve_mccfr(_multi(ctx, sl, SIX), 64, eps=0.0, max_iters=20, check_every=10, sample=3, seed=7)
    assert t == 20 and [c[0] for c in curve] == [10, 20]
    assert g.mccfr_counters() == (463 * 64 * 3 * 20, 240 * 64 * 3 * 20, 20) and np.isfinite(curve[-1][1])
