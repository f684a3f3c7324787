"""The chance game's kernels (scopa_chance_*: k_chance_sweep, k_chance_reduce, k_chance_reduce_sampled, k_chance_reduce_mccfr, k_mccfr_chance, the
cross-deal exploitability, the Deep CFR traversal and key-table policy over a set of deals) at the deal sets of tests/chance_sets.py, where a row is
shared by up to 8, 70 and 495 deals and the deals' infoset counts differ by more than a factor of two, from edge tables, and under a lowered LDS
limit.  The other chance tests compare bit for bit on six deals only.

Every table comparison is np.array_equal, cfr_edges.same / same_bits (the project's rule for non-finite cells) or, for the regrets of an MCCFR
iteration, the reorder budget of tests/test_gpu_chance_mccfr.py (_in_budget).  The only absolute tolerance is the 1e-15 row-sum bound of the key-table
policy.  The references are tests/chance_ref.py, chance_sampled_ref.py and chance_mccfr_ref.py (each anchored to the C oracle by its own CPU test);
they are computed once per process, cached and never modified.  Each test asserts the figures of its set -- (n, G, occurrences) on the game, the
multiplicities on the reference -- before anything else, and (R1 != R0).any() after an iteration, so that nothing passes vacuously."""
import numpy as np
import pytest

import cfr_edges as E
import chance_sets as CS
import mccfr_edges as ME
from chance_mccfr_ref import PAIR_VISITS, ChanceMccfrRef
from test_gpu_chance_mccfr import SEED as MC_SEED, _in_budget
from test_gpu_chance_sdcfr import SENTINEL, World, _same as _same_rings

pytestmark = pytest.mark.gpu

N_DECISION = 1653
EDGE_W = np.array([[1.0, 0.5, 0.75]])
EDGE_CASES = tuple(E.CASES)
NINE_OF_25 = np.array([[0, 3, 4, 8, 11, 12, 17, 20, 24], [23, 19, 16, 13, 10, 7, 5, 2, 1]], np.int32)     # the second list descending
KB = 1024


def _game(ctx, sl, name):
    """the set's game, its (n, G, occurrences) asserted first"""
    f = CS.FIGURES[name]
    g = sl.ChanceGame(CS.multi(ctx, sl, name))
    assert (g.n, g.G, g.n_occurrences) == (f["n"], f["G"], f["n_occ"])
    return g


def _ref(oracle, name):
    r = CS.ref(oracle, name)
    CS.check_figures(r, name)
    return r


def _tables_equal(g, R, S):
    Rg, Sg = g.tables_get()
    return np.array_equal(Rg, R) and np.array_equal(Sg, S)


# ---- 1. index ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["BOTH25", "HIDDEN495"])
def test_index(ctx, sl, oracle, name):
    r = _ref(oracle, name)
    m = CS.multi(ctx, sl, name)
    assert np.array_equal(m.n_infosets, r.I)
    g = sl.ChanceGame(m)
    assert (g.n, g.G, g.n_occurrences) == (r.n, r.G, r.n_occ)
    keys, mp = g.index()
    assert keys.dtype == np.uint64 and mp.dtype == np.int32 and mp.shape == (r.n, N_DECISION)
    assert np.array_equal(keys, r.keys) and np.array_equal(mp, r.map)


# ---- 2. weighted CFR at multiplicity ------------------------------------------------------------------------------------------------------------
def _both25_tables(oracle, weighting, alternating, _cache={}):
    """the reference's tables after 1, 2 and 5 iterations on BOTH25, and out4 / policy of the average policy and of sigma(R) after 5"""
    key = (weighting, alternating)
    if key not in _cache:
        r, w = _ref(oracle, "BOTH25"), CS.weights(weighting, 5)
        R, S = r.tables()
        out, t = {}, 0
        for upto in (1, 2, 5):
            r.run(R, S, w[t:upto], alternating)
            t = upto
            out[upto] = (R.copy(), S.copy())
        P, given = r.average_policy(S), r.sigma(R)
        out["average"], out["given"] = (P, r.exploitability(P)), (given, r.exploitability(given))
        _cache[key] = out
    return _cache[key]


@pytest.mark.parametrize("alternating", [False, True])
@pytest.mark.parametrize("weighting", CS.WEIGHTINGS)
def test_both25_tables_and_exploitability(ctx, sl, oracle, weighting, alternating):
    r, want = _ref(oracle, "BOTH25"), _both25_tables(oracle, weighting, alternating)
    assert CS.histogram(r) == CS.BOTH25_HISTOGRAM
    w = CS.weights(weighting, 5)
    g = _game(ctx, sl, "BOTH25")
    R0, t = g.tables_get()[0], 0
    for upto in (1, 2, 5):
        g.cfr_iterate_weighted(w[t:upto], alternating)
        t = upto
        R, S = g.tables_get()
        assert (R != R0).any()
        assert np.array_equal(R, want[upto][0]) and np.array_equal(S, want[upto][1]), (weighting, alternating, upto)
        R0 = R
    out, pol = g.exploitability(return_policy=True)
    assert np.array_equal(pol, want["average"][0]) and np.array_equal(out, want["average"][1])
    out_g, pol_g = g.exploitability(want["given"][0], return_policy=True)
    assert np.array_equal(pol_g, want["given"][0]) and np.array_equal(out_g, want["given"][1])
    assert np.isfinite(want["average"][1]).all() and np.isfinite(want["given"][1]).all() and not np.array_equal(out, out_g)


def test_hidden495_tables_and_exploitability(ctx, sl, oracle):
    """the 495-term sums of k_chance_reduce, k_chance_xbr_choose and k_chance_xbr_sum"""
    r = _ref(oracle, "HIDDEN495")
    w = CS.weights("dcfr", 2)
    R, S = r.tables()
    r.run(R, S, w[:1], True)
    R1, S1 = R.copy(), S.copy()
    r.run(R, S, w[1:], True)
    g = _game(ctx, sl, "HIDDEN495")
    g.cfr_iterate_weighted(w[:1], True)
    assert (g.tables_get()[0] != 0).any() and _tables_equal(g, R1, S1)
    g.cfr_iterate_weighted(w[1:], True)
    assert (R != R1).any() and _tables_equal(g, R, S)
    P = r.average_policy(S)
    out, pol = g.exploitability(return_policy=True)
    want = r.exploitability(P)
    assert np.isfinite(want).all()
    assert np.array_equal(pol, P) and np.array_equal(out, want)


# ---- 3. edge tables through chance_apply and the policy kernels ------------------------------------------------------------------------------
def _edge_start(r, case):
    """(R, S) of a cfr_edges case over the global rows: its regret table and the strategy-sum kind the case is paired with (all four S_KINDS occur)"""
    r_name, s_kind, _ = E.CASES[case]
    if case == "nan_held":
        R, S, _ = E.tables(case, r.nlegal)
        return R, S
    return E.regret_table(r_name, r.nlegal), E.strategy_sum_table(s_kind, r.nlegal)


def _edge_want(oracle, case, alternating, _cache={}):
    """the reference after one and two full iterations from the case's tables (with out4 / policy of the average policy of each S), and after two
    sampled iterations over NINE_OF_25 from the same tables"""
    key = (case, alternating)
    if key not in _cache:
        r = _ref(oracle, "BOTH25")
        R0, S0 = _edge_start(r, case)
        R, S = R0.copy(), S0.copy()
        out = {}
        for it in (1, 2):
            r.run(R, S, EDGE_W, alternating)
            with np.errstate(invalid="ignore", over="ignore"):
                P = r.average_policy(S)
            out[it] = (R.copy(), S.copy(), P, r.exploitability(P))
        Rs, Ss = R0.copy(), S0.copy()
        r.run_sampled(Rs, Ss, NINE_OF_25, np.tile(EDGE_W, (2, 1)), alternating)
        out["sampled"] = (Rs, Ss)
        _cache[key] = out
    return _cache[key]


def _same_where_finite(case, got, want):
    """bit for bit where the reference is finite (everywhere on a finite case)"""
    fin = np.isfinite(want)
    if case not in E.NONFINITE_CASES:
        assert fin.all()
    return E.same_bits(np.asarray(got)[fin], np.asarray(want)[fin])


def test_edge_pairings_use_every_strategy_kind():
    assert {E.CASES[c][1] for c in EDGE_CASES} == set(E.S_KINDS) and set(E.FINITE_CASES + E.NONFINITE_CASES) <= set(EDGE_CASES)


@pytest.mark.parametrize("alternating", [False, True])
@pytest.mark.parametrize("case", EDGE_CASES)
def test_edge_tables(ctx, sl, oracle, case, alternating):
    r, want = _ref(oracle, "BOTH25"), _edge_want(oracle, case, alternating)
    assert CS.histogram(r) == CS.BOTH25_HISTOGRAM
    R0, S0 = _edge_start(r, case)
    assert not R0[~r.legal].any() and not S0[~r.legal].any()
    g = _game(ctx, sl, "BOTH25")
    g.tables_set(R0, S0)
    assert E.same_bits(g.tables_get()[0], R0) and E.same_bits(g.tables_get()[1], S0)
    for it in (1, 2):                                          # the second iteration's sweep reads the sigma rows the first reduce left
        g.cfr_iterate_weighted(EDGE_W, alternating)
        R, S = g.tables_get()
        Rw, Sw, P, out4 = want[it]
        assert not E.same_bits(Rw, R0 if it == 1 else want[1][0])
        assert E.same(case, R, Rw) and E.same(case, S, Sw), (case, alternating, it)
        assert E.same_bits(R[~r.legal], R0[~r.legal]) and E.same_bits(S[~r.legal], S0[~r.legal])
        out, pol = g.exploitability(return_policy=True)
        assert _same_where_finite(case, pol, P) and _same_where_finite(case, out, out4), (case, alternating, it)
        if case in E.FINITE_CASES:
            assert np.isfinite(out4).all()
    # the same start tables through the sampled reduce, 9 of the 25 deals per iteration
    for deals in NINE_OF_25:
        total, sampled, first_sampled = r.occurrence_stats(deals)
        assert ((sampled > 0) & (sampled < total)).any() and (~first_sampled & (sampled > 0)).any() and ((total > 1) & (sampled == 0)).any()
    g.tables_set(R0, S0)
    g.cfr_iterate_sampled(NINE_OF_25, np.tile(EDGE_W, (2, 1)), alternating)
    R, S = g.tables_get()
    assert not E.same_bits(want["sampled"][0], R0) and not E.same_bits(want["sampled"][0], want[2][0])
    assert E.same(case, R, want["sampled"][0]) and E.same(case, S, want["sampled"][1]), (case, alternating)
    assert E.same_bits(R[~r.legal], R0[~r.legal]) and E.same_bits(S[~r.legal], S0[~r.legal])


@pytest.mark.parametrize("alternating", [False, True])
def test_illegal_cells_keep_any_bits(ctx, sl, oracle, alternating):
    """cells past a row's legal count are neither read nor written: with a sentinel in them the legal cells are those of the clean tables"""
    r, want = _ref(oracle, "BOTH25"), _edge_want(oracle, "onehot", alternating)
    R0, S0 = _edge_start(r, "onehot")
    Rm, Sm = np.where(r.legal, R0, 7.5), np.where(r.legal, S0, -7.5)
    g = _game(ctx, sl, "BOTH25")
    for sampled in (False, True):
        g.tables_set(Rm, Sm)
        if sampled:
            g.cfr_iterate_sampled(NINE_OF_25, np.tile(EDGE_W, (2, 1)), alternating)
        else:
            g.cfr_iterate_weighted(np.tile(EDGE_W, (2, 1)), alternating)
        R, S = g.tables_get()
        Rw, Sw = want["sampled"] if sampled else want[2][:2]
        assert (R[~r.legal] == 7.5).all() and (S[~r.legal] == -7.5).all()
        assert E.same_bits(R[r.legal], Rw[r.legal]) and E.same_bits(S[r.legal], Sw[r.legal]) and not E.same_bits(Rw, R0)
    out, pol = g.exploitability(return_policy=True)
    P = r.average_policy(want["sampled"][1])
    assert E.same_bits(pol, P) and np.array_equal(out, r.exploitability(P))


# ---- 4. sampled CFR at the benchmark's sizes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", CS.SAMPLE_SIZES)
def test_hidden495_sampled_then_full(ctx, sl, oracle, m):
    r = _ref(oracle, "HIDDEN495")
    lists = CS.sampled_lists(m)
    assert CS.check_sampled_lists(r, lists)                   # the 495-fold row: some but not all occurrences; a shared row without any
    w = CS.weights("cfr+", CS.SAMPLE_ITERS + 1)
    R, S = r.tables()
    r.run_sampled(R, S, lists, w[:CS.SAMPLE_ITERS], True)
    Rs, Ss = R.copy(), S.copy()
    r.run(R, S, w[CS.SAMPLE_ITERS:], True)
    g = _game(ctx, sl, "HIDDEN495")
    g.cfr_iterate_sampled(lists, w[:CS.SAMPLE_ITERS], True)
    assert (Rs != 0).any() and _tables_equal(g, Rs, Ss)
    g.cfr_iterate_weighted(w[CS.SAMPLE_ITERS:], True)          # stale stamps and the compact image leave nothing behind
    assert (R != Rs).any() and _tables_equal(g, R, S)


# ---- 5. MCCFR at multiplicity -------------------------------------------------------------------------------------------------------------------
def test_hidden70_mccfr(ctx, sl, oracle):
    full = _ref(oracle, "HIDDEN70")
    ref = ChanceMccfrRef(full)
    big = int(np.argmax(full.I))
    deals = sorted({0, big} | set(range(3, 70, 5)))            # 16 of 70, with deal 0 and the deal of the most infosets
    assert len(deals) == 16 and 0 in deals and big in deals and big != 0
    R0 = ME.edge_table("small_large", ref.nlegal)
    S0 = (1.0 + np.arange(ref.G * 4, dtype=np.float64).reshape(-1, 4)) * ref.legal
    R, S = R0.copy(), S0.copy()
    A, visits, touched, vis = ref.iterate(R, S, 8, MC_SEED, 0)
    assert touched.all() and vis == (PAIR_VISITS[0] * 8 * 70, PAIR_VISITS[1] * 8 * 70) and visits.max() == 8 * 70
    R1, S1 = R.copy(), S.copy()
    A2, visits2, touched2, vis2 = ref.iterate(R, S, 8, MC_SEED, 1, deals)
    listed = ref.listed_rows(deals)
    assert np.array_equal(touched2, listed) and listed.any() and (~listed).any() and (full.count[listed] > len(deals)).any()
    assert np.isfinite(R).all()
    g = _game(ctx, sl, "HIDDEN70")
    g.tables_set(R0, S0)
    g.mccfr_iterate(8, 1, MC_SEED)
    Rg, Sg = g.tables_get()
    assert (Rg != R0).any() and g.mccfr_counters() == (vis[0], vis[1], 1)
    assert np.array_equal(Sg, S1) and _in_budget(Rg, R1, A)
    g.tables_set(R1, S1)                                        # the second iteration from the reference's tables: one iteration's budget
    g.mccfr_iterate(8, 1, MC_SEED, [deals])
    Rg, Sg = g.tables_get()
    assert g.mccfr_counters() == (vis[0] + vis2[0], vis[1] + vis2[1], 2) and vis2 == (PAIR_VISITS[0] * 8 * 16, PAIR_VISITS[1] * 8 * 16)
    assert E.same_bits(Rg[~listed], R1[~listed]) and E.same_bits(Sg[~listed], S1[~listed])
    assert (Rg[listed] != R1[listed]).any() and np.array_equal(Sg, S) and _in_budget(Rg, R, A2)


# ---- 6. LDS routes ----------------------------------------------------------------------------------------------------------------------------
# The host's sizes (scopa_chance.hip: sweep_lds; scopa_mccfr.hip: multi_lds_bytes, kStaticLdsMulti, sizeof(WaveScratch)), restated for the derivation
def _sweep_lds(max_infosets):
    return max_infosets * 4 * 8 + 8 * 2229 * 3 + 1656 * 2 * 2


def _mccfr_lds(max_infosets, waves):
    wave_scratch = 168 * 4 + 128 + 64 * 16
    b = ((max_infosets + 1) * 6 + max_infosets * 4) * 8 + waves * wave_scratch
    b += ((max_infosets * 4 + 15) & ~15) + 1656 * 2 + 576 + max_infosets
    return ((b + 15) & ~15) + 64 + 15 * 1024


def _raises_elimit(sl, call):
    with pytest.raises(sl.ScopaError) as e:
        call()
    assert e.value.status == sl.SCOPA_ELIMIT and "LDS" in str(e.value), str(e.value)


def test_refusals_under_a_64_kb_limit(ctx, sl, oracle):
    """BOTH25's largest deal has 1 008 infosets: sweep_lds = 92 376 bytes and the MCCFR walk needs 106 864 bytes with ONE wavefront, both above 64 KB"""
    r = _ref(oracle, "BOTH25")
    assert _sweep_lds(max(r.I)) > 64 * KB and _mccfr_lds(max(r.I), 1) > 64 * KB
    m = CS.multi(ctx, sl, "BOTH25")
    g = sl.ChanceGame(m)
    g.cfr_iterate_weighted(CS.weights("dcfr", 1))
    g.mccfr_iterate(4, 1, MC_SEED)
    R, S = g.tables_get()
    state = g.mccfr_counters()
    assert (R != 0).any() and state[2] == 1
    try:
        ctx.debug_lds_limit(64 * KB)
        _raises_elimit(sl, lambda: sl.ChanceGame(m))
        for call in (lambda: g.cfr_iterate_weighted(CS.weights("dcfr", 1)), lambda: g.cfr_iterate_weighted(CS.weights("dcfr", 1), True),
                     lambda: g.cfr_iterate_sampled(NINE_OF_25), lambda: g.mccfr_iterate(4, 1, MC_SEED), lambda: g.mccfr_iterate(4, 2, MC_SEED, NINE_OF_25)):
            _raises_elimit(sl, call)
            assert E.same_bits(g.tables_get()[0], R) and E.same_bits(g.tables_get()[1], S) and g.mccfr_counters() == state
    finally:
        ctx.debug_lds_limit(0)
    g.cfr_iterate_weighted(CS.weights("dcfr", 1))               # and the handle still works under the device's own limit
    assert not E.same_bits(g.tables_get()[0], R)


def test_fewer_wavefronts_under_a_128_kb_limit(ctx, sl, oracle):
    """launch_mccfr_chance starts from 16 wavefronts and drops two at a time until multi_lds_bytes + kStaticLdsMulti fits.  For BOTH25's
    max_infosets = 1 008 that sum is 134 224 bytes with 16 wavefronts and 130 576 with 14, so under 128 KB = 131 072 bytes the walk runs with 14
    wavefronts (896 threads).  sweep_lds(1 008) = 92 376 <= 131 072: the three CFR calls RUN, with the reference's bits."""
    r = _ref(oracle, "BOTH25")
    limit = 128 * KB
    assert _mccfr_lds(max(r.I), 16) == 134224 > limit >= _mccfr_lds(max(r.I), 14) == 130576 and _sweep_lds(max(r.I)) == 92376 <= limit
    ref = ChanceMccfrRef(r)
    want = _both25_tables(oracle, "dcfr", True)
    w = CS.weights("dcfr", 2)
    R0 = ME.edge_table("onehot", ref.nlegal)
    S0 = (1.0 + np.arange(ref.G * 4, dtype=np.float64).reshape(-1, 4)) * ref.legal
    R, S = R0.copy(), S0.copy()
    A, visits, touched, vis = ref.iterate(R, S, 37, MC_SEED, 0)
    Rs, Ss = r.tables()
    r.run_sampled(Rs, Ss, NINE_OF_25, w, False)
    try:
        ctx.debug_lds_limit(limit)
        g = _game(ctx, sl, "BOTH25")
        g.tables_set(R0, S0)
        g.mccfr_iterate(37, 1, MC_SEED)                         # 37 pairs over 14 wavefronts: ragged
        Rg, Sg = g.tables_get()
        assert (Rg != R0).any() and touched.all() and g.mccfr_counters() == (vis[0], vis[1], 1)
        assert np.array_equal(Sg, S) and _in_budget(Rg, R, A)
        g.tables_reset()
        g.cfr_iterate_weighted(w, True)
        assert _tables_equal(g, *want[2])
        g.tables_reset()
        g.cfr_iterate_sampled(NINE_OF_25, w, False)
        assert (Rs != 0).any() and _tables_equal(g, Rs, Ss)
    finally:
        ctx.debug_lds_limit(0)


# ---- 7. Deep CFR over keys at multiplicity ------------------------------------------------------------------------------------------------------
class World70(World):
    """test_gpu_chance_sdcfr.World on HIDDEN70, with per-deal contexts for five deals only"""

    def __init__(self, sl):
        import torch
        from test_gpu_chance_sdcfr import SEED
        self.sl, self.torch = sl, torch
        self.stream = torch.cuda.Stream(device=0)
        self.ctx = sl.Context(0, stream=self.stream.cuda_stream)
        self.ctx.mccfr_seed(SEED)
        self.multi = CS.multi(self.ctx, sl, "HIDDEN70")
        self.game = sl.ChanceGame(self.multi)
        I = self.multi.n_infosets
        small, big = int(np.argmin(I)), int(np.argmax(I))
        self.deals = [d for d in dict.fromkeys([big, 0, small, 33, 52, 17])][:5]        # deal 0 is itself the smallest here: a third "other" deal
        assert len(self.deals) == 5 and {0, small, big} <= set(self.deals) and I[small] < I[big]
        self.deal_ctx = {}
        for d in self.deals:
            c = sl.Context(0)
            c.mccfr_seed(SEED)
            assert c.set_deal(np.ascontiguousarray(CS.HIDDEN70[d])) == I[d]
            self.deal_ctx[d] = c
        gen = torch.Generator().manual_seed(20240611)
        self.nets = [self.random_net(gen) for _ in range(2)]
        self.image = torch.zeros((2, sl.lib().scopa_sdcfr_image_floats()), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        for p, net in enumerate(self.nets):
            self.ctx.sdcfr_pack_weights(p, *(t.data_ptr() for t in net), self.image.data_ptr())
        self.ctx.synchronize()

    def close(self):
        for c in self.deal_ctx.values():
            c.close()
        self.ctx.close()


@pytest.fixture(scope="module")
def world70(sl):
    try:
        w = World70(sl)
    except sl.ScopaError as e:
        if e.status == sl.SCOPA_ENODEV:
            pytest.skip("no GPU on this box")
        raise
    f = CS.FIGURES["HIDDEN70"]
    assert (w.game.n, w.game.G, w.game.n_occurrences) == (f["n"], f["G"], f["n_occ"])
    yield w
    w.close()


@pytest.mark.parametrize("traverser", [0, 1])
def test_hidden70_sdcfr_rows_equal_single_deal_calls(world70, traverser):
    deals, batch = world70.deals, 13
    capacity, write_base = 41 * len(deals) * batch + 50, 17
    got = world70.chance_call(traverser, batch, deals, capacity, write_base, True)
    exp = world70.single_calls(traverser, batch, deals, capacity, write_base, True)
    assert (exp[0][write_base:write_base + 41 * len(deals) * batch] != SENTINEL).all() and (exp[3] != SENTINEL).all()
    assert _same_rings(got, exp)
    assert (got[0][:write_base] == SENTINEL).all() and (got[1][write_base + 41 * len(deals) * batch:] == SENTINEL).all()


def test_hidden70_average_policy_over_keys(world70):
    torch, w = world70.torch, world70
    keys, mp = w.game.index()
    nl = ((keys >> np.uint64(1)) & np.uint64(7)).astype(np.int64)
    count = np.bincount(mp[mp >= 0], minlength=w.game.G)
    root = int(mp[0, 0])
    assert count[root] == 70 and (mp[:, 0] == root).all() and w.deals[0] != 0      # the 70-fold key's first occurrence is deal 0's: another deal is compared
    gen = torch.Generator().manual_seed(99)
    nets = [w.random_net(gen, scale=1.0 + 0.2 * s) for s in range(5)]
    store = [torch.stack([n[i] for n in nets]).contiguous() for i in range(6)]
    d_slots = torch.tensor([4, 0, 2], dtype=torch.int32, device="cuda:0")
    d_coef = torch.tensor([0.5, 0.3, 0.2], dtype=torch.float32, device="cuda:0")
    ptrs = [t.data_ptr() for t in store]
    out_G = torch.full((w.game.G, 4), float("nan"), dtype=torch.float64, device="cuda:0")
    local = {d: torch.full((c.n_infosets, 4), float("nan"), dtype=torch.float64, device="cuda:0") for d, c in w.deal_ctx.items()}
    torch.cuda.synchronize()
    for p in (0, 1):
        w.game.sdcfr_average_policy(p, 3, ptrs, 5, d_slots.data_ptr(), d_coef.data_ptr(), out_G.data_ptr())
        for d, c in w.deal_ctx.items():
            c.sdcfr_average_policy(p, 3, ptrs, 5, d_slots.data_ptr(), d_coef.data_ptr(), local[d].data_ptr())
            c.synchronize()
    w.ctx.synchronize()
    G = out_G.cpu().numpy()
    assert not np.isnan(G).any()                                                    # defined on every row
    for d, c in w.deal_ctx.items():
        I = c.n_infosets
        assert (mp[d, :I] >= 0).all() and (mp[d, I:] == -1).all()
        assert np.array_equal(G[mp[d, :I]], local[d].cpu().numpy()), d
    legal = np.arange(4)[None, :] < nl[:, None]
    assert (G[~legal] == 0.0).all() and np.abs(G.sum(1) - 1.0).max() <= 1e-15
    assert not np.array_equal(G, np.where(legal, 1.0 / nl[:, None], 0.0))
