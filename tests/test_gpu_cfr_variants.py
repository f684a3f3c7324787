"""k_cfr_sync_weighted (scopa_cfr_sync_iterate_weighted, scopa_multi_cfr_sync_iterate_weighted) and what is built on it -- CFRTrainer's
variants, MultiDeal.solve -- on the GPU.

The kernel is held BIT FOR BIT to tests/cfr_variants_ref.py (a float64 numpy restatement that tests/test_cfr_variants_ref.py anchors to the C
oracle): both receive the same weight rows, so nothing but IEEE add, multiply and divide sits between them.  Tables are compared as uint64 views
(cfr_edges.same_bits); in the NaN case the finite cells bit for bit and the others by kind (cfr_edges.same).

k_cfr_sync has one launch route -- under a scopa_debug_lds_limit its tables do not fit the call returns SCOPA_ELIMIT -- and so has the weighted
kernel: there is no narrow route to reach, and the refusal is what is tested.  The multi-deal ABI has no getter for a single deal's first-visit
marks or counters: the inactive deals are checked through their tables and through the exact total of the counters."""
import numpy as np
import pytest

import cfr_edges as E
from cfr_variants_ref import Ref

pytestmark = pytest.mark.gpu

N_DECISION, N_TERMINAL = 1653, 576
KB64 = 64 * 1024
VARIANTS = ("vanilla", "cfr+", "linear", "dcfr")


def _schedule(*a, **k):
    from scopa_amd.algorithms import schedule
    return schedule(*a, **k)


def _tree(oracle, deal, _cache={}):
    if deal not in _cache:
        t = oracle.Tree(seed=deal)
        _cache[deal] = (t, Ref(t))
    return _cache[deal]


def _deal(ctx, sl, oracle, deal):
    t, ref = _tree(oracle, deal)
    assert ctx.set_deal(sl.deal_py_seed(deal)) == t.n_infosets
    assert [sl.key_to_string(k) for k in ctx.tree_export()["infoset_key"]] == t.infoset_strings
    return t, ref


def _game(seed=42):
    from scopa_amd.envs.openspiel_mini_scopa import MiniScopaGame
    return MiniScopaGame(seed=seed)


# ---- bits against the reference -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alternating", [False, True])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("deal", [42, 7])
def test_bits_against_the_reference(ctx, sl, oracle, deal, variant, alternating):
    """Each schedule in both forms, split 1 + 4 + 20 with the schedule continued, from zeroed tables: R and S bit for bit after every part,
    local_strategy untouched, counters exact (an alternating iteration counts two sweeps), every infoset marked as first seen by a batched launch."""
    t, ref = _deal(ctx, sl, oracle, deal)
    ctx.tables_reset()
    R, S, L = t.tables()
    t0, sweeps = 0, 2 if alternating else 1
    assert not ctx.visited_get().any()
    for k in (1, 4, 20):
        w = _schedule(variant, t0, k)
        c0 = ctx.counters()
        ctx.cfr_sync_iterate_weighted(w, alternating)
        ref.run(R, S, w, alternating)
        t0 += k
        Rg, Sg, Lg = ctx.tables_get()
        assert E.same_bits(Rg, R) and E.same_bits(Sg, S) and E.same_bits(Lg, L), (deal, variant, alternating, t0)
        c1 = ctx.counters()
        assert (c1[0] - c0[0], c1[1] - c0[1]) == (N_DECISION * k * sweeps, N_TERMINAL * k * sweeps)
        assert np.array_equal(ctx.visited_get(), 0x40000000 + np.arange(t.n_infosets, dtype=np.uint32))
    c0 = ctx.counters()
    ctx.cfr_sync_iterate_weighted(np.zeros((0, 3)), alternating)                    # no iterations: SCOPA_OK and nothing moves
    assert ctx.counters() == c0 and E.same_bits(ctx.tables_get()[0], R)


def test_refused_under_an_lds_limit_its_tables_do_not_fit(ctx, sl, oracle):
    """The 738-infoset deal needs 104 KB of LDS: under a 64 KB limit the weighted call returns SCOPA_ELIMIT before any launch, as
    scopa_cfr_sync_iterate does, and leaves tables and counters alone; with the limit restored it matches the reference."""
    t, ref = _deal(ctx, sl, oracle, 42)
    R, S, L = E.tables("small_large", t.infoset_nlegal)
    ctx.tables_reset()
    ctx.tables_set(regret=R, strategy=S, local=L)
    w = _schedule("dcfr", 0, 3)
    try:
        ctx.debug_lds_limit(KB64)
        c0 = ctx.counters()
        with pytest.raises(sl.ScopaError) as e:
            ctx.cfr_sync_iterate_weighted(w)
        assert e.value.status == sl.SCOPA_ELIMIT
        assert ctx.counters() == c0
        assert all(E.same_bits(a, b) for a, b in zip(ctx.tables_get(), (R, S, L)))
    finally:
        ctx.debug_lds_limit(0)
    ctx.cfr_sync_iterate_weighted(w)
    ref.run(R, S, w)
    Rg, Sg, _ = ctx.tables_get()
    assert E.same_bits(Rg, R) and E.same_bits(Sg, S)


# ---- bits against the existing kernel -------------------------------------------------------------------------------------------------
def test_unit_weights_are_the_unweighted_kernel(ctx, sl, oracle):
    """From the tables 3 exact-CFR iterations leave: weights (1, 1, 1), simultaneous, on a second context give the bits scopa_cfr_sync_iterate gives
    on the first -- all three tables, first-visit marks of the fresh infosets aside, counters."""
    t, _ = _deal(ctx, sl, oracle, 42)
    ctx.tables_reset()
    ctx.cfr_exact_iterate(3)
    start = ctx.tables_get()
    other = sl.Context(0)
    try:
        assert other.set_deal(sl.deal_py_seed(42)) == t.n_infosets
        other.tables_set(*start)
        ca, cb = ctx.counters(), other.counters()
        ctx.cfr_sync_iterate(2); ctx.cfr_sync_iterate(5)
        other.cfr_sync_iterate_weighted(np.ones((2, 3))); other.cfr_sync_iterate_weighted(np.ones((5, 3)), False)
        for a, b in zip(ctx.tables_get(), other.tables_get()):
            assert E.same_bits(a, b)
        assert not E.same_bits(ctx.tables_get()[0], start[0])
        da, db = ctx.counters(), other.counters()
        assert (da[0] - ca[0], da[1] - ca[1]) == (db[0] - cb[0], db[1] - cb[1]) == (7 * N_DECISION, 7 * N_TERMINAL)
    finally:
        other.close()


# ---- edge tables ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alternating", [False, True])
@pytest.mark.parametrize("case", ["allneg", "nan_held", "onehot", "small_large", "subnormal"])
def test_edge_tables_follow_the_select(ctx, sl, oracle, case, alternating):
    """Negative regrets (and -0.0) under neg = 0, a NaN regret (it fails `R <= 0`, takes the pos weight and stays NaN; its row plays uniform), exact
    zeros, 1e-9 next to 1e6 and subnormals, under CFR+ (neg = 0) and DCFR with beta = -inf and 0.5: reference == GPU after 1 + 3 iterations."""
    t, ref = _deal(ctx, sl, oracle, 42)
    for w in (_schedule("cfr+", 0, 4), _schedule("dcfr", 2, 4, beta=-np.inf), _schedule("dcfr", 0, 4, alpha=2.0, beta=0.5, gamma=3.0)):
        R, S, L = E.tables(case, t.infoset_nlegal)
        ctx.tables_reset()
        ctx.tables_set(regret=R, strategy=S, local=L)
        ctx.cfr_sync_iterate_weighted(w[:1], alternating)
        ctx.cfr_sync_iterate_weighted(w[1:], alternating)
        ref.run(R, S, w, alternating)
        Rg, Sg, Lg = ctx.tables_get()
        assert E.same(case, Rg, R) and E.same(case, Sg, S) and E.same_bits(Lg, L), (case, alternating, w[0])
        if case == "nan_held":
            assert np.isnan(Rg).any() and np.isfinite(Rg).sum() > Rg.size // 2


@pytest.mark.parametrize("n", [9, 10])
def test_from_the_references_own_edge_tables(ctx, sl, oracle, golden, n):
    """Start tables from tests/golden/vanilla_cfr_edges.npz: what the reference's CFRTrainer held after 3 iterations from the allneg and the
    nan_held tables on the seed-42 deal (cases 9 and 10); CFR+ and alternating DCFR, 1 + 4 iterations."""
    g, meta = E.fixture(golden.dir)
    case = meta[n]["case"]
    assert meta[n]["deal"] == 42 and case in ("allneg", "nan_held")
    t, ref = _deal(ctx, sl, oracle, 42)
    for variant, alternating in (("cfr+", False), ("dcfr", True)):
        R, S, L = g[f"c{n}_regret"].copy(), g[f"c{n}_strategy"].copy(), g[f"c{n}_local"].copy()
        ctx.tables_reset()
        ctx.tables_set(regret=R, strategy=S, local=L)
        w = _schedule(variant, 3, 5)
        ctx.cfr_sync_iterate_weighted(w[:1], alternating)
        ctx.cfr_sync_iterate_weighted(w[1:], alternating)
        ref.run(R, S, w, alternating)
        Rg, Sg, _ = ctx.tables_get()
        assert E.same(case, Rg, R) and E.same(case, Sg, S), (case, variant)


# ---- multi-deal -----------------------------------------------------------------------------------------------------------------------
def test_multi_deal_matches_the_reference_and_respects_the_mask(ctx, sl, oracle):
    """64 deals (py seeds 0..63): DCFR 1 + 4 iterations on all of them, per deal bit for bit against the reference; then alternating CFR+ with every
    second deal inactive -- the inactive deals' tables keep their bits, the active ones match the reference continued, and the counters' total
    is exactly the active deals' visits (nothing counted for an inactive deal)."""
    n = 64
    m = sl.MultiDeal(ctx, n)
    try:
        m.deal_py_seeds(np.arange(n))
        ninf = m.build()
        refs = [_tree(oracle, s) for s in range(n)]
        assert list(ninf) == [t.n_infosets for t, _ in refs]
        w = _schedule("dcfr", 0, 5)
        m.cfr_sync_iterate_weighted(w[:1])
        m.cfr_sync_iterate_weighted(w[1:], False, None)
        tables = []
        for i, (t, ref) in enumerate(refs):
            R, S, L = t.tables()
            ref.run(R, S, w)
            Rg, Sg, Lg, _ = m.tables_get(i)
            assert E.same_bits(Rg, R) and E.same_bits(Sg, S) and E.same_bits(Lg, L), i
            tables.append((R, S))
        assert m.counters() == (5 * N_DECISION * n, 5 * N_TERMINAL * n)
        active = np.arange(n) % 2 == 0
        w2 = _schedule("cfr+", 5, 3)
        m.cfr_sync_iterate_weighted(w2, True, active)
        for i, (t, ref) in enumerate(refs):
            R, S = tables[i]
            if active[i]:
                ref.run(R, S, w2, True)
            Rg, Sg, _, _ = m.tables_get(i)
            assert E.same_bits(Rg, R) and E.same_bits(Sg, S), (i, bool(active[i]))
        k = int(active.sum())
        assert m.counters() == ((5 * n + 2 * 3 * k) * N_DECISION, (5 * n + 2 * 3 * k) * N_TERMINAL)
        c = m.counters()
        m.cfr_sync_iterate_weighted(w2, False, np.zeros(n, np.uint8))                # nobody active: nothing moves
        assert m.counters() == c and E.same_bits(m.tables_get(0)[0], tables[0][0])
    finally:
        m.close()


def test_masked_call_leaves_inactive_deals_as_built(ctx, sl, oracle):
    """What the mask leaves alone, seen through a solver that depends on it: after a masked weighted call the exact solver still runs on every deal
    and gives, on the inactive ones, exactly the oracle's tables from zero (their tables were never touched)."""
    n = 6
    m = sl.MultiDeal(ctx, n)
    try:
        m.deal_py_seeds(np.arange(n))
        m.build()
        active = np.array([1, 0, 1, 0, 0, 1], np.uint8)
        m.cfr_sync_iterate_weighted(_schedule("linear", 0, 4), False, active)
        assert m.counters() == (4 * 3 * N_DECISION, 4 * 3 * N_TERMINAL)
        m.cfr_exact_iterate(2)
        for i in np.flatnonzero(active == 0):
            t, _ = _tree(oracle, int(i))
            R, S, L = t.tables()
            t.cfr_exact(R, S, L, 2)
            Rg, Sg, Lg, _ = m.tables_get(int(i))
            assert E.same_bits(Rg, R) and E.same_bits(Sg, S) and E.same_bits(Lg, L), i
    finally:
        m.close()


# ---- trainer --------------------------------------------------------------------------------------------------------------------------
def test_trainer_variants_converge_and_continue(sl, oracle):
    from scopa_amd.algorithms import CFRTrainer
    game = _game()
    a = CFRTrainer(game, mode="sync", variant="dcfr")
    a.train(200)
    ea = a.exploitability()
    print(f"dcfr, 200 iterations: {ea:.4e}")
    assert ea < 1e-4
    b = CFRTrainer(game, mode="sync", variant="dcfr")
    b.train(100); b.train(100)                                                     # the trainer owns t across calls
    c = CFRTrainer(game, mode="sync", variant="dcfr")
    hist = c.train(200, eval_interval=40, compute_exploitability=True)             # ... and across the exploitability chunks
    assert [h[0] for h in hist] == [40, 80, 120, 160, 200] and hist[-1][1] == ea
    Ta = a._engine.ctx.tables_get()
    for other in (b, c):
        assert all(E.same_bits(x, y) for x, y in zip(Ta, other._engine.ctx.tables_get()))
    t, ref = _tree(oracle, 42)
    R, S, _ = t.tables()
    ref.run(R, S, _schedule("dcfr", 0, 200))
    assert E.same_bits(Ta[0], R) and E.same_bits(Ta[1], S)
    assert set(a.info_set_map) == set(t.infoset_strings)
    p = CFRTrainer(game, mode="sync", variant="cfr+")
    p.train(200)
    print(f"cfr+, 200 iterations: {p.exploitability():.4e}")
    assert p.exploitability() < 1e-3
    alt = CFRTrainer(game, mode="sync", variant="dcfr", alternating=True)
    alt.train(50)
    R, S, _ = t.tables()
    ref.run(R, S, _schedule("dcfr", 0, 50), True)
    assert E.same_bits(alt._engine.ctx.tables_get()[0], R)
    for tr in (a, b, c, p, alt):
        tr._engine.close()


def test_trainer_without_a_variant_is_unchanged_and_exact_mode_refuses_one(sl, oracle):
    from scopa_amd.algorithms import CFRTrainer
    game = _game()
    tr = CFRTrainer(game, mode="sync", variant=None)
    tr.train(30)
    t, _ = _tree(oracle, 42)
    R, S, _ = t.tables()
    t.cfr_sync(R, S, 30)
    Rg, Sg, _ = tr._engine.ctx.tables_get()
    assert E.same_bits(Rg, R) and E.same_bits(Sg, S)
    tr._engine.close()
    with pytest.raises(ValueError):
        CFRTrainer(game, mode="exact", variant="dcfr")
    with pytest.raises(ValueError):
        CFRTrainer(game, variant="cfr+")                                            # mode defaults to "exact"
    with pytest.raises(ValueError):
        CFRTrainer(game, mode="sync", variant="cfr++")


# ---- MultiDeal.solve ------------------------------------------------------------------------------------------------------------------
def test_solve_stops_each_deal_at_its_own_iteration(ctx, sl):
    """256 deals, eps 1e-3, check_every 10, at most 400 iterations: every deal ends below eps or at max_iters, the counts are multiples of 10, a deal
    that stopped early was not run further (the counters' total is the counts' sum), and DCFR needs fewer iterations on average than vanilla."""
    n, eps, cap = 256, 1e-3, 400
    used = {}
    for variant in ("dcfr", "vanilla"):
        m = sl.MultiDeal(ctx, n)
        try:
            m.deal_py_seeds(np.arange(n))
            m.build()
            u = m.solve(variant, eps, cap, check_every=10)
            expl = m.exploitability()[:, 0]
            assert u.shape == (n,) and (u % 10 == 0).all() and (u >= 10).all() and (u <= cap).all()
            assert ((expl < eps) | (u == cap)).all()
            assert m.counters() == (int(u.sum()) * N_DECISION, int(u.sum()) * N_TERMINAL)
            used[variant] = u
            print(f"{variant}: mean {u.mean():.1f} iterations, max {u.max()}, {int((u == cap).sum())} deals at the cap, worst exploitability {expl.max():.3e}")
        finally:
            m.close()
    assert used["dcfr"].mean() < used["vanilla"].mean()


# ---- argument checks ------------------------------------------------------------------------------------------------------------------
def test_argument_checks(ctx, sl, oracle):
    L = sl.lib()
    ok = np.ones((2, 3))

    def rc(w, n=2, alternating=0):
        return L.scopa_cfr_sync_iterate_weighted(ctx._h, n, sl._ptr(w), alternating)

    assert rc(ok) == sl.SCOPA_ESTATE                                                # no deal yet
    _deal(ctx, sl, oracle, 282)
    before = ctx.tables_get()
    c0 = ctx.counters()
    for bad in (1.5, -0.1, float("nan"), float("inf"), -float("inf")):
        for col in range(3):
            w = ok.copy(); w[1, col] = bad
            assert rc(w) == sl.SCOPA_EINVAL, (bad, col)
    assert rc(ok, alternating=2) == sl.SCOPA_EINVAL and rc(ok, alternating=-1) == sl.SCOPA_EINVAL
    assert rc(None) == sl.SCOPA_EINVAL and rc(ok, n=-1) == sl.SCOPA_EINVAL and rc(ok, n=(1 << 20) + 1) == sl.SCOPA_EINVAL
    assert rc(ok, n=0) == sl.SCOPA_OK
    assert ctx.counters() == c0 and all(E.same_bits(a, b) for a, b in zip(before, ctx.tables_get()))
    assert rc(np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 1.0]])) == sl.SCOPA_OK          # the ends of the range are weights
    m = sl.MultiDeal(ctx, 3)
    try:
        def mrc(w, n=2, alternating=0, active=None):
            return L.scopa_multi_cfr_sync_iterate_weighted(m._h, n, sl._ptr(w), alternating, sl._ptr(active))
        assert mrc(ok) == sl.SCOPA_ESTATE                                           # not built
        m.deal_py_seeds([1, 2, 3]); m.build()
        w = ok.copy(); w[0, 2] = 1.5
        assert mrc(w) == sl.SCOPA_EINVAL and mrc(ok, alternating=2) == sl.SCOPA_EINVAL and mrc(None) == sl.SCOPA_EINVAL
        w[0, 2] = float("nan")
        assert mrc(w) == sl.SCOPA_EINVAL and mrc(ok, n=-1) == sl.SCOPA_EINVAL
        assert m.counters() == (0, 0)
        assert mrc(ok, n=0) == sl.SCOPA_OK and mrc(ok, active=np.array([0, 1, 0], np.uint8)) == sl.SCOPA_OK
        assert m.counters() == (2 * N_DECISION, 2 * N_TERMINAL)
    finally:
        m.close()
