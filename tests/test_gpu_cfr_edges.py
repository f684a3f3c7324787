"""The exact tabular solvers on edge-case tables, by every launch route: k_cfr_exact_sched, k_cfr_exact with its tables in LDS and in HBM,
the multi-deal k_cfr_exact, k_cfr_exact_lanes / k_rows_pack, k_cfr_sync and k_exploitability (single deal and multi-deal).

Tables (oracle/cfr_edges.py): regrets with nothing positive (-0.0 included), one-hot rows, 1e-9 next to 1e6, subnormals, 1e12, +inf, NaN, a
local_strategy that is not regret-matching of regret_sum, strategy sums with zero rows, subnormal rows and rows whose sum overflows.  The
reference's own CFRTrainer made tests/golden/vanilla_cfr_edges.npz from them and the oracle reproduces that fixture bit for bit
(tests/test_cfr_edges_ref.py); here the kernels are held to the fixture and, where the fixture has no case, to the oracle.  Every table
comparison is of uint64 views (cfr_edges.same_bits: -0.0 is not +0.0); in the inf / nan cases the finite cells bit for bit and the others by kind.

Launch routes of scopa_cfr_exact_*: 0 = the scheduled kernel, 1 = the one-lane walk with the tables in LDS, 2 = the same walk with the tables in
HBM.  scopa_cfr_exact_last_route says which one ran; scopa_cfr_exact_mode and scopa_debug_lds_limit (64 KB: the 738-infoset deal's tables no
longer fit beside the walk's maps) select them.  No limit used here is one the library refuses, and the calls that must fail return their error
code before any launch."""
import numpy as np
import pytest

import cfr_edges as E

pytestmark = pytest.mark.gpu

KB64 = 64 * 1024
DEVICE_LDS = 160 * 1024          # gfx950: 160 KB of LDS per workgroup
N_DECISION, N_TERMINAL = 1653, 576


def _tree(oracle, deal, _cache={}):
    if deal not in _cache:
        _cache[deal] = oracle.Tree(seed=deal)
    return _cache[deal]


def _deal(ctx, sl, oracle, deal):
    t = _tree(oracle, deal)
    assert ctx.set_deal(sl.deal_py_seed(deal)) == t.n_infosets
    assert [sl.key_to_string(k) for k in ctx.tree_export()["infoset_key"]] == t.infoset_strings
    return t


def _seed(ctx, R, S, L):
    ctx.tables_reset()
    ctx.tables_set(regret=R, strategy=S, local=L)
    got = ctx.tables_get()
    assert all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(got, (R, S, L)))      # set / get carry every bit, NaN payloads included


def _same_tables(case, got, want, what):
    for name, a, b in zip(("regret", "strategy", "local"), got, want):
        assert E.same(case, a, b), (what, name, np.argwhere(np.asarray(a).view(np.uint64) != np.asarray(b).view(np.uint64))[:4])


def _route(ctx, route):
    """Select a launch route for the deal at hand; returns the route the library must report."""
    ctx.debug_lds_limit(KB64 if route == 2 else 0)
    ctx.cfr_exact_mode(route == 1)
    return route


def _restore(ctx):
    ctx.debug_lds_limit(0)
    ctx.cfr_exact_mode(False)


def _subtree(t, path):
    """(decision nodes, terminals, first-visit sequence numbers by infoset) of the DFS below the state reached by legal-action indices `path`"""
    node = 0
    for a in path:
        node = int(t.child[node][a])
    seq, dec, term, stack = np.zeros(t.n_infosets, np.uint32), 0, 0, [node]
    while stack:
        k = stack.pop()
        if t.term[k]:
            term += 1
            continue
        dec += 1
        if seq[t.infoset[k]] == 0:
            seq[t.infoset[k]] = seq.max() + 1
        stack.extend(int(t.child[k][a]) for a in reversed(range(t.nlegal[k])))
    return dec, term, seq


# ---- fixture x route ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", range(len(E.FIXTURE_CASES)))
def test_fixture_cases_by_every_route(ctx, sl, oracle, golden, n):
    """Every case of vanilla_cfr_edges.npz (the REFERENCE's tables after 3 iterations from the seeded tables) through scopa_cfr_exact_iterate on
    the scheduled route and the LDS walk -- and, on the 738-infoset deal, the HBM walk --, whole, split 1 + 2, and as six cfr_exact_traverse
    calls: root values, the three tables, first-visit numbers, counters, and the route the library says it took.
    The HBM walk against the FIXTURE is therefore the two seed-42 cases only: the smallest limit scopa_debug_lds_limit accepts is 64 KB, and the
    251-infoset deal's tables (24 KB + 10.5 KB of maps) still fit under it, so the nine seed-282 cases cannot be sent down that route.  The other
    cases take it on the seed-42 deal against the oracle (test_hbm_walk_on_every_case_vs_oracle), which tests/test_cfr_edges_ref.py pins to the
    fixture on the same cases."""
    g, meta = E.fixture(golden.dir)
    case, deal = meta[n]["case"], meta[n]["deal"]
    t = _deal(ctx, sl, oracle, deal)
    want = (g[f"c{n}_regret"], g[f"c{n}_strategy"], g[f"c{n}_local"])
    R, S, L = E.tables(case, t.infoset_nlegal)
    routes = (0, 1, 2) if t.n_infosets * 96 + 10756 > KB64 else (0, 1)       # the walk's tables + its static maps against the 64 KB the hook accepts
    assert deal != 42 or routes == (0, 1, 2)
    try:
        assert ctx.cfr_exact_last_route() in (-1, 0, 1, 2)
        for route in routes:
            _route(ctx, route)
            for form in ("whole", "split", "traversals"):
                _seed(ctx, R, S, L)
                c0 = ctx.counters()
                if form == "whole":
                    rv = ctx.cfr_exact_iterate(3)
                elif form == "split":
                    rv = np.concatenate([ctx.cfr_exact_iterate(1), ctx.cfr_exact_iterate(2)])
                else:
                    rv = np.array([[ctx.cfr_exact_traverse(0), ctx.cfr_exact_traverse(1)] for _ in range(3)])
                what = (case, deal, route, form)
                assert ctx.cfr_exact_last_route() == route, what
                assert E.same(case, rv, g[f"c{n}_root"]), what
                _same_tables(case, ctx.tables_get(), want, what)
                assert np.array_equal(ctx.visited_get(), np.arange(1, t.n_infosets + 1)), what
                c1 = ctx.counters()
                assert (c1[0] - c0[0], c1[1] - c0[1]) == (2 * 3 * N_DECISION, 2 * 3 * N_TERMINAL), what
    finally:
        _restore(ctx)


@pytest.mark.parametrize("n", range(len(E.FIXTURE_CASES), len(E.FIXTURE_CASES) + len(E.TRAVERSE_FROM)))
def test_traverse_from_fixture_cases(ctx, sl, oracle, golden, n):
    """scopa_cfr_exact_traverse_from on a state three / six plies down with reach arguments (0.0, 1.0) and (5e-324, 1e-300) against the
    reference: always the one-lane walk (route 1), whatever the mode."""
    g, meta = E.fixture(golden.dir)
    m = meta[n]
    t = _deal(ctx, sl, oracle, m["deal"])
    R, S, L = E.tables(m["case"], t.infoset_nlegal)
    dec, term, seq = _subtree(t, m["path"])
    try:
        for sequential in (False, True):
            ctx.cfr_exact_mode(sequential)
            _seed(ctx, R, S, L)
            c0 = ctx.counters()
            v = ctx.cfr_exact_traverse_from(m["traverser"], m["path"], float(m["r0"]), float(m["r1"]))
            assert ctx.cfr_exact_last_route() == 1
            assert E.same_bits(np.array([v]), g[f"c{n}_value"])
            _same_tables(m["case"], ctx.tables_get(), (g[f"c{n}_regret"], g[f"c{n}_strategy"], g[f"c{n}_local"]), m)
            assert np.array_equal(ctx.visited_get(), seq)
            c1 = ctx.counters()
            assert (c1[0] - c0[0], c1[1] - c0[1]) == (dec, term)
    finally:
        _restore(ctx)


def test_hbm_walk_on_every_case_vs_oracle(ctx, sl, oracle):
    """The route no other test takes: k_cfr_exact with use_lds = 0 (tables read and written in HBM by the one walking lane), every case of
    oracle/cfr_edges.py on the 738-infoset deal, 2 iterations, against the oracle; reached from either mode."""
    t = _deal(ctx, sl, oracle, 42)
    try:
        for k, case in enumerate(E.CASES):
            R, S, L = E.tables(case, t.infoset_nlegal)
            ctx.debug_lds_limit(KB64)
            ctx.cfr_exact_mode(bool(k & 1))
            _seed(ctx, R, S, L)
            rv = ctx.cfr_exact_iterate(2)
            assert ctx.cfr_exact_last_route() == 2, case
            rvo = t.cfr_exact(R, S, L, 2)
            assert E.same(case, rv, rvo), case
            _same_tables(case, ctx.tables_get(), (R, S, L), case)
    finally:
        _restore(ctx)


# ---- where the routes switch ----------------------------------------------------------------------------------------------------------
def sched_steps(t):
    """Length of the exact-CFR schedule of a deal, restated from its definition (scopa_cfr.hip, head): exit events levelled as soon as possible; a
    node opens no earlier than its parent and than the exit of the previous node (in DFS order) of its infoset, and exits one step after the last
    of its children."""
    last_exit = np.zeros(t.n_infosets, np.int64)
    top = 0

    def visit(k, opened):
        nonlocal top
        mx = opened
        for a in range(t.nlegal[k]):
            c = int(t.child[k][a])
            if not t.term[c]:
                mx = max(mx, visit(c, max(opened, int(last_exit[t.infoset[c]]))))
        last_exit[t.infoset[k]] = mx + 1
        top = max(top, mx + 1)
        return mx + 1

    visit(0, 0)
    return top


def sched_lds_bytes(n_infosets, n_steps):
    """scopa_cfr.hip:sched_lds_bytes restated: three tables, node values, event words, the node -> infoset area, step offsets (padded to 8),
    path cells, payoffs, 32 bytes of slack."""
    return n_infosets * 4 * 8 * 3 + N_DECISION * 8 + (N_DECISION + 1) * 4 + (1656 + ((n_steps + 2 + 7) & ~7) + N_DECISION * 8) * 2 + N_TERMINAL + 32


@pytest.mark.parametrize("deal", [282, 42, 129, 1282])
def test_route_at_the_devices_real_limit(ctx, sl, oracle, deal):
    """With the device's own LDS limit, the route scopa_cfr_exact_iterate takes is the one sched_lds_bytes predicts -- the 1177-infoset deal
    (seed 1282, the largest known) sits within a few hundred bytes of the switch -- and every finite case and the stale one match the oracle over
    2 iterations on it."""
    t = _deal(ctx, sl, oracle, deal)
    assert t.n_infosets == {282: 251, 42: 738, 129: 1144, 1282: 1177}[deal]
    steps = sched_steps(t)
    need = sched_lds_bytes(t.n_infosets, steps)
    predicted = 0 if need <= DEVICE_LDS else (1 if t.n_infosets * 96 + 10756 <= DEVICE_LDS else 2)
    print(f"deal {deal}: {t.n_infosets} infosets, {steps} steps, scheduled kernel needs {need} of {DEVICE_LDS} bytes -> route {predicted}")
    # which side of the switch each deal falls on, and by how much: the 1177-infoset deal has 592 bytes to spare, so every deal known takes the scheduled kernel
    assert (steps, need) == {282: (194, 74704), 42: (75, 121216), 129: (31, 160112), 1282: (22, 163248)}[deal] and predicted == 0
    try:
        ctx.debug_lds_limit(DEVICE_LDS)                   # accepted only if the device offers that much ...
        with pytest.raises(sl.ScopaError):
            ctx.debug_lds_limit(DEVICE_LDS + 1)           # ... and this only if it offers more: the real limit is DEVICE_LDS
        ctx.debug_lds_limit(0)
        for case in E.FINITE_CASES + ("stale",):
            R, S, L = E.tables(case, t.infoset_nlegal)
            _seed(ctx, R, S, L)
            rv = ctx.cfr_exact_iterate(2)
            assert ctx.cfr_exact_last_route() == predicted, case
            rvo = t.cfr_exact(R, S, L, 2)
            assert E.same_bits(rv, rvo), case
            _same_tables(case, ctx.tables_get(), (R, S, L), (deal, case))
    finally:
        _restore(ctx)


# ---- multi-deal -----------------------------------------------------------------------------------------------------------------------
def _multi(ctx, sl, oracle, n):
    seeds = [282, 42, 129, 1282] + list(range(3, n - 1))
    m = sl.MultiDeal(ctx, n)
    m.deal_py_seeds(seeds)
    ninf = m.build()
    trees = [_tree(oracle, s) if s in (282, 42, 129, 1282) else oracle.Tree(seed=s) for s in seeds]
    assert list(ninf) == [t.n_infosets for t in trees]
    return m, trees


@pytest.mark.parametrize("n", [65, 200])
def test_multi_deal_exact_cfr_from_edge_tables(ctx, sl, oracle, n):
    """scopa_multi_tables_set, then the workgroup-per-deal kernel (every case, by deal index) and the lane-per-deal kernel (the consistent cases:
    the finite ones and nan_held) against the oracle on every deal; 1 + 2 iterations.
    nan_held is consistent by its definition -- local_strategy = InfoNode.get_strategy(regret_sum), the uniform row where a regret is NaN -- so
    k_rows_pack must ACCEPT it (the lanes call not raising is that assertion; under `R > 0 ? R : 0` regret matching of such a row is the
    normalised rest of the row and the pack refuses), and lane_rec must play uniform on those rows: this is the cover of scopa_multi.hip's own
    regret_match, which the workgroup-per-deal kernel (scopa_cfr.hip's) does not go through."""
    all_cases = list(E.CASES)
    for lanes, cases in ((False, all_cases), (True, list(E.LANE_CASES))):
        m, trees = _multi(ctx, sl, oracle, n)
        try:
            for i, t in enumerate(trees):
                R, S, L = E.tables(cases[i % len(cases)], t.infoset_nlegal)
                m.tables_set(i, R, S, L)
            step = m.cfr_exact_iterate_lanes if lanes else m.cfr_exact_iterate
            step(1)
            if lanes:                                         # a partial set while the tables live in the row image: only that table changes
                t = trees[7]
                R7, S7, L7, _ = m.tables_get(7)
                m.tables_set(7, strategy=S7 + 1.0)
                got = m.tables_get(7)
                assert E.same_bits(got[0], R7) and E.same_bits(got[1], S7 + 1.0) and E.same_bits(got[2], L7)
                m.tables_set(7, strategy=S7)
            step(2)
            for i, t in enumerate(trees):
                case = cases[i % len(cases)]
                R, S, L = E.tables(case, t.infoset_nlegal)
                t.cfr_exact(R, S, L, 3)
                _same_tables(case, m.tables_get(i)[:3], (R, S, L), (n, lanes, i, case))
            assert m.counters() == (2 * 3 * N_DECISION * n, 2 * 3 * N_TERMINAL * n)
        finally:
            m.close()


def test_lanes_refuse_a_stale_local_strategy_and_change_nothing(ctx, sl, oracle):
    """The `stale` case on one deal of 65: the lane-per-deal call raises (k_rows_pack compares local_strategy with regret-matching of regret_sum
    BIT FOR BIT: a -0.0 for a 0.0 is a difference too), every table of every deal is bit-unchanged, and the workgroup-per-deal kernel then
    matches the oracle on all of them."""
    n = 65
    m, trees = _multi(ctx, sl, oracle, n)
    try:
        cases = [E.FINITE_CASES[i % 5] for i in range(n)]
        cases[64] = "stale"                                   # the ragged second wavefront's only deal
        for i, t in enumerate(trees):
            m.tables_set(i, *E.tables(cases[i], t.infoset_nlegal))
        with pytest.raises(sl.ScopaError) as e:
            m.cfr_exact_iterate_lanes(1)
        assert e.value.status == sl.SCOPA_ESTATE
        for i, t in enumerate(trees):
            _same_tables(cases[i], m.tables_get(i)[:3], E.tables(cases[i], t.infoset_nlegal), ("unchanged", i))
        assert m.counters() == (0, 0)
        # a local_strategy row that differs from regret-matching only in the SIGN of a zero is refused as well
        R, S, L = E.tables("onehot", trees[3].infoset_nlegal)
        Lz = L.copy()
        Lz[np.flatnonzero(trees[3].infoset_nlegal > 1)[0], np.flatnonzero(L[np.flatnonzero(trees[3].infoset_nlegal > 1)[0]] == 0)[0]] = -0.0
        assert np.array_equal(Lz, L) and not E.same_bits(Lz, L)
        m.tables_set(64, *E.tables("big", trees[64].infoset_nlegal))
        m.tables_set(3, R, S, Lz)
        with pytest.raises(sl.ScopaError):
            m.cfr_exact_iterate_lanes(1)
        m.tables_set(3, local=L)
        m.tables_set(64, *E.tables("stale", trees[64].infoset_nlegal))
        cases[3] = "onehot"
        m.cfr_exact_iterate(2)
        for i, t in enumerate(trees):
            R, S, L = E.tables(cases[i], t.infoset_nlegal)
            t.cfr_exact(R, S, L, 2)
            _same_tables(cases[i], m.tables_get(i)[:3], (R, S, L), ("workgroup kernel", i))
    finally:
        m.close()


@pytest.mark.parametrize("n", [65, 200])
def test_multi_deal_sync_cfr_and_exploitability_from_edge_tables(ctx, sl, oracle, n):
    """k_cfr_sync (1 + 4 iterations) and k_exploitability in multi-deal mode from the finite cases and nan_held (k_cfr_sync's regret-matching select
    in multi-deal mode), per deal against the oracle."""
    m, trees = _multi(ctx, sl, oracle, n)
    try:
        cases = [E.LANE_CASES[i % len(E.LANE_CASES)] for i in range(n)]
        for i, t in enumerate(trees):
            m.tables_set(i, *E.tables(cases[i], t.infoset_nlegal))
        before = m.exploitability()
        for i, t in enumerate(trees):
            _, S, _ = E.tables(cases[i], t.infoset_nlegal)
            P = t.average_policy(S)
            e, br = t.exploitability(P)
            assert E.same_bits(before[i], np.array([e, br[0], br[1], t.policy_value(P)])), (i, cases[i])
        m.cfr_sync_iterate(1)
        m.cfr_sync_iterate(4)
        after = m.exploitability()
        for i, t in enumerate(trees):
            R, S, L = E.tables(cases[i], t.infoset_nlegal)
            t.cfr_sync(R, S, 5)
            _same_tables(cases[i], m.tables_get(i)[:3], (R, S, L), ("sync", i))        # local_strategy is not synchronous CFR's to touch
            P = t.average_policy(S)
            e, br = t.exploitability(P)
            assert E.same_bits(after[i], np.array([e, br[0], br[1], t.policy_value(P)])), (i, cases[i])
    finally:
        m.close()


# ---- synchronous CFR and exploitability on one context --------------------------------------------------------------------------------
@pytest.mark.parametrize("deal", [282, 42, 1282])
def test_sync_cfr_and_exploitability_from_edge_tables(ctx, sl, oracle, deal):
    """scopa_cfr_sync_iterate split 1 + 4 from every finite case (and the NaN table: k_cfr_sync has the regret-matching select too) against
    Tree.cfr_sync; scopa_exploitability with policy=None from the edge strategy sums (zero rows, subnormal rows, overflowing sums) and with explicit
    edge policies, the returned policy included."""
    t = _deal(ctx, sl, oracle, deal)
    n = t.infoset_nlegal.astype(int)
    for case in E.FINITE_CASES + ("nan_held",):
        R, S, L = E.tables(case, n)
        _seed(ctx, R, S, L)
        ctx.cfr_sync_iterate(1)
        ctx.cfr_sync_iterate(4)
        t.cfr_sync(R, S, 5)
        _same_tables(case, ctx.tables_get(), (R, S, L), ("sync", deal, case))
    legal = np.arange(4)[None, :] < n[:, None]
    for kind in E.S_KINDS:
        S = E.strategy_sum_table(kind, n)
        ctx.tables_set(strategy=S)
        got = ctx.exploitability(return_policy=True)
        P = t.average_policy(S)
        e, br = t.exploitability(P)
        assert E.same_bits(got["policy"], P), (deal, kind)
        assert E.same_bits(np.array([got["exploitability"], got["br0"], got["br1"], got["value_p0"]]), np.array([e, br[0], br[1], t.policy_value(P)])), (deal, kind)
    policies = {"uniform": np.where(legal, 1.0 / n[:, None], 0.0), "onehot": E.reference_sigma(E.edge_table("onehot", n), n),
                "small_large": E.reference_sigma(E.edge_table("small_large", n), n), "negzero": np.where(legal, E.reference_sigma(E.edge_table("onehot", n), n), -0.0)}
    for name, P in policies.items():
        got = ctx.exploitability(policy=P, return_policy=True)
        e, br = t.exploitability(P)
        assert E.same_bits(got["policy"], P), (deal, name)
        assert E.same_bits(np.array([got["exploitability"], got["br0"], got["br1"], got["value_p0"]]), np.array([e, br[0], br[1], t.policy_value(P)])), (deal, name)


def test_exploitability_refuses_an_lds_limit_its_tables_do_not_fit(ctx, sl, oracle):
    """k_exploitability keeps policy, q, reach and values in LDS (119 KB at 1177 infosets): under a 64 KB limit the call returns SCOPA_ELIMIT
    before any launch, the tables are untouched, and with the limit restored it matches the oracle."""
    t = _deal(ctx, sl, oracle, 1282)
    R, S, L = E.tables("small_large", t.infoset_nlegal)
    _seed(ctx, R, S, L)
    try:
        ctx.debug_lds_limit(KB64)
        c0 = ctx.counters()
        with pytest.raises(sl.ScopaError) as e:
            ctx.exploitability()
        assert e.value.status == sl.SCOPA_ELIMIT
        with pytest.raises(sl.ScopaError) as e:
            ctx.cfr_sync_iterate(1)
        assert e.value.status == sl.SCOPA_ELIMIT
        assert ctx.counters() == c0
        _same_tables("small_large", ctx.tables_get(), (R, S, L), "refused")
    finally:
        _restore(ctx)
    assert ctx.exploitability()["exploitability"] == t.exploitability(t.average_policy(S))[0]


# ---- interleaving ---------------------------------------------------------------------------------------------------------------------
def test_entry_points_interleaved_on_one_context(ctx, sl, oracle):
    """One context, one scripted sequence mirrored on the oracle: the validity flags the entry points hand each other (sigma | threshold rows,
    the exact-CFR schedule, evaluation thresholds) are invalidated by hand in the library; a missing invalidation gives stale strategies
    silently.  Exact, synchronous and exploitability segments bit for bit; MCCFR segments at the 1e-10 the project uses for several iterations
    (test_mccfr_batched_iterations_vs_oracle), after which the oracle continues from the device's own tables."""
    import torch
    t = _deal(ctx, sl, oracle, 42)
    R, S, L = t.tables()
    seed = 77
    ctx.mccfr_seed(seed)

    def check_bits(what):
        _same_tables("finite", ctx.tables_get(), (R, S, L), what)

    def reload(what):
        Rg, Sg, Lg = ctx.tables_get()
        np.testing.assert_allclose(Rg, R, rtol=1e-10, atol=1e-10, err_msg=what)
        np.testing.assert_allclose(Sg, S, rtol=1e-10, atol=1e-10, err_msg=what)
        assert E.same_bits(Lg, L), what                        # MCCFR does not touch local_strategy
        return Rg, Sg, Lg

    assert E.same_bits(ctx.cfr_exact_iterate(2), t.cfr_exact(R, S, L, 2)); check_bits("exact 1")
    it0 = ctx.mccfr_iteration()
    ctx.mccfr_iterate(32, 2)
    t.mccfr_batched(R, S, seed, it0, 2, 32)
    R, S, L = reload("mccfr_iterate")
    assert E.same_bits(ctx.cfr_exact_iterate(1), t.cfr_exact(R, S, L, 1)); check_bits("exact 2")
    it0 = ctx.mccfr_iteration()
    ctx.mccfr_iterate(32, 1)                                    # nothing but exact CFR since the last MCCFR step: its sigma rows are stale unless run_exact said so
    t.mccfr_batched(R, S, seed, it0, 1, 32)
    R, S, L = reload("mccfr_iterate right after exact CFR")
    ctx.cfr_sync_iterate(2)
    t.cfr_sync(R, S, 2); check_bits("sync 1")
    R, S, L = E.tables("onehot", t.infoset_nlegal)             # sigma of exactly 0 and 1: nothing like the rows the previous segments left
    ctx.tables_set(regret=R, strategy=S, local=L)
    ctx.mccfr_traverse(5, 0, 32)                                # must sample with sigma of the tables just set, not of the previous ones
    ctx.mccfr_apply()
    t.mccfr_batched(R, S, seed, 5, 1, 32)
    R, S, L = reload("mccfr_traverse + mccfr_apply after tables_set")
    P = t.average_policy(S)
    got = ctx.exploitability(return_policy=True)
    e, br = t.exploitability(P)
    assert E.same_bits(got["policy"], P) and (got["exploitability"], got["br0"], got["br1"]) == (e, br[0], br[1])
    pol = torch.from_numpy(got["policy"]).to("cuda:0")
    ctx.eval_tabular_prepare(pol.data_ptr())
    st = ctx.eval_tabular_match(256, 128, 1)
    assert st[0, 0] == 128 and st[1, 0] == 128
    t2 = _deal(ctx, sl, oracle, 282)                            # another deal: schedule, rows and thresholds of deal 42 are void
    with pytest.raises(sl.ScopaError) as ex:
        ctx.eval_tabular_match(256, 128, 1)
    assert ex.value.status == sl.SCOPA_ESTATE
    R, S, L = t2.tables()
    check_bits("tables after set_deal")
    assert E.same_bits(ctx.cfr_exact_iterate(2), t2.cfr_exact(R, S, L, 2)); check_bits("exact on the new deal")
    assert ctx.cfr_exact_last_route() == 0
    it0 = ctx.mccfr_iteration()
    ctx.mccfr_iterate(32, 1)
    t2.mccfr_batched(R, S, seed, it0, 1, 32)
    R, S, L = reload("mccfr_iterate on the new deal")
    ctx.tables_reset()
    R, S, L = t2.tables()
    check_bits("tables_reset")
    ctx.cfr_sync_iterate(3)
    t2.cfr_sync(R, S, 3); check_bits("sync after reset")
    ctx.mccfr_traverse(9, 0, 32)                                # after sync CFR moved the regrets
    ctx.mccfr_apply()
    t2.mccfr_batched(R, S, seed, 9, 1, 32)
    R, S, L = reload("mccfr after sync")
    ctx.cfr_sync_iterate(1)                                     # nothing but synchronous CFR between two MCCFR steps
    t2.cfr_sync(R, S, 1); check_bits("sync between two MCCFR steps")
    ctx.mccfr_traverse(10, 0, 32)
    ctx.mccfr_apply()
    t2.mccfr_batched(R, S, seed, 10, 1, 32)
    reload("mccfr right after sync")
