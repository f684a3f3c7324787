"""The batched MCCFR step (k_mccfr_prepare / k_mccfr_traverse / k_mccfr_apply_groups, k_mccfr_fold + k_mccfr_apply, k_mccfr_multi)
on edge-case regret tables and on deals of every workgroup shape.

Tables (oracle/mccfr_edges.py): rows with nothing positive (negatives, -0.0), one-hot rows (sigma exactly 0 and 1: thresholds 0 and 2^31,
re-expanded actions of sampling probability 0), 1e-9 next to 1e6 (thresholds of a few units, importance weights up to 1e30 through the LDS
and memory-side float64 atomics), subnormals, |R| ~ 1e12, and a table on which the REFERENCE's own weights overflow.  The reference's own
_sample made tests/golden/mccfr_frozen_edges.npz from them; the oracle reproduces that fixture bit for bit (tests/test_mccfr_edges_ref.py),
and here the kernels are held to the fixture and to the oracle.

Exact: visit counts, counters, marked infosets, strategy sums after one apply (count * sigma: the same float64 operations as numpy's),
exploitability.  Regret deltas are compared PER INFOSET ROW: |kernel - oracle| <= K_REORDER * eps * A_row, A_row = the sum of |increment| over
everything the oracle added into the row, eps = 2^-53 -- one global max|dR| would hide every ordinary row behind a 1e30 one.
K_REORDER = 25 896 = 8 x 3 237, the largest error (in eps * A_row) of the ORACLE AGAINST ITSELF when the same increments are added in another
order (test_mccfr_edges_ref.py::test_reorder_budget: 3 237 at 17 923 pairs on the small_large table, below 900 at 3 000 pairs; a row that
receives thousands of like-signed increments far below its running sum rounds the same way every time, so the error grows with the number
of additions).  8 x because the kernel adds in arrival order over 16 group tables and up to 1024 lanes, which a shard shuffle only samples.
Neither number comes from a kernel's output.  After several iterations the tables feed back into sigma, and the bound is 100 x that over
the A_row summed over the iterations (the project's 1e-10 after a few iterations against 1e-12 per launch).

Deals (seed -> infosets -> wavefronts per traversal workgroup; prepare_traverse takes the largest of 16, 14, 12, ... whose
traverse_lds_bytes(I, w) + kStaticLds = ((I + 1) * 6 + 4 I) * 8 + 3648 w + pad16(4 I) + 3888 + I (+ pad) + 15 424 fits 163 840 bytes:
16 up to 1012 infosets, 14 up to 1098, 12 up to 1184; deal_py_seed(0 .. 2999) spans 251 .. 1177, so these three are all that real deals get):
    282 -> 251 -> 16 (fewest)      42 -> 738 -> 16      40 -> 1000 -> 16      2244 -> 1009 -> 16 | 474 -> 1018 -> 14 (the first switch)
    2797 -> 1095 -> 14 | 1789 -> 1108 -> 12 (the second switch)      1282 -> 1177 -> 12 (most)
"""
import numpy as np
import pytest

import mccfr_edges as E

pytestmark = pytest.mark.gpu

K = E.K_REORDER
DEAL_INFOSETS = {282: 251, 42: 738, 40: 1000, 2244: 1009, 474: 1018, 2797: 1095, 1789: 1108, 1282: 1177}
assert tuple(DEAL_INFOSETS) == E.DEALS


def _within(got, want, A, what, k=K):
    e = E.row_errors(got, want, A)
    print(f"{what}: largest row error {e.max():.1f} eps A_row (budget {k:.0f})")
    assert e.max() <= k, (what, int(e.argmax()), e.max())


def _check_delta(d, dR, dS, A, what, k=K):
    assert np.array_equal(d[:, 4], np.rint(dS.sum(1))), what      # traverser-visit counts per infoset: exact
    _within(d[:, :4], dR, A, what, k)


def _setup(ctx, sl, oracle, deal=42):
    t = oracle.Tree(seed=deal)
    assert ctx.set_deal(sl.deal_py_seed(deal)) == t.n_infosets
    return t


def _table(t, name):
    return np.zeros((t.n_infosets, 4)) if name == "zero" else E.edge_table(name, t.infoset_nlegal)


def _apply_expect(t, R, S0, dR, dS):
    """R + dR and S0 + count * sigma(R), sigma by the reference's current_strategy formula in numpy float64"""
    count = np.rint(dS.sum(1))
    return R + dR, S0 + count[:, None] * E.reference_sigma(R, t.infoset_nlegal)


def _check_applied(ctx, t, R, S0, dR, dS, A, what):
    Rn, Sn, _ = ctx.tables_get()
    Re, Se = _apply_expect(t, R, S0, dR, dS)
    assert np.array_equal(Sn, Se), what                           # one multiplication and one addition per cell, as numpy's
    # R + d: the delta's own budget plus the rounding of the one addition on either side
    err = np.abs(Rn - Re)
    tol = K * E.EPS * A.sum(1)[:, None] + 2 * E.EPS * np.abs(Re)
    assert (err <= tol).all(), (what, np.argwhere(err > tol)[:4])
    return Rn, Sn


@pytest.mark.parametrize("case", range(5))
def test_edge_fixture_cases_vs_reference_sample(ctx, sl, oracle, golden, case):
    """Each finite case of mccfr_frozen_edges.npz -- the deltas of the REFERENCE's own MCCFRTrainer._sample on an edge table -- through
    tables_set / mccfr_traverse / mccfr_delta_get / mccfr_apply / tables_get / visited_get: visit counts and counters exact, the marked
    infosets exactly the reference's dict keys, regret deltas and the applied tables within the row budget, strategy sums exact."""
    t = _setup(ctx, sl, oracle)
    keys = [sl.key_to_string(k) for k in ctx.tree_export()["infoset_key"]]
    name, R, seed, it, b0, nb, dR, dS, idx, _ = E.edge_case(golden.dir, keys, t.infoset_nlegal, case)
    assert name == E.FINITE_TABLES[case]
    _, _, A, _, _ = t.mccfr_batched_delta_abs(R, seed, it, b0, nb)
    S0 = np.zeros_like(R)
    ctx.tables_set(regret=R, strategy=S0)
    ctx.mccfr_seed(seed)
    ctx.mccfr_traverse(it, b0, nb)
    _check_delta(ctx.mccfr_delta_get(), dR, dS, A, f"fixture {name}")
    assert ctx.counters() == (463 * nb, 240 * nb)
    ctx.mccfr_apply()
    _check_applied(ctx, t, R, S0, dR, dS, A, f"fixture {name} applied")
    assert set(np.flatnonzero(ctx.visited_get() != 0)) == set(idx)


def test_nonfinite_fixture_case(ctx, sl, oracle, golden):
    """The table on which the reference's own weights overflow (reach / sampling probability = inf; inf * 0 = NaN, inf - inf = NaN).
    At infosets with a choice the kernel's delta is NaN / +inf / -inf in exactly the cells where the reference's is (their kind does not
    depend on the order of the additions, test_mccfr_edges_ref.py), every finite cell within the row budget, visit counts and counters exact.
    Two places where the step LEAVES the reference, both documented in DESIGN.md section 5 and asserted here as documented:
      * single-action infosets (plies 6-7).  The reference adds weight * (cfv - v) = weight * 0 there: 0 for every finite weight, NaN for an
        overflowed one (4 cells of this case, measured on an MI355X: reference NaN, kernel 0.0).  The kernel has no update lane for those
        nodes -- only their visit counts -- so their regret stays exactly what it was.  Matching would mean rebuilding reach and sampling
        probability for 120 more nodes per task in the hot path to produce a NaN the reference itself cannot survive (below).
      * the next row.  np.maximum / sum / divide turn a row that holds a NaN (or two +inf) into an all-NaN strategy, on which
        np.random.choice raises: the reference cannot run on.  mc_sigma's `R > 0` treats a NaN as not positive, so the step continues
        with the positive part of the row's other cells (uniform if there is none).  Asserted: a second traversal from the applied
        table runs, and its visit counts and counters are those of the recursion tree.
    The cells masked from the value comparison are the ones non-finite in the REFERENCE's fixture (8 of 381 touched cells, 2 %)."""
    t = _setup(ctx, sl, oracle)
    keys = [sl.key_to_string(k) for k in ctx.tree_export()["infoset_key"]]
    name, R, seed, it, b0, nb, dR, dS, idx, _ = E.edge_case(golden.dir, keys, t.infoset_nlegal, E.EDGE_TABLES.index("nonfinite"))
    _, _, A, _, _ = t.mccfr_batched_delta_abs(R, seed, it, b0, nb)
    S0 = np.zeros_like(R)
    ctx.tables_set(regret=R, strategy=S0)
    ctx.mccfr_seed(seed)
    ctx.mccfr_traverse(it, b0, nb)
    d = ctx.mccfr_delta_get()
    bad = ~np.isfinite(dR)
    assert 0 < bad.sum() < 0.05 * (np.arange(4)[None, :] < t.infoset_nlegal[:, None])[dS.sum(1) > 0].sum()
    g = d[:, :4]
    choice = (t.infoset_nlegal > 1)[:, None] & np.ones(4, bool)[None, :]
    assert (bad & choice).any() and (bad & ~choice).any()         # the case reaches both kinds of infoset
    for kind in (np.isnan, np.isposinf, np.isneginf):
        assert np.array_equal(kind(g)[choice], kind(dR)[choice]), kind.__name__
    assert not g[~choice].any()                                   # single-action infosets: no regret increment at all (documented)
    assert np.isnan(dR[bad & ~choice]).all() and not dR[~bad & ~choice].any()   # ... where the reference has 0, or NaN = inf * 0
    _check_delta(np.column_stack([np.where(bad, 0.0, g), d[:, 4]]), np.where(bad, 0.0, dR), dS, A, "fixture nonfinite")
    assert ctx.counters() == (463 * nb, 240 * nb)
    ctx.mccfr_apply()
    Rn, Sn, _ = ctx.tables_get()
    Re, Se = _apply_expect(t, R, S0, np.where(bad, 0.0, dR), dS)
    assert np.array_equal(Sn, Se)
    for kind in (np.isnan, np.isposinf, np.isneginf):
        assert np.array_equal(kind(Rn)[choice], kind(dR)[choice]), kind.__name__
    assert np.array_equal(Rn[~choice], R[~choice])
    assert (np.abs(Rn - Re)[~bad] <= (K * E.EPS * A.sum(1)[:, None] + 2 * E.EPS * np.abs(Re))[~bad]).all()
    assert set(np.flatnonzero(ctx.visited_get() != 0)) == set(idx)
    # the documented continuation: the next launch runs on the rows apply wrote
    c0 = ctx.counters()
    ctx.mccfr_traverse(it + 1, 0, 64)
    d2 = ctx.mccfr_delta_get()
    c1 = ctx.counters()
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (463 * 64, 240 * 64)
    assert d2[:, 4].sum() == 172 * 64 and d2[0, 4] == 64


# the batch shapes test_gpu_parity.py::test_mccfr_batched_delta_vs_oracle explains: one pair; fewer pairs than a workgroup's wavefronts x
# workgroups; 16 wavefronts x 256 workgroups + a ragged last one; more than four pairs per wavefront (double takes, single ones, ragged tail)
@pytest.mark.parametrize("batch", [1, 64, 4101, 17923])
@pytest.mark.parametrize("name", E.FINITE_TABLES)
def test_edge_tables_vs_oracle(ctx, sl, oracle, name, batch):
    t = _setup(ctx, sl, oracle)
    R = _table(t, name)
    ctx.tables_set(regret=R)
    ctx.mccfr_seed(0xABCDEF12345)
    ctx.mccfr_traverse(5, 10, batch)
    dR, dS, A, dv, tv = t.mccfr_batched_delta_abs(R, 0xABCDEF12345, 5, 10, batch)
    d = ctx.mccfr_delta_get()
    _check_delta(d, dR, dS, A, f"{name} x {batch}")
    assert d[:, 4].sum() == 172 * batch
    assert ctx.counters() == (dv, tv) == (463 * batch, 240 * batch)


def _oracle_iterations(t, R, S, seed, iter0, n_iters, batch):
    """Tree.mccfr_batched iteration by iteration, also returning the A_row summed over the iterations"""
    R, S, A = R.copy(), S.copy(), np.zeros_like(R)
    for it in range(iter0, iter0 + n_iters):
        dR, dS, dA, _, _ = t.mccfr_batched_delta_abs(R, seed, it, 0, batch)
        R += dR
        S += dS
        A += dA
    return R, S, A


def _check_iterations(ctx, t, R0, S0, seed, iter0, n_iters, batch, what):
    Ro, So, A = _oracle_iterations(t, R0, S0, seed, iter0, n_iters, batch)
    chk, Sc = R0.copy(), S0.copy()
    t.mccfr_batched(chk, Sc, seed, iter0, n_iters, batch)
    assert np.array_equal(chk, Ro) and np.array_equal(Sc, So)     # the helper above IS Tree.mccfr_batched
    Rg, Sg, _ = ctx.tables_get()
    err = np.abs(Rg - Ro)
    tol = 100 * K * E.EPS * A.sum(1)[:, None] + 100 * n_iters * E.EPS * np.abs(Ro)
    print(f"{what}: largest error / tolerance {np.max(err / np.maximum(tol, 1e-300)):.3g}")
    assert (err <= tol).all(), (what, np.argwhere(err > tol)[:4])
    np.testing.assert_allclose(Sg, So, rtol=1e-10, atol=1e-10)


@pytest.mark.parametrize("name", E.FINITE_TABLES)
def test_apply_and_the_next_row(ctx, sl, oracle, name):
    """After mccfr_apply on an edge table: tables_get = R + dR, S0 + count * sigma(R) (numpy float64, the reference's current_strategy
    formula, from a non-zero S0); a second mccfr_traverse from the applied table equals the oracle's delta from that table -- the only way the
    sigma | threshold rows written by apply_row_store (not by k_mccfr_prepare) get checked on such rows; then mccfr_iterate(256, 4) from
    the edge table against Tree.mccfr_batched."""
    t = _setup(ctx, sl, oracle)
    R = _table(t, name)
    S0 = np.where(np.arange(4)[None, :] < t.infoset_nlegal[:, None], np.random.RandomState(3).random_sample(R.shape) * 50, 0.0)
    seed = 0x5C09A
    ctx.tables_set(regret=R, strategy=S0)
    ctx.mccfr_seed(seed)
    ctx.mccfr_traverse(1, 100, 3000)
    dR, dS, A, _, _ = t.mccfr_batched_delta_abs(R, seed, 1, 100, 3000)
    _check_delta(ctx.mccfr_delta_get(), dR, dS, A, f"{name} first launch")
    ctx.mccfr_apply()
    Rn, Sn = _check_applied(ctx, t, R, S0, dR, dS, A, f"{name} applied")
    assert not ctx.mccfr_delta_get().any()
    # the second launch samples with the rows apply wrote; the oracle starts from the kernel's own applied table (its thresholds are a
    # function of the rounded regrets)
    ctx.mccfr_traverse(2, 7, 3000)
    dR2, dS2, A2, _, _ = t.mccfr_batched_delta_abs(Rn, seed, 2, 7, 3000)
    _check_delta(ctx.mccfr_delta_get(), dR2, dS2, A2, f"{name} second launch")
    # whole iterations from the edge table
    ctx.tables_set(regret=R, strategy=S0)
    ctx.mccfr_delta_set(np.zeros((t.n_infosets, 5)))
    it0 = ctx.mccfr_iteration()
    c0 = ctx.counters()
    ctx.mccfr_iterate(256, 4)
    c1 = ctx.counters()
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (463 * 256 * 4, 240 * 256 * 4)
    _check_iterations(ctx, t, R, S0, seed, it0, 4, 256, f"{name} 4 iterations")


@pytest.mark.parametrize("name", ["onehot", "small_large", "allneg"])
def test_other_routes_to_the_same_arithmetic(ctx, sl, oracle, name):
    """Graph mode, the split path (three ragged shards + k_mccfr_fold / k_mccfr_apply), mccfr_iterate_sharded on one rank
    (k_mccfr_exchange_apply) and the narrow-workgroup forms (debug_lds_limit), each from an edge table."""
    t = _setup(ctx, sl, oracle)
    R = _table(t, name)
    S0 = np.zeros_like(R)
    seed = 77
    ctx.mccfr_seed(seed)
    # graph mode: 5 iterations as one captured graph, then eager ones take over
    ctx.tables_set(regret=R, strategy=S0)
    it0 = ctx.mccfr_iteration()
    ctx.mccfr_graph_mode(True)
    try:
        ctx.mccfr_iterate(256, 5)
    finally:
        ctx.mccfr_graph_mode(False)
    assert ctx.mccfr_iteration() == it0 + 5
    _check_iterations(ctx, t, R, S0, seed, it0, 5, 256, f"{name} graph mode")
    # split path: three ragged shards into one delta, then apply
    ctx.tables_set(regret=R, strategy=S0)
    ctx.mccfr_delta_set(np.zeros((t.n_infosets, 5)))
    for b0, nb in ((50, 100), (150, 2371), (2521, 529)):
        ctx.mccfr_traverse(3, b0, nb)
    dR, dS, A, _, _ = t.mccfr_batched_delta_abs(R, seed, 3, 50, 3000)
    _check_delta(ctx.mccfr_delta_get(), dR, dS, A, f"{name} split path")
    ctx.mccfr_apply()
    _check_applied(ctx, t, R, S0, dR, dS, A, f"{name} split path applied")
    # one rank of a sharded run: the exchange-and-apply kernel
    ctx.tables_set(regret=R, strategy=S0)
    h = ctx.p2p_create(0, 1)
    try:
        ctx.p2p_connect(h.reshape(1, 64))
        it0 = ctx.mccfr_iteration()
        ctx.mccfr_iterate_sharded(0, 256, 3)
        assert ctx.p2p_status()[0] == 0
    finally:
        ctx.p2p_destroy()
    _check_iterations(ctx, t, R, S0, seed, it0, 3, 256, f"{name} sharded, one rank")
    # narrow workgroups: 16, 8, 4, 2, 1 wavefronts at 738 infosets (82 098 + 3 648 bytes per wavefront)
    ctx.tables_set(regret=R, strategy=S0)
    dR, dS, A, dv, tv = t.mccfr_batched_delta_abs(R, seed, 4, 100, 3000)
    try:
        for limit in (0, 112 * 1024, 98 * 1024, 90 * 1024, 86 * 1024):
            ctx.debug_lds_limit(limit)
            c0 = ctx.counters()
            ctx.mccfr_delta_set(np.zeros((t.n_infosets, 5)))
            ctx.mccfr_traverse(4, 100, 3000)
            d = ctx.mccfr_delta_get()
            c1 = ctx.counters()
            assert (c1[0] - c0[0], c1[1] - c0[1]) == (dv, tv) == (463 * 3000, 240 * 3000), limit
            _check_delta(d, dR, dS, A, f"{name} lds limit {limit}")
    finally:
        ctx.debug_lds_limit(0)


@pytest.mark.parametrize("deal", E.DEALS)
def test_deals_of_every_workgroup_shape(ctx, sl, oracle, deal):
    """The deals of the module docstring -- fewest and most infosets, and both sides of each switch of the wavefront count: the zero table,
    onehot and small_large at 3000 pairs against the oracle; six iterations against Tree.mccfr_batched; exploitability bit-equal."""
    t = _setup(ctx, sl, oracle, deal)
    assert t.n_infosets == DEAL_INFOSETS[deal]
    seed = 0x5C09A + deal
    ctx.mccfr_seed(seed)
    for name in ("zero", "onehot", "small_large"):
        R = _table(t, name)
        ctx.tables_set(regret=R, strategy=np.zeros_like(R))
        ctx.mccfr_delta_set(np.zeros((t.n_infosets, 5)))
        c0 = ctx.counters()
        ctx.mccfr_traverse(2, 11, 3000)
        d = ctx.mccfr_delta_get()
        c1 = ctx.counters()
        dR, dS, A, dv, tv = t.mccfr_batched_delta_abs(R, seed, 2, 11, 3000)
        assert (c1[0] - c0[0], c1[1] - c0[1]) == (dv, tv) == (463 * 3000, 240 * 3000)
        _check_delta(d, dR, dS, A, f"deal {deal} {name}")
    ctx.tables_reset()
    ctx.mccfr_delta_set(np.zeros((t.n_infosets, 5)))
    it0 = ctx.mccfr_iteration()
    ctx.mccfr_iterate(256, 6)
    Z = np.zeros((t.n_infosets, 4))
    _check_iterations(ctx, t, Z, Z, seed, it0, 6, 256, f"deal {deal} 6 iterations")
    _, Sg, _ = ctx.tables_get()
    assert ctx.exploitability()["exploitability"] == t.exploitability(t.average_policy(Sg))[0]


@pytest.mark.parametrize("batch", [1, 37, 48])
def test_multi_deal_persistent_mccfr_on_more_deals_and_batches(ctx, sl, oracle, batch):
    """k_mccfr_multi shares the walk: the shape of test_gpu_multi.py::test_multi_deal_persistent_mccfr_matches_oracle with the deal of most
    infosets (seed 1282: 12 wavefronts) and with batches of 1 and 37 pairs (fewer pairs than wavefronts; not a multiple of them)."""
    seeds = [42, 1282, 282, 474, 1789, 7]
    m = sl.MultiDeal(ctx, len(seeds))
    try:
        m.deal_py_seeds(seeds)
        m.build()
        m.mccfr_iterate(batch=batch, n_iters=5, seed=321)
        for i, s in enumerate(seeds):
            t = oracle.Tree(seed=s)
            Z = np.zeros((t.n_infosets, 4))
            Ro, So, A = _oracle_iterations(t, Z, Z, 321, 0, 5, batch)
            Rg, Sg, _, _ = m.tables_get(i)
            np.testing.assert_allclose(Rg, Ro, rtol=1e-10, atol=1e-10)
            np.testing.assert_allclose(Sg, So, rtol=1e-10, atol=1e-10)
        assert m.counters() == (463 * batch * 5 * len(seeds), 240 * batch * 5 * len(seeds))
    finally:
        m.close()
