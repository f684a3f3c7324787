"""The entries of k_mccfr_traverse and k_mccfr_apply_groups: every kernel argument in its slot at every launch site.

k_mccfr_traverse takes its arguments in the order its prologue needs them (the first 14 dwords arrive in SGPRs), with the launch geometry
passed explicitly, and is launched from four places: the plain launch and the launch that carries profiling events (launch_traverse), the
captured launch of graph mode (graph_for), and, through launch_traverse, the sharded iteration.  An argument in the wrong slot at ONE of
them is what these tests aim at, so the fixed inputs make every argument distinguishable from its neighbours: a 64-bit seed whose halves
are non-zero and differ, iteration 3, a first traversal id of 5 on the shard, a regret table that three iterations have already moved.

Deltas are held to the oracle's mccfr_batched_delta as test_gpu_parity.py::test_mccfr_batched_delta_vs_oracle holds them (regret
increments to 1e-12 of the largest, visit counts and the visit counters exact).  Where a route leaves no delta buffer behind (graph mode,
the sharded iteration) the delta is the difference of the tables around it; that difference carries the rounding of the kernel's one
addition R + d and of the subtraction here, 2 eps max|R| (eps = 2^-53), which is added to the bound.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 0x9E3779B15C09A7F3          # high word 0x9E3779B1, low word 0x5C09A7F3
ITER = 3
DEAL = 42
PRIOR_BATCH = 16                   # the three prior iterations that made the table
EPS = 2.0 ** -53
# one pair | around a workgroup's 16 wavefronts | two pairs in flight (8200 > 2 x 16 x 256) | takes from the workgroup counter
BATCHES = [1, 15, 16, 17, 8200, 10000]
LDS_2_WAVES = 90 * 1024            # at 738 infosets: 82 098 + 3 648 bytes per wavefront -> 2 wavefronts, a geometry argument of 128


@functools.lru_cache(maxsize=None)
def _tree(oracle):
    return oracle.Tree(seed=DEAL)


@functools.lru_cache(maxsize=None)
def _start(oracle):
    """the regret | strategy tables after three iterations, by the oracle"""
    t = _tree(oracle)
    R, S, _ = t.tables()
    t.mccfr_batched(R, S, SEED, 0, ITER, PRIOR_BATCH)
    assert (R != 0).any()
    R.setflags(write=False)
    S.setflags(write=False)
    return R, S


@functools.lru_cache(maxsize=None)
def _delta(oracle, iteration, b0, nb, after=None):
    """the oracle's delta of one launch from the start table (after = (iteration, b0, nb): from the table that launch left)"""
    R, _ = _start(oracle)
    if after is not None:
        R = R + _delta(oracle, *after)[0]
    out = _tree(oracle).mccfr_batched_delta(R, SEED, iteration, b0, nb)
    for a in out[:2]:
        a.setflags(write=False)
    return out


def _begin(ctx, sl, oracle):
    """deal set, iteration counter at 3, the start tables in place, nothing pending"""
    t = _tree(oracle)
    assert ctx.set_deal(sl.deal_py_seed(DEAL)) == t.n_infosets
    ctx.mccfr_seed(SEED)
    ctx.mccfr_iterate(1, ITER)
    assert ctx.mccfr_iteration() == ITER
    R, S = _start(oracle)
    ctx.tables_set(regret=R, strategy=S)
    ctx.mccfr_delta_set(np.zeros((t.n_infosets, 5)))
    return t, R, S


def _check(what, got_dR, got_count, got_visits, want, n_launch_pairs, slack=0.0):
    dR, dS, dv, tv = want
    err = np.abs(got_dR - dR)
    tol = 1e-12 * np.abs(dR) + 1e-12 * max(1.0, np.abs(dR).max()) + slack
    print(f"{what}: largest |delta - oracle| {err.max():.3g}, largest error / bound {np.max(err / tol):.3g}")
    assert np.array_equal(got_count, np.rint(dS.sum(1))), what            # traverser-visit counts per infoset: exact
    assert got_count.sum() == 172 * n_launch_pairs, what
    assert got_visits == (dv, tv) == (463 * n_launch_pairs, 240 * n_launch_pairs), what
    assert (err <= tol).all(), (what, np.argwhere(err > tol)[:4])


def _launch_and_check(ctx, what, want, b0, nb):
    c0 = ctx.counters()
    ctx.mccfr_traverse(ITER, b0, nb)
    d = ctx.mccfr_delta_get()
    c1 = ctx.counters()
    _check(what, d[:, :4], d[:, 4], (c1[0] - c0[0], c1[1] - c0[1]), want, nb)
    ctx.mccfr_delta_set(np.zeros_like(d))


@pytest.mark.parametrize("batch", BATCHES)
def test_traverse_arguments_by_every_launch_route(ctx, sl, oracle, batch):
    t, R, S = _begin(ctx, sl, oracle)
    want = _delta(oracle, ITER, 0, batch)
    # 1. the plain launch
    _launch_and_check(ctx, f"plain x {batch}", want, 0, batch)
    # 2. the launch that carries profiling events (every launch is sampled at stride 1)
    ctx.prof_enable(1)
    try:
        _launch_and_check(ctx, f"sampled x {batch}", want, 0, batch)
        assert ctx.prof_read()[0] == 1
    finally:
        ctx.prof_enable(0)
    # 3. the shard of a sharded iteration, traversal ids 5 .. 5 + batch, on one rank (k_mccfr_exchange_apply applies it)
    want5 = _delta(oracle, ITER, 5, batch)
    slack = 2 * EPS * max(1.0, np.abs(R).max() + np.abs(want5[0]).max())
    h = ctx.p2p_create(0, 1)
    try:
        ctx.p2p_connect(h.reshape(1, 64))
        c0 = ctx.counters()
        ctx.mccfr_iterate_sharded(5, batch, 1)
        assert ctx.p2p_status()[0] == 0
        c1 = ctx.counters()
    finally:
        ctx.p2p_destroy()
    R1, S1, _ = ctx.tables_get()
    count = np.rint((S1 - S).sum(1))                               # each visit adds a probability vector
    _check(f"shard b0 = 5 x {batch}", R1 - R, count, (c1[0] - c0[0], c1[1] - c0[1]), want5, batch, slack)
    np.testing.assert_allclose(S1 - S, want5[1], rtol=1e-10, atol=1e-10)
    assert ctx.mccfr_iteration() == ITER + 1
    # 4. graph mode: iterations 3 and 4 as one captured graph (the iteration number in a device word, advanced by the apply kernel)
    t, R, S = _begin(ctx, sl, oracle)
    want4 = _delta(oracle, ITER + 1, 0, batch, after=(ITER, 0, batch))
    both = (want[0] + want4[0], want[1] + want4[1], want[2] + want4[2], want[3] + want4[3])
    slack = 4 * EPS * max(1.0, np.abs(R).max() + np.abs(both[0]).max())
    c0 = ctx.counters()
    ctx.mccfr_graph_mode(True)
    try:
        ctx.mccfr_iterate(batch, 2)
    finally:
        ctx.mccfr_graph_mode(False)
    c1 = ctx.counters()
    assert ctx.mccfr_iteration() == ITER + 2
    R2, S2, _ = ctx.tables_get()
    count = np.rint((S2 - S).sum(1))
    dR, dS, dv, tv = both
    err = np.abs(R2 - R - dR)
    tol = 1e-12 * np.abs(dR) + 1e-12 * max(1.0, np.abs(dR).max()) + slack
    print(f"graph mode x {batch}: largest |delta - oracle| {err.max():.3g}, largest error / bound {np.max(err / tol):.3g}")
    assert np.array_equal(count, np.rint(dS.sum(1)))
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (dv, tv) == (463 * 2 * batch, 240 * 2 * batch)
    assert (err <= tol).all(), np.argwhere(err > tol)[:4]
    np.testing.assert_allclose(S2 - S, dS, rtol=1e-10, atol=1e-10)


def test_traverse_arguments_in_a_narrow_workgroup(ctx, sl, oracle):
    """Two wavefronts per workgroup (a geometry argument of 128, not 1024): 8200 pairs are 32 per workgroup over 256 workgroups,
    two in flight per wavefront and the rest taken from the workgroup counter."""
    _begin(ctx, sl, oracle)
    ctx.debug_lds_limit(LDS_2_WAVES)
    try:
        _launch_and_check(ctx, "two wavefronts x 8200", _delta(oracle, ITER, 0, 8200), 0, 8200)
    finally:
        ctx.debug_lds_limit(0)


# seed 42: 738 rows = 92 wavefronts of 8 rows and a quarter; seed 129: 1144 rows, the most among seeds 0..399 (14 wavefronts per
# traversal workgroup), whose last apply wavefront is full
@pytest.mark.parametrize("deal,n_inf", [(42, 738), (129, 1144)])
def test_apply_rows_after_three_iterations(ctx, sl, oracle, deal, n_inf):
    """mccfr_iterate(16, 3) against Tree.mccfr_batched: k_mccfr_apply_groups writes every row, the last one included, and the rows it
    prepares (the key word carried through the launch) are what the next traversal samples with."""
    t = oracle.Tree(seed=deal)
    assert t.n_infosets == n_inf == ctx.set_deal(sl.deal_py_seed(deal))
    ctx.mccfr_seed(SEED)
    ctx.mccfr_iterate(16, 3)
    R, S, _ = ctx.tables_get()
    Ro, So, _ = t.tables()
    t.mccfr_batched(Ro, So, SEED, 0, 3, 16)
    assert ctx.mccfr_iteration() == 3
    assert ctx.counters() == (463 * 16 * 3, 240 * 16 * 3)
    print(f"deal {deal}: largest |R - oracle| {np.abs(R - Ro).max():.3g}, |S - oracle| {np.abs(S - So).max():.3g}")
    np.testing.assert_allclose(R, Ro, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(S, So, rtol=1e-10, atol=1e-10)
    n = ctx.tree_export()["infoset_nlegal"]
    np.testing.assert_allclose(R[-1], Ro[-1], rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(S[-1], So[-1], rtol=1e-10, atol=1e-10)
    assert not R[-1, n[-1]:].any() and not S[-1, n[-1]:].any()    # nothing beyond the row's legal actions
    # the rows the last apply prepared: one more launch from the kernel's own table
    ctx.mccfr_delta_set(np.zeros((n_inf, 5)))
    ctx.mccfr_traverse(3, 0, 64)
    d = ctx.mccfr_delta_get()
    dR, dS, dv, tv = t.mccfr_batched_delta(R, SEED, 3, 0, 64)
    assert np.array_equal(d[:, 4], np.rint(dS.sum(1)))
    np.testing.assert_allclose(d[:, :4], dR, rtol=1e-12, atol=1e-12 * max(1.0, np.abs(dR).max()))
