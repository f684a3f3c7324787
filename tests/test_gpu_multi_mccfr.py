"""k_mccfr_multi (scopa_multi_mccfr_iterate, MultiDeal.mccfr_iterate) held to the standard of the single-deal batched MCCFR step.

The kernel shares the walk body with k_mccfr_traverse and k_mccfr_chance; everything around the walk is its own: the deal's regret table loaded
into LDS and kept there for n_iters iterations, sigma | thresholds frozen from that LIVE table in-kernel (mc_sigma + choice_cdf, not
k_mccfr_prepare / apply_row_store), the walks' LDS float64 atomics straight into the live table, count * sigma added to the strategy sums in HBM,
the counters.  Checked here: non-zero starting tables (the finite edge tables of oracle/mccfr_edges.py through MultiDeal.tables_set) and a non-zero
S0, exact strategy sums and counters, batches around and far above the wavefront count, more deals than CUs, narrow workgroups and the LDS limit,
a seed with a non-zero high word, iteration numbers reached by resuming and by tables_set on a used handle, and the argument edges.

THE ERROR MEASURE, one iteration from the table R0 (oracle/mccfr_edges.py:live_table_tol, derived there, checked on the oracle alone by
tests/test_mccfr_edges_ref.py::test_live_table_budget; nothing in it comes from a kernel):
    |R_kernel - (R0 + dR_oracle)| <= tol_row = 2 (c_row + 1) eps (max|R0_row| + A_row)      per infoset row
c_row = the oracle's traverser-visit count of the row, A_row = the sum of |increment| the oracle added into the row, eps = 2^-53.  The walks add onto
the live value, so every addition rounds at the magnitude of |R0| + the running sum: the single-deal budget K_REORDER eps A_row does not apply.
Strategy sums after one iteration are S0 + count * sigma(R0) in numpy float64, BIT FOR BIT; rows nobody visited and the cells k >= n keep their bits.
Several iterations: the project's multi-iteration form (test_gpu_mccfr_edges.py::_check_iterations) plus tol_row summed over the iterations.

WORKGROUP WIDTHS.  launch_mccfr_multi takes the largest of 16, 14, ..., 2 wavefronts whose multi_lds_bytes(max_infosets, w) + kStaticLdsMulti fits
the LDS limit (restated below as _multi_lds).  One WaveScratch per wavefront (1 824 bytes, k_mccfr_traverse keeps two), so under the device's own
163 840 bytes EVERY deal_py_seed deal runs 16 wavefronts wide here (1 177 infosets: 148 608 bytes); narrower workgroups are reached through
Context.debug_lds_limit, with limits derived -- and asserted -- from the restated sizes:
    seed 1282 (1 177 infosets) at 140 KB -> 12      seed 282 (251) at 64 KB, the smallest limit the hook takes -> 12      seed 42 (738) at 98 KB -> 10
    seed 42 at 92 KB -> 6      seed 42 at 88 KB -> 4      seed 42 at 84 KB -> 2 (86 016 >= 85 760: two wavefronts fit)
    seed 42 at 82 KB: two wavefronts do not fit (85 760) but the formula with ZERO does (82 112) -- the window in which the launcher's descent used
    to reach 0 wavefronts and issue a launch with blockDim = 0; seed 42 at 64 KB: below even that.  Both: SCOPA_ELIMIT, nothing touched.
"""
import numpy as np
import pytest

import mccfr_edges as E
from test_gpu_mccfr_edges import _oracle_iterations, _table

pytestmark = pytest.mark.gpu

KB = 1024
DEVICE_LDS = 160 * KB
SEED = 0x5C09A
SEED_HI = 0x9E3779B97F4A7C15                  # a non-zero high word
PAIR = (463, 240)                             # decision / terminal visits of one traversal pair
INFOSETS = {282: 251, 42: 738, 7: 702, 474: 1018, 1789: 1108, 1282: 1177}


# ---- the host's sizes (scopa_mccfr.hip: multi_lds_bytes, kStaticLdsMulti, sizeof(WaveScratch)), restated for the derivations ------------------------
def _multi_lds(max_infosets, waves):
    wave_scratch = 168 * 4 + 128 + 64 * 16
    b = ((max_infosets + 1) * 6 + max_infosets * 4) * 8 + waves * wave_scratch
    b += ((max_infosets * 4 + 15) & ~15) + 1656 * 2 + 576 + max_infosets
    return ((b + 15) & ~15) + 64 + 15 * 1024


def _waves(max_infosets, limit):
    """the launcher's rule: the largest of 16, 14, ..., 2 that fits; None where two wavefronts do not fit (SCOPA_ELIMIT)"""
    return next((w for w in range(16, 0, -2) if _multi_lds(max_infosets, w) <= limit), None)


# ---- the oracle, once per distinct (deal, table, seed, iteration, batch); nothing cached is ever modified ----------------------------------------
_TREES, _ONE = {}, {}


def _tree(oracle, deal):
    if deal not in _TREES:
        _TREES[deal] = oracle.Tree(seed=deal)
        assert _TREES[deal].n_infosets == INFOSETS.get(deal, _TREES[deal].n_infosets)
    return _TREES[deal]


def _start(t, name):
    """(R0, S0) of a deal: the table `name`, and for an edge table a strategy sum random in [0, 50) on the legal cells, 0 elsewhere (the
    construction of test_gpu_mccfr_edges.py::test_apply_and_the_next_row); the zero table starts from S0 = 0 like a fresh handle"""
    R = _table(t, name)
    legal = np.arange(4)[None, :] < t.infoset_nlegal[:, None]
    S = np.zeros_like(R) if name == "zero" else np.where(legal, np.random.RandomState(3).random_sample(R.shape) * 50, 0.0)
    return R, S


def _expect_one(oracle, deal, name, seed, iteration, batch):
    """one iteration from (R0, S0): -> R0, S0, R0 + dR, S0 + count * sigma(R0) (numpy float64, the reference's current_strategy formula), tol_row,
    count"""
    key = (deal, name, seed, iteration, batch)
    if key not in _ONE:
        t = _tree(oracle, deal)
        R0, S0 = _start(t, name)
        dR, dS, A, dv, tv = t.mccfr_batched_delta_abs(R0, seed, iteration, 0, batch)
        assert (dv, tv) == (PAIR[0] * batch, PAIR[1] * batch)
        count = np.rint(dS.sum(1))
        assert count.sum() == 172 * batch and count[0] == batch
        _ONE[key] = (R0, S0, R0 + dR, S0 + count[:, None] * E.reference_sigma(R0, t.infoset_nlegal), E.live_table_tol(R0, dS, A), count)
    return _ONE[key]


def _bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _check_one(m, i, t, exp, what):
    """deal i of m after ONE iteration against _expect_one's tuple -> the largest row error in units of tol_row"""
    R0, S0, Re, Se, tol, count = exp
    Rg, Sg, _, _ = m.tables_get(i)
    assert _bits(Sg, Se), (what, np.argwhere(Sg != Se)[:4])       # one product and one sum per cell, as numpy's
    legal = np.arange(4)[None, :] < t.infoset_nlegal[:, None]
    assert _bits(Rg[~legal], R0[~legal]) and _bits(Sg[~legal], S0[~legal]), what        # cells k >= n: untouched
    assert _bits(Rg[count == 0], R0[count == 0]) and _bits(Sg[count == 0], S0[count == 0]), what     # rows nobody visited
    assert (Rg != R0).any(), what
    e = E.live_row_errors(Rg, Re, tol)
    assert e.max() <= 1.0, (what, int(e.argmax()), e.max())
    return e.max()


def _multi(ctx, sl, seeds):
    m = sl.MultiDeal(ctx, len(seeds))
    try:
        m.deal_py_seeds(seeds)
        assert list(m.build()) == [INFOSETS[s] for s in seeds]
    except BaseException:
        m.close()
        raise
    return m


def _set(m, i, t, name):
    R0, S0 = _start(t, name)
    m.tables_set(i, regret=R0, strategy=S0)


def _raises(sl, status, call):
    with pytest.raises(sl.ScopaError) as e:
        call()
    assert e.value.status == status, str(e.value)
    return e.value


# ---- 1. edge tables, one iteration ---------------------------------------------------------------------------------------------------------------------
def test_edge_tables_one_iteration(ctx, sl, oracle):
    """Six copies of the seed-42 deal in one MultiDeal: deals 0..4 start from the five finite edge tables (one-hot rows: thresholds 0 and 2^31; rows with
    nothing positive and -0.0; subnormals; 1e-9 next to 1e6; |R| ~ 1e12) and a non-zero S0 through tables_set, deal 5 from the zero table.  3000
    pairs, one iteration: R within tol_row, S bit-equal to S0 + count * sigma(R0), counters exact."""
    t = _tree(oracle, 42)
    names = E.FINITE_TABLES + ("zero",)
    assert len(names) == 6
    m = _multi(ctx, sl, [42] * 6)
    try:
        for i, name in enumerate(E.FINITE_TABLES):
            _set(m, i, t, name)
        assert m.counters() == (0, 0)
        m.mccfr_iterate(batch=3000, n_iters=1, seed=SEED)
        worst = {name: _check_one(m, i, t, _expect_one(oracle, 42, name, SEED, 0, 3000), f"edge table {name}") for i, name in enumerate(names)}
        print("edge tables, 3000 pairs: largest row error / tol_row " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
        assert m.counters() == (PAIR[0] * 3000 * 6, PAIR[1] * 3000 * 6)
    finally:
        m.close()


# ---- 2. several iterations, resume, split, seed ----------------------------------------------------------------------------------------------------------
def _expect_iterations(t, R0, S0, seed, iter0, n_iters, batch):
    """test_gpu_mccfr_edges.py::_oracle_iterations (asserted: the same bits) plus the live-table term summed over the iterations, each from the
    oracle's own table at the start of that iteration -> R, S, tol [I][1]"""
    R, S, A, live = R0.copy(), S0.copy(), np.zeros_like(R0), np.zeros(len(R0))
    for it in range(iter0, iter0 + n_iters):
        dR, dS, dA, _, _ = t.mccfr_batched_delta_abs(R, seed, it, 0, batch)
        live += E.live_table_tol(R, dS, dA)
        R += dR
        S += dS
        A += dA
    Ro, So, Ao = _oracle_iterations(t, R0, S0, seed, iter0, n_iters, batch)
    assert _bits(R, Ro) and _bits(S, So) and _bits(A, Ao)
    tol = 100 * E.K_REORDER * E.EPS * A.sum(1)[:, None] + 100 * n_iters * E.EPS * np.abs(R) + live[:, None]
    return R, S, tol


def _iterations_error(m, i, exp):
    """deal i against _expect_iterations' tuple -> the largest |error| / tolerance; S with rtol = atol = 1e-10 as _check_iterations does"""
    Ro, So, tol = exp
    Rg, Sg, _, _ = m.tables_get(i)
    np.testing.assert_allclose(Sg, So, rtol=1e-10, atol=1e-10)
    err = np.abs(Rg - Ro)
    return float(np.max(np.where(err == 0.0, 0.0, err / np.maximum(tol, 1e-300))))


@pytest.mark.parametrize("name", ["onehot", "small_large", "allneg"])
def test_iterations_resume_and_seed(ctx, sl, oracle, name):
    """256 pairs x 4 iterations from an edge table on the seed-42 deal and on the deal of most infosets (seed 1282): the in-kernel freeze reads the live
    table the walks just wrote.  One call of 4 and two calls of 1 + 3 from the same tables_set against the same oracle run -- the second call starts at
    iteration 1: its result is NOT the oracle's with the iteration number restarted --, then, on the handle now at iteration 4, tables_set again and 4
    more with a seed whose high word is non-zero, against the oracle at iterations 4..7 with that seed."""
    deals = [42, 1282]
    trees = [_tree(oracle, d) for d in deals]
    start = [_start(t, name) for t in trees]
    exp = [_expect_iterations(t, R0, S0, SEED, 0, 4, 256) for t, (R0, S0) in zip(trees, start)]
    worst = {}
    a = _multi(ctx, sl, deals)
    try:
        for i, t in enumerate(trees):
            _set(a, i, t, name)
        a.mccfr_iterate(batch=256, n_iters=4, seed=SEED)
        worst["4"] = max(_iterations_error(a, i, exp[i]) for i in range(2))
        assert a.counters() == (PAIR[0] * 256 * 4 * 2, PAIR[1] * 256 * 4 * 2)
    finally:
        a.close()
    b = _multi(ctx, sl, deals)
    try:
        for i, t in enumerate(trees):
            _set(b, i, t, name)
        b.mccfr_iterate(batch=256, n_iters=1, seed=SEED)
        b.mccfr_iterate(batch=256, n_iters=3, seed=SEED)
        worst["1 + 3"] = max(_iterations_error(b, i, exp[i]) for i in range(2))
        assert b.counters() == (PAIR[0] * 256 * 4 * 2, PAIR[1] * 256 * 4 * 2)
        for i, (t, (R0, S0)) in enumerate(zip(trees, start)):      # what a second call restarting at iteration 0 would give is far outside
            R1, S1, _ = _expect_iterations(t, R0, S0, SEED, 0, 1, 256)
            Rr, _, tol = _expect_iterations(t, R1, S1, SEED, 0, 3, 256)
            assert (np.abs(b.tables_get(i)[0] - Rr) > 1e3 * tol).any()
        for i, t in enumerate(trees):
            _set(b, i, t, name)
        b.mccfr_iterate(batch=256, n_iters=4, seed=SEED_HI)
        exp_hi = [_expect_iterations(t, R0, S0, SEED_HI, 4, 4, 256) for t, (R0, S0) in zip(trees, start)]
        worst["high-word seed, iterations 4..7"] = max(_iterations_error(b, i, exp_hi[i]) for i in range(2))
        for i, (t, (R0, S0)) in enumerate(zip(trees, start)):      # ... and so is the low word alone
            Rl, _, tol = _expect_iterations(t, R0, S0, SEED_HI & 0xFFFFFFFF, 4, 4, 256)
            assert (np.abs(b.tables_get(i)[0] - Rl) > 1e3 * tol).any()
    finally:
        b.close()
    print(f"{name}, 256 pairs x 4 iterations: largest error / tolerance " + ", ".join(f"{k}: {v:.3g}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


# ---- 3. batches and shapes -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 15, 16, 17, 1000, 4101])
def test_batches_and_deal_shapes(ctx, sl, oracle, batch):
    """The deals of fewest and most infosets and three between, zero tables, one iteration: fewer pairs than the 16 wavefronts, one fewer, as many, one
    more, and batches that are no multiple of 16 (1000 = 62 x 16 + 8, 4101 = 256 x 16 + 5)."""
    deals = [282, 42, 474, 1789, 1282]
    assert _waves(max(INFOSETS[d] for d in deals), DEVICE_LDS) == 16
    m = _multi(ctx, sl, deals)
    try:
        m.mccfr_iterate(batch=batch, n_iters=1, seed=SEED)
        worst = max(_check_one(m, i, _tree(oracle, d), _expect_one(oracle, d, "zero", SEED, 0, batch), f"deal {d} x {batch}") for i, d in enumerate(deals))
        print(f"batch {batch}: largest row error {worst:.3f} tol_row")
        assert m.counters() == (PAIR[0] * batch * len(deals), PAIR[1] * batch * len(deals))
    finally:
        m.close()


# ---- 4. more deals than CUs --------------------------------------------------------------------------------------------------------------------------------
def test_more_deals_than_cus(ctx, sl, oracle):
    """600 deals cycling over six seeds: the grid wraps, and every one of the 600 workgroups must have used its OWN deal's offsets into the maps, the
    tables and the counters.  Then every deal is set back to zero tables except deal 599, which gets the onehot table: a wrapped workgroup reading deal
    0's rows would give deal 0's result.  The second run is at iteration 1 on a handle whose tables were replaced by tables_set."""
    seeds = [42, 282, 7, 474, 1789, 1282]
    n, batch = 600, 64
    m = sl.MultiDeal(ctx, n)
    try:
        m.deal_py_seeds([seeds[i % 6] for i in range(n)])
        ninf = m.build()
        assert list(ninf) == [INFOSETS[seeds[i % 6]] for i in range(n)]
        m.mccfr_iterate(batch=batch, n_iters=1, seed=SEED)
        worst = max(_check_one(m, i, _tree(oracle, seeds[i % 6]), _expect_one(oracle, seeds[i % 6], "zero", SEED, 0, batch), f"deal {i}") for i in range(n))
        assert m.counters() == (PAIR[0] * batch * n, PAIR[1] * batch * n)
        for i in range(n):
            _set(m, i, _tree(oracle, seeds[i % 6]), "onehot" if i == n - 1 else "zero")
        m.mccfr_iterate(batch=batch, n_iters=1, seed=SEED)
        table = lambda i: "onehot" if i == n - 1 else "zero"
        worst2 = max(_check_one(m, i, _tree(oracle, seeds[i % 6]), _expect_one(oracle, seeds[i % 6], table(i), SEED, 1, batch), f"deal {i}, second run")
                     for i in range(n))
        assert not _bits(m.tables_get(n - 1)[0], m.tables_get(n - 7)[0])      # the same seed's deal from the zero table
        assert m.counters() == (PAIR[0] * batch * n * 2, PAIR[1] * batch * n * 2)
        print(f"600 deals x 64 pairs: largest row error {worst:.3f} tol_row; with deal 599 on onehot, iteration 1: {worst2:.3f}")
    finally:
        m.close()


# ---- 5. narrow workgroups and the limit --------------------------------------------------------------------------------------------------------------------
def _two_deals_one_iteration(ctx, sl, oracle, deal, what):
    """two copies of `deal`, deal 0 from onehot (and a non-zero S0), deal 1 from zero: test 1's form"""
    t = _tree(oracle, deal)
    m = _multi(ctx, sl, [deal, deal])
    try:
        _set(m, 0, t, "onehot")
        m.mccfr_iterate(batch=3000, n_iters=1, seed=SEED)
        e = [_check_one(m, i, t, _expect_one(oracle, deal, name, SEED, 0, 3000), f"{what} {name}") for i, name in enumerate(("onehot", "zero"))]
        assert m.counters() == (PAIR[0] * 3000 * 2, PAIR[1] * 3000 * 2)
    finally:
        m.close()
    print(f"{what}: largest row error / tol_row onehot {e[0]:.3f}, zero {e[1]:.3f}")


@pytest.mark.parametrize("deal,limit_kb,waves", [(1282, 140, 12), (282, 64, 12), (42, 98, 10), (42, 92, 6), (42, 88, 4), (42, 84, 2)])
def test_narrow_workgroups(ctx, sl, oracle, deal, limit_kb, waves):
    I, limit = INFOSETS[deal], limit_kb * KB
    assert _waves(I, limit) == waves and _multi_lds(I, waves) <= limit < _multi_lds(I, waves + 2)
    try:
        ctx.debug_lds_limit(limit)
        _two_deals_one_iteration(ctx, sl, oracle, deal, f"seed {deal} at {limit_kb} KB ({waves} wavefronts)")
    finally:
        ctx.debug_lds_limit(0)


@pytest.mark.parametrize("limit_kb", [64, 82])
def test_lds_limit_refusal_leaves_everything_untouched(ctx, sl, oracle, limit_kb):
    """seed 42 (738 infosets) under 64 KB -- below the tables alone -- and under 82 KB: two wavefronts need 85 760 bytes, the formula with none 82 112, so
    a descent 16, 14, ..., 2, 0 used to pass the size check with zero wavefronts.  SCOPA_ELIMIT, tables, counters and the iteration number as they
    were; under the device's own limit the same handle then runs iteration 0 correctly."""
    I, limit = INFOSETS[42], limit_kb * KB
    assert _waves(I, limit) is None and _multi_lds(I, 2) > limit
    assert (_multi_lds(I, 0) <= limit) == (limit_kb == 82)
    t = _tree(oracle, 42)
    m = _multi(ctx, sl, [42, 42])
    try:
        _set(m, 0, t, "onehot")
        before = [m.tables_get(i)[:2] for i in range(2)]
        try:
            ctx.debug_lds_limit(limit)
            e = _raises(sl, sl.SCOPA_ELIMIT, lambda: m.mccfr_iterate(batch=3000, n_iters=1, seed=SEED))
            assert "LDS" in str(e)
            for i in range(2):
                Rg, Sg, _, _ = m.tables_get(i)
                assert _bits(Rg, before[i][0]) and _bits(Sg, before[i][1])
            assert m.counters() == (0, 0)
        finally:
            ctx.debug_lds_limit(0)
        m.mccfr_iterate(batch=3000, n_iters=1, seed=SEED)
        e = [_check_one(m, i, t, _expect_one(oracle, 42, name, SEED, 0, 3000), f"after the refusal, {name}") for i, name in enumerate(("onehot", "zero"))]
        print(f"after SCOPA_ELIMIT at {limit_kb} KB: largest row error / tol_row onehot {e[0]:.3f}, zero {e[1]:.3f}")
        assert m.counters() == (PAIR[0] * 3000 * 2, PAIR[1] * 3000 * 2)
    finally:
        m.close()


def test_chance_game_refuses_the_zero_wavefront_window(ctx, sl, oracle):
    """launch_mccfr_chance has k_mccfr_multi's carving and descent: the one-deal game on seed 42 under 82 KB.  SCOPA_ELIMIT, nothing touched; under the
    device's own limit the handle runs: the chance game over one deal IS that deal (traversal ids 0 * batch + i), so its tables are the oracle's --
    strategy sums exact, regrets within the reorder budget of a zeroed delta table (K_REORDER eps A_row)."""
    I, limit = INFOSETS[42], 82 * KB
    assert _multi_lds(I, 0) <= limit < _multi_lds(I, 2)
    t = _tree(oracle, 42)
    m = _multi(ctx, sl, [42])
    try:
        g = sl.ChanceGame(m)
        try:
            assert g.G == I
            mp = g.index()[1][0, :I]
            R0, S0 = g.tables_get()
            try:
                ctx.debug_lds_limit(limit)
                e = _raises(sl, sl.SCOPA_ELIMIT, lambda: g.mccfr_iterate(8, 1, SEED))
                assert "LDS" in str(e)
                Rg, Sg = g.tables_get()
                assert _bits(Rg, R0) and _bits(Sg, S0) and g.mccfr_counters() == (0, 0, 0)
            finally:
                ctx.debug_lds_limit(0)
            g.mccfr_iterate(8, 1, SEED)
            Rg, Sg = g.tables_get()
            dR, dS, A, _, _ = t.mccfr_batched_delta_abs(np.zeros((I, 4)), SEED, 0, 0, 8)
            assert g.mccfr_counters() == (PAIR[0] * 8, PAIR[1] * 8, 1)
            count = np.rint(dS.sum(1))
            assert _bits(Sg[mp], count[:, None] * E.reference_sigma(np.zeros((I, 4)), t.infoset_nlegal)) and (Rg != 0).any()
            e = E.row_errors(Rg[mp], dR, A)
            print(f"chance game, one deal, after SCOPA_ELIMIT at 82 KB: largest row error {e.max():.1f} eps A_row (budget {E.K_REORDER:.0f})")
            assert e.max() <= E.K_REORDER
        finally:
            g.close()
    finally:
        m.close()


# ---- 6. argument edges ---------------------------------------------------------------------------------------------------------------------------------------
def test_argument_edges(ctx, sl, oracle):
    """Host-side checks before any launch: batch 0 and batch, n_iters above 2^24 are SCOPA_EINVAL; n_iters = 0 is a no-op.  Tables (an edge table and a
    non-zero S0), counters and the iteration number stay as they were: the next real call is iteration 0."""
    t = _tree(oracle, 42)
    m = _multi(ctx, sl, [42, 282])
    try:
        _set(m, 0, t, "onehot")
        before = [m.tables_get(i)[:2] for i in range(2)]
        for kw in (dict(batch=0, n_iters=1), dict(batch=2 ** 24 + 1, n_iters=1), dict(batch=16, n_iters=2 ** 24 + 1)):
            _raises(sl, sl.SCOPA_EINVAL, lambda: m.mccfr_iterate(seed=SEED, **kw))
        m.mccfr_iterate(batch=16, n_iters=0, seed=SEED)
        for i in range(2):
            Rg, Sg, _, _ = m.tables_get(i)
            assert _bits(Rg, before[i][0]) and _bits(Sg, before[i][1])
        assert m.counters() == (0, 0)
        m.mccfr_iterate(batch=16, n_iters=1, seed=SEED)
        e = [_check_one(m, 0, t, _expect_one(oracle, 42, "onehot", SEED, 0, 16), "after the refused calls, onehot"),
             _check_one(m, 1, _tree(oracle, 282), _expect_one(oracle, 282, "zero", SEED, 0, 16), "after the refused calls, zero")]
        print(f"after the refused calls, 16 pairs: largest row error / tol_row {max(e):.3f}")
        assert m.counters() == (PAIR[0] * 16 * 2, PAIR[1] * 16 * 2)
    finally:
        m.close()
