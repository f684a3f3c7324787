"""GPU checks of the sampling solver on Team MiniScopa over a set of deals (scopa_team_chance_mccfr.hip) against the restatement
tests/team_chance_mccfr_ref.py, which tests/test_team_chance_mccfr_ref.py pins to the one-deal restatement, and against the one-deal solver itself.

Every iteration is compared from the device's OWN tables (regrets that differ in their last bits give sigmas that do, so only a common start makes the
strategy sums comparable bit for bit, as tests/test_gpu_team_mccfr.py::batched_iteration does).  Strategy sums, visit counts, the sigma rows of
untouched rows and the counters are exact.  The regrets, sums of float64 increments added in arrival order -- here across the workgroups of several
deals -- are held per row to the project's reorder budget (oracle/mccfr_edges.py):  |R_gpu - R_ref| <= K_REORDER * eps * A_row + 2 * eps * |R_ref|,
A_row = the sum of |increment| the restatement added into the row.  The budget was derived for up to 17 923 increments per row; a row here receives at
most n * 2 * batch <= 768 (six deals at batch 64).  The sigma row of a touched row is regret matching of the device's own new regrets, exactly.

Not exercised: n * batch > 2^32 (SCOPA_EINVAL) needs more than 256 deals, whose index alone takes tens of seconds to build; it is one host compare
next to the batch bounds that are exercised.

The sets here (`swap`, `six`) share rows at depths 0 and 1 only, all inside the LDS accumulator, and `copies` shares every row but is held to its visit
counts alone; regrets of delta rows of depth 5 or more hit from several deals and of shared rows of depths 2..4 in the flush are
tests/test_gpu_team_chance_shared.py's (both4, reordered, hidden6)."""
import ctypes as C

import numpy as np
import pytest

import mccfr_edges as E
import philox_words as W
import team_chance_mccfr_ref as CM

pytestmark = pytest.mark.gpu

SEED = 0x5C09A
PACKETS = [[0, 5, 10, 15], [1, 4, 11, 14], [2, 7, 8, 13], [3, 6, 9, 12]]
DRAWS, TERMINALS = CM.DRAWS, CM.TERMINALS
_CACHE = {}


def deal_set(name):
    from scopa_amd.algorithms.team_chance import packet_deals
    six = packet_deals(PACKETS, fix_seat0=True)
    if name == "one":
        return six[:1]
    if name == "copies":
        return six[[0, 0]]
    if name == "swap":          # seats 2 and 3 swap their hands: the rows of depths 0 and 1 are shared
        return six[:2]
    assert name == "six"
    return six


def ref_of(name, oracle):
    if name not in _CACHE:
        _CACHE[name] = CM.ChanceMCRef(deal_set(name))
    return _CACHE[name]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def in_budget(R_gpu, R_ref, A, what, k=1.0):
    """per row, printed before it is asserted: the largest error in units of its budget.  Cells whose reference value is not finite are compared by
    kind; a row's A then counts its finite cells only, which can only tighten the bound of the others"""
    fin = np.isfinite(R_ref)
    A_row = np.where(np.isfinite(A), A, 0.0).sum(1)
    with np.errstate(invalid="ignore"):
        bound = k * (E.K_REORDER * E.EPS * A_row)[:, None] + 2.0 * E.EPS * np.abs(R_ref)
        err = np.abs(R_gpu - R_ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = np.where(fin & (err != 0.0), err / bound, 0.0).max()
    print(what, "largest regret error / budget:", worst)
    kinds = all(np.array_equal(f(R_gpu), f(R_ref)) for f in (np.isnan, np.isposinf, np.isneginf))
    return kinds and bool((err[fin] <= bound[fin]).all())


@pytest.fixture()
def game_of(sl, ctx, oracle):
    games = []
    ctx.mccfr_seed(SEED)

    def make(name):
        games.append(sl.TeamChanceGame(deal_set(name), ctx))
        return games[-1]
    yield make
    for g in games:
        g.close()


def state_of(game):
    R, S = game.tables_get()
    return R, S, game.sigma_get()


def check_iteration(game, cm, batch, deals, what, exact=None, seed=SEED):
    """one iteration on the device and in the restatement from the device's own tables -> (count, A) of the restatement"""
    same = exact or (lambda a, b: np.array_equal(bits(a), bits(b)))
    R0, S0, sig0 = state_of(game)
    it = game.mccfr_counters()[2]
    R, S, sig = R0.copy(), S0.copy(), sig0.copy()
    A, cnt = cm.iterate(R, S, sig, batch, seed, it, deals)
    game.mccfr_iterate(batch, 1, None if deals is None else [deals])
    m = game.n if deals is None else len(deals)
    assert cnt.sum() == m * batch * 2 * CM.PER_TRAVERSAL
    Rg, Sg, sigg = state_of(game)
    assert same(Sg, S), f"{what}: strategy differs in {np.count_nonzero(Sg != S)} cells"
    assert in_budget(Rg, R, A, what), what
    idle = cnt == 0
    assert np.array_equal(bits(Rg[idle]), bits(R0[idle])) and np.array_equal(bits(sigg[idle]), bits(sig0[idle])), what
    assert same(sigg, cm.cr.sigma(Rg)), f"{what}: sigma is not regret matching of the new regrets"
    assert not game.mccfr_delta_get().any(), what
    assert game.mccfr_counters()[2] == it + 1
    return cnt, A


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_exist_and_count(game_of):
    game = game_of("one")
    assert game.mccfr_counters() == (0, 0, 0)
    game.mccfr_iterate(5)
    assert game.mccfr_counters() == (5 * DRAWS, 5 * TERMINALS, 1)
    R, S = game.tables_get()
    assert abs(S.sum() - 5 * 2 * CM.PER_TRAVERSAL) < 1e-6 and np.count_nonzero(R) > 1000   # sigma sums to 1 per visit, up to rounding


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,batch", [("swap", 1), ("swap", 3), ("swap", 64), ("six", 64)])
def test_iterations_against_the_restatement(oracle, game_of, name, batch):
    """swap at batch 1: 2 tasks per deal, fewer than a deal's share of the grid; six at batch 64: 128 tasks per deal on about 85 workgroups, which loop"""
    cm, game = ref_of(name, oracle), game_of(name)
    keys, mp = game.index()
    assert np.array_equal(keys, cm.cr.gkey) and np.array_equal(mp, cm.cr.map)
    for it in range(3):
        check_iteration(game, cm, batch, None, f"{name}, batch {batch}, iteration {it + 1}")
    assert game.mccfr_counters() == (3 * game.n * batch * DRAWS, 3 * game.n * batch * TERMINALS, 3)


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------------
def test_one_deal_equals_the_one_deal_solver(ctx, oracle, game_of):
    cm, game = ref_of("one", oracle), game_of("one")
    mp = cm.cr.map[0]
    game.mccfr_traverse(5, 0, 3, 4)
    d = game.mccfr_delta_get()
    ctx.team_set_deal(deal_set("one")[0])
    ctx.team_mccfr_traverse(5, 3, 4)
    d1 = ctx.team_mccfr_delta_get()
    assert np.array_equal(d[mp, 4], d1[:, 4]) and d[:, 4].sum() == 4 * 2 * CM.PER_TRAVERSAL
    dR, cnt, A = cm.traverse(cm.tables()[0], SEED, 5, 0, 3, 4)
    assert np.array_equal(d[:, 4], cnt)
    assert in_budget(d[:, :4], dR, A, "chance form") and in_budget(d1[:, :4], dR[mp], A[mp], "one-deal form")
    assert in_budget(d[mp, :4], d1[:, :4], A[mp], "chance form against one-deal form", k=2.0)
    R, S = game.tables_get()
    assert not R.any() and not S.any() and game.mccfr_counters() == (4 * DRAWS, 4 * TERMINALS, 0)     # walks write only the delta buffer


@pytest.mark.parametrize("seed,iteration,b0", CM.WORD_CASES, ids=W.case_id)
def test_traverse_at_wide_philox_words(ctx, oracle, game_of, seed, iteration, b0):
    """the six Philox words at their wide ends on the LAST deal of `swap` (first = b0 + deal * 0): the count column exact, the increments in the budget;
    tests/test_team_chance_mccfr_ref.py::test_wide_word_traversals_separate asserts that a narrowed word would give other counts"""
    cm, game, nb = ref_of("swap", oracle), game_of("swap"), CM.WORD_NB
    ctx.mccfr_seed(seed)
    deal = game.n - 1
    game.mccfr_traverse(iteration, deal, b0, nb)
    d = game.mccfr_delta_get()
    dR, cnt, A = cm.traverse(cm.tables()[0], seed, iteration, deal, b0, nb)
    assert np.array_equal(d[:, 4], cnt) and cnt.sum() == nb * 2 * CM.PER_TRAVERSAL
    assert in_budget(d[:, :4], dR, A, "wide words")
    R, S = game.tables_get()
    assert not R.any() and not S.any() and game.mccfr_counters() == (nb * DRAWS, nb * TERMINALS, 0)


def test_iterations_under_a_wide_seed(ctx, oracle, game_of):
    """ids deal * batch + i under a seed with a high word: over all deals (iteration 0), then over a list whose order is not ascending (iteration 1), so
    that `first` follows the deal and not its slot"""
    cm, game = ref_of("swap", oracle), game_of("swap")
    ctx.mccfr_seed(W.WIDE_SEED)
    check_iteration(game, cm, CM.WORD_BATCH, None, "wide seed, all deals", seed=W.WIDE_SEED)
    check_iteration(game, cm, CM.WORD_BATCH, CM.WORD_LIST, "wide seed, deals [1, 0]", seed=W.WIDE_SEED)
    assert game.mccfr_counters() == (2 * game.n * CM.WORD_BATCH * DRAWS, 2 * game.n * CM.WORD_BATCH * TERMINALS, 2)


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------------
def test_copies_draw_independent_traversals(ctx, game_of):
    game = game_of("copies")
    _, mp = game.index()
    game.mccfr_walk(0, 8)
    cnt = game.mccfr_delta_get()[:, 4]
    ctx.team_set_deal(deal_set("one")[0])
    ctx.team_mccfr_traverse(0, 0, 16)
    assert np.array_equal(cnt[mp[0]], ctx.team_mccfr_delta_get()[:, 4]) and cnt.sum() == 16 * 2 * CM.PER_TRAVERSAL
    game.mccfr_apply()
    game.tables_reset()
    game.mccfr_iterate(8)                                            # the iteration counter is 1 now: other words, the same number of visits
    S = game.tables_get()[1]
    assert abs(S.sum() - 16 * 2 * CM.PER_TRAVERSAL) < 1e-6 and game.mccfr_counters() == (2 * 16 * DRAWS, 2 * 16 * TERMINALS, 2)


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------------------
def test_split_independence(oracle, game_of):
    """traverse(9, 1, 0, 64) against traverse(9, 1, 0, 17) + traverse(9, 1, 17, 47) before one apply, on deal 1 of `swap`"""
    cm, game = ref_of("swap", oracle), game_of("swap")
    R, S, sig = cm.tables()
    dR, cnt, A = cm.traverse(R, SEED, 9, 1, 0, 64)
    cm.apply(R, S, sig, dR, cnt)
    got = []
    for cuts in ([(0, 64)], [(0, 17), (17, 47)]):
        game.tables_reset()
        for b0, nb in cuts:
            game.mccfr_traverse(9, 1, b0, nb)
        assert np.array_equal(game.mccfr_delta_get()[:, 4], cnt)
        game.mccfr_apply()
        Rg, Sg = game.tables_get()
        assert np.array_equal(bits(Sg), bits(S)) and in_budget(Rg, R, A, str(cuts))
        got.append(Rg)
    assert in_budget(got[1], got[0], A, "split against whole", k=2.0)
    assert game.mccfr_counters() == (2 * 64 * DRAWS, 2 * 64 * TERMINALS, 2)


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------------------
def test_deal_lists(sl, oracle, game_of):
    cm, game = ref_of("six", oracle), game_of("six")
    rng = np.random.default_rng(11)
    legal = np.arange(4)[None, :] < cm.cr.nleg[:, None]
    R0, S0 = np.where(legal, rng.standard_normal((cm.G, 4)), 0.0), np.where(legal, rng.random((cm.G, 4)), 0.0)
    listed = np.zeros(cm.G, bool)
    listed[cm.cr.map[[0, 3, 5]].reshape(-1)] = True
    got = []
    for deals in ([0, 3, 5], [5, 0, 3]):
        game.tables_set(R0, S0)
        sig0 = game.sigma_get()
        game.mccfr_walk(4, 8, deals)
        cnt = game.mccfr_delta_get()[:, 4]
        game.mccfr_apply()
        R, S, sig = state_of(game)
        assert cnt.sum() == 3 * 8 * 2 * CM.PER_TRAVERSAL and not cnt[~listed].any()
        for a, b in ((R, R0), (S, S0), (sig, sig0)):
            assert np.array_equal(bits(a[~listed]), bits(b[~listed]))
        got.append((cnt, S, R))
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(bits(got[0][1]), bits(got[1][1]))
    dR, cnt, A = cm.delta(R0, SEED, 4, 8, [0, 3, 5])
    assert np.array_equal(got[0][0], cnt) and in_budget(got[0][2], R0 + dR, A, "[0, 3, 5]") and in_budget(got[1][2], R0 + dR, A, "[5, 0, 3]")
    before, counters = state_of(game), game.mccfr_counters()
    with pytest.raises(sl.ScopaError) as e:
        game.mccfr_iterate(8, 1, [[0, 3, 3]])
    assert e.value.status == sl.SCOPA_EINVAL and game.mccfr_counters() == counters
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(state_of(game), before)) and not game.mccfr_delta_get().any()
    check_iteration(game, cm, 8, [4, 1], "an iterate call with a list")


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------------------
def edge_regrets(case, nleg):
    """all-negative and one-hot: oracle/mccfr_edges.py's tables; nan / inf / neginf: a standard-normal table with that value in one legal cell of every 5th
    row (slot row mod b), and for inf a second +inf in every 35th row"""
    if case in ("allneg", "onehot"):
        return E.edge_table(case, nleg)
    rows = np.arange(nleg.size)
    R = np.where(np.arange(4)[None, :] < nleg[:, None], np.random.RandomState(3).randn(nleg.size, 4), 0.0)
    fifth = rows % 5 == 0
    R[rows[fifth], (rows % nleg)[fifth]] = {"nan": np.nan, "inf": np.inf, "neginf": -np.inf}[case]
    if case == "inf":
        R[::35, 0] = np.inf
        R[::35, 1] = np.inf
    return R


@pytest.mark.parametrize("case", ["allneg", "onehot", "nan", "inf", "neginf"])
def test_edge_regret_tables(oracle, game_of, case):
    cm, game = ref_of("swap", oracle), game_of("swap")
    R0 = edge_regrets(case, cm.cr.nleg)
    S0 = (1.0 + np.arange(R0.size, dtype=np.float64).reshape(-1, 4) % 7) * (np.arange(4)[None, :] < cm.cr.nleg[:, None])
    game.tables_set(R0, S0)
    cnt, A = check_iteration(game, cm, 3, None, case, exact=E.same_bits_or_same_nonfinite)
    if case == "onehot":
        assert (A.sum(1)[cnt > 0] == 0).sum() > 0                      # visited rows below a probability-0 loop child: weight 0, nothing added
    if case in ("nan", "inf"):
        assert not np.isfinite(game.tables_get()[0][cnt > 0]).all()


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------------------
def test_an_mccfr_iteration_then_exact_cfr(oracle, game_of):
    """the apply leaves the sigma rows as the CFR reduce leaves them: one CFR iteration from the device's tables equals ChanceRef.iterate from the same
    tables with sigma recomputed on the host, bit for bit"""
    cm, game = ref_of("swap", oracle), game_of("swap")
    game.mccfr_iterate(2)
    R, S = game.tables_get()
    sig = cm.cr.sigma(R)
    assert np.count_nonzero(S.any(1)) > 3000 and not np.array_equal(sig, cm.cr.sigma(np.zeros_like(R)))
    rv_want = cm.cr.iterate(R, S, sig, 1)
    rv = game.cfr_iterate(1, root_values=True)
    Rg, Sg, sigg = state_of(game)
    assert np.array_equal(bits(rv), bits(rv_want))
    assert np.array_equal(bits(Rg), bits(R)) and np.array_equal(bits(Sg), bits(S)) and np.array_equal(bits(sigg), bits(sig))


# ---- 9 ---------------------------------------------------------------------------------------------------------------------------------------
def test_contracts(sl, game_of):
    L, game = sl.lib(), game_of("swap")
    lst = lambda *ids: np.array(ids, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    it = lambda n_iters, batch, m=0, deals=None: L.scopa_team_chance_mccfr_iterate(game._h, n_iters, batch, m, None if deals is None else p(deals))
    tr = lambda deal, b0, nb: L.scopa_team_chance_mccfr_traverse(game._h, 0, deal, b0, nb)
    bad = [it(1, 0), it(1, (1 << 24) + 1), it(-1, 4), it((1 << 20) + 1, 4), tr(0, 0, (1 << 24) + 1), tr(0, 0xFFFFFFFF, 1), tr(0, 0xFFFFFF00, 0x101), tr(-1, 0, 1), tr(2, 0, 1),
           it(1, 4, 2, lst(0, 2)), it(1, 4, 2, lst(-1, 0)), it(1, 4, 2, lst(1, 1)), it(2, 4, 2, lst(0, 1, 0, 0)), it(1, 4, 0, lst(0)), it(1, 4, 3, lst(0, 1, 0)),
           L.scopa_team_chance_mccfr_walk(game._h, 0, 0, 0, None), L.scopa_team_chance_mccfr_walk(game._h, 0, 4, 2, p(lst(1, 1)))]
    assert bad == [sl.SCOPA_EINVAL] * len(bad)
    assert it(0, 0) == sl.SCOPA_EINVAL and it(0, 4) == sl.SCOPA_OK and it(0, 4, 2, lst()) == sl.SCOPA_OK and tr(1, 7, 0) == sl.SCOPA_OK and tr(1, 0xFFFFFFFF, 0) == sl.SCOPA_OK
    R, S = game.tables_get()
    assert not R.any() and not S.any() and not game.mccfr_delta_get().any() and game.mccfr_counters() == (0, 0, 0)
    game.mccfr_iterate(2, 2, [[1, 0], [0, 1]])                       # the same list in both orders is two valid iterations
    assert game.mccfr_counters() == (2 * 2 * 2 * DRAWS, 2 * 2 * 2 * TERMINALS, 2)
    game.mccfr_traverse(0, 0, 0, 2)
    game.tables_reset()                                              # tables and pending walks go, the counters stay
    assert not game.mccfr_delta_get().any() and not game.tables_get()[1].any() and game.mccfr_counters() == (10 * DRAWS, 10 * TERMINALS, 2)


# ---- 10 --------------------------------------------------------------------------------------------------------------------------------------
def test_it_solves(ctx):
    """solve_mccfr on `six` at batch 16 for 40 iterations ends below the uniform policy of the zero tables.  Chosen on the CPU: the restatement with the
    same batch, seed and iteration numbers goes from exploitability 4.5931713 (uniform) to 3.4644928 after 20 iterations and 3.1803049 after 40
    (ChanceRef.exploitability of ChanceRef.average_policy).  Only the drop is asserted."""
    from scopa_amd.algorithms import team_chance
    game, iters, curve = team_chance.solve_mccfr(deal_set("six"), 16, eps=0.0, max_iters=40, check_every=20, seed=SEED, device=ctx)
    print(curve)
    assert iters == 40 and [t for t, _ in curve] == [20, 40] and game.mccfr_counters()[2] == 40
    game.tables_reset()
    uniform = float(game.exploitability()[0])
    print("uniform:", uniform)
    assert 0.0 <= curve[-1][1] < uniform
    game.close()
