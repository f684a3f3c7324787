"""GPU checks of the deal-sampled and simultaneous iterations of Team MiniScopa over a set of deals (scopa_team_chance_cfr_iterate_sampled,
TeamChanceGame.cfr_iterate_sampled, algorithms.team_chance.solve(sample=, alternating=)) against the float64 restatement
tests/team_chance_sampled_ref.py, which tests/test_team_chance_sampled_ref.py pins to team_chance_ref.ChanceRef, and against cfr_iterate itself.

Everything is compared bit for bit: every row has one writer and every float64 sum a fixed order.  The deal sets are those of
tests/team_chance_sets.py (the tree is fixed at 321 365 rows per deal, so 2 to 6 deals are the smallest shapes); three iterations each; the
restatement's runs are computed once per process and handed out read-only."""
import numpy as np
import pytest

import team_chance_sampled_ref as SR
import team_chance_sets as TS
from test_gpu_team_chance import bits
from test_gpu_team_chance_shared import same_tables

pytestmark = pytest.mark.gpu

HIDDEN_LISTS = [[1, 3, 4], [0, 5, 2], [4, 1, 3]]
BOTH_LISTS = [[1, 3], [0, 1], [2, 0]]


@pytest.fixture()
def game_of(sl, ctx, oracle):
    games = []

    def make(perms):
        games.append(sl.TeamChanceGame(TS.deal_set(perms) if isinstance(perms, str) else perms, ctx))
        return games[-1]
    yield make
    for g in games:
        g.close()


def sampled_ref(name):
    return TS.cached(("sampled ref", name), lambda: SR.SampledRef(TS.chance_ref(name)))


def ref_run(name, variant, lists, alternating):
    """(R, S, sigma, root values) of the restatement after the iterations `lists` of `variant` from reset, read-only"""
    def make():
        from scopa_amd.algorithms import schedule
        sr = sampled_ref(name)
        R, S, sig = sr.cr.tables()
        rv = sr.iterate(R, S, sig, lists, schedule(variant, 0, len(lists)), alternating)
        for a in (R, S, sig, rv):
            a.setflags(write=False)
        return R, S, sig, rv
    return TS.cached(("sampled run", name, variant, repr(lists), alternating), make)


def listed_counts(sr, lst):
    """listed occurrences of every global row under the list `lst`"""
    return np.diff(sr.sub(lst).occ_off)


# ---- 1: hidden6, three of six deals ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["vanilla", "cfr+", "dcfr"])
def test_hidden6_lists_against_the_restatement(game_of, variant):
    """Even-depth rows have 1, 2, 3 or 6 occurrences: under [1, 3, 4] a row's sum starts at a listed occurrence that is not the row's first; the
    odd-depth rows of the unlisted deals have no listed occurrence and take +0.0"""
    from scopa_amd.algorithms import schedule
    sr = sampled_ref("hidden6")
    cr = sr.cr
    cnt = listed_counts(sr, HIDDEN_LISTS[0])
    first_deal = cr.occ[cr.occ_off[:-1]] // 321365
    assert ((cnt > 0) & ~np.isin(first_deal, HIDDEN_LISTS[0]) & (cr.depth % 2 == 0)).sum() > 1000      # starts past the row's first occurrence
    assert ((cnt == 0) & (cr.depth % 2 == 1)).sum() > 100000                                            # the +0.0 path
    want = ref_run("hidden6", variant, HIDDEN_LISTS, True)
    game = game_of("hidden6")
    rv = game.cfr_iterate_sampled(HIDDEN_LISTS, schedule(variant, 0, 3), alternating=True, root_values=True)
    print("root values", rv.tolist(), want[3].tolist())
    assert same_tables(game, want[:3], f"hidden6 {variant}")
    assert np.array_equal(bits(rv), bits(want[3]))


# ---- 2: both4, two of four deals, alternating and simultaneous ------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,alternating", [("cfr+", 1), ("cfr+", 0), ("dcfr", 1), ("dcfr", 0)])
def test_both4_lists_against_the_restatement(game_of, variant, alternating):
    from scopa_amd.algorithms import schedule
    sr = sampled_ref("both4")
    seen = [set() for _ in range(12)]
    for lst in BOTH_LISTS:
        cnt = listed_counts(sr, lst)
        for d in range(12):
            seen[d] |= set(np.unique(cnt[sr.cr.depth == d]).tolist())
    assert all(s >= {0, 1, 2} for s in seen), seen                                 # rows with 0, 1 and 2 listed occurrences at every depth
    want = ref_run("both4", variant, BOTH_LISTS, bool(alternating))
    game = game_of("both4")
    rv = game.cfr_iterate_sampled(BOTH_LISTS, schedule(variant, 0, 3), alternating=alternating, root_values=True)
    print("root values", rv.tolist(), want[3].tolist())
    assert same_tables(game, want[:3], f"both4 {variant} alternating={alternating}")
    assert np.array_equal(bits(rv), bits(want[3]))
    if not alternating:
        assert np.all(rv[:, 1] == -rv[:, 0])                                        # both sweeps read one sigma


# ---- 3: m = n is cfr_iterate ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hidden6", "reordered"])
def test_full_lists_are_cfr_iterate(game_of, name):
    from scopa_amd.algorithms import schedule
    w = schedule("dcfr", 0, 3)
    exact, game = game_of(name), game_of(name)
    n = game.n
    rv_want = exact.cfr_iterate(w, root_values=True)
    want = (*exact.tables_get(), exact.sigma_get())
    full = np.array([np.roll(np.arange(n)[::-1], k) for k in range(3)], np.int32)
    again = np.ascontiguousarray(full[:, ::-1])                                    # the same lists, the ids of each row in another order
    assert not np.array_equal(full, again) and np.array_equal(np.sort(full), np.sort(again))
    for what, deals, weights in (("NULL list", None, w), ("permuted full list", full, w), ("the same call again", full, w), ("ids permuted", again, w)):
        game.tables_reset()
        rv = game.cfr_iterate_sampled(deals, weights, alternating=True, root_values=True)
        assert same_tables(game, want, f"{name} {what}"), what
        assert np.array_equal(bits(rv), bits(rv_want)), what


def test_sampled_runs_repeat_bit_for_bit(game_of):
    from scopa_amd.algorithms import schedule
    game = game_of("hidden6")
    got = []
    for deals in (HIDDEN_LISTS, HIDDEN_LISTS, [row[::-1] for row in HIDDEN_LISTS]):
        game.tables_reset()
        rv = game.cfr_iterate_sampled(deals, schedule("dcfr", 0, 3), alternating=False, root_values=True)
        got.append((*game.tables_get(), game.sigma_get(), rv))
    for other in got[1:]:
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got[0], other))


# ---- 4: sampled, exact and simultaneous iterations and the best response on one handle ---------------------------------------------------------------
def test_mixed_calls_on_one_handle(game_of):
    from scopa_amd.algorithms import schedule
    w = schedule("dcfr", 0, 3)

    def make():
        sr = sampled_ref("both4")
        R, S, sig = sr.cr.tables()
        rv = [sr.iterate(R, S, sig, [[1, 3]], w[0:1], True), sr.cr.iterate(R, S, sig, weights=w[1:2]), sr.iterate(R, S, sig, [[0, 1]], w[2:3], False)]
        out4 = sr.cr.exploitability(sr.cr.average_policy(S))[0]
        for a in (R, S, sig, out4):
            a.setflags(write=False)
        return R, S, sig, np.concatenate(rv), out4
    R, S, sig, rv_want, out4_want = TS.cached(("sampled mixed", "both4"), make)
    game = game_of("both4")
    rv = [game.cfr_iterate_sampled([[1, 3]], w[0:1], alternating=True, root_values=True), game.cfr_iterate(w[1:2], root_values=True),
          game.cfr_iterate_sampled([[0, 1]], w[2:3], alternating=False, root_values=True)]
    out4 = game.exploitability()
    assert same_tables(game, (R, S, sig), "mixed")
    assert np.array_equal(bits(np.concatenate(rv)), bits(rv_want))
    print(out4, out4_want)
    assert np.array_equal(bits(out4), bits(out4_want))


# ---- 5: refusals ---------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(sl, game_of):
    game = game_of("both4")
    n = game.n
    game.cfr_iterate_sampled([[1, 3]], [(0.5, 0.25, 0.75)])                        # tables away from zero
    before = (*game.tables_get(), game.sigma_get())
    ok = [[0, 1], [2, 3]]
    ones = np.ones((2, 3))
    cases = {"m = 0 with a list": (np.zeros((1, 0), np.int32), None, 1), "m = n + 1": ([list(range(n + 1))], None, 1), "an id of n": ([[0, n]], None, 1),
             "an id of -1": ([[-1, 0]], None, 1), "a repeated id in the second iteration": ([[0, 1], [2, 2]], None, 1), "alternating = 2": (ok, None, 2),
             "a weight of 1.5": (ok, [(1.0, 1.0, 1.0), (1.0, 1.5, 1.0)], 1), "a NaN weight": (ok, [(1.0, 1.0, 1.0), (float("nan"), 1.0, 1.0)], 1),
             "a negative weight": (ok, -0.5 * ones, 0), "n_iters = -1": (None, -1, 1), "n_iters above 2^20": (None, (1 << 20) + 1, 0),
             "alternating = -1 without a list": (None, 2, -1)}
    for what, (deals, weights, alternating) in cases.items():
        with pytest.raises(sl.ScopaError) as e:
            game.cfr_iterate_sampled(deals, weights, alternating=alternating, root_values=True)
        assert e.value.status == sl.SCOPA_EINVAL, what
        assert same_tables(game, before, what), what
    assert game.cfr_iterate_sampled(None, 0, root_values=True).shape == (0, 2)     # n_iters = 0: a no-op
    assert game.cfr_iterate_sampled(np.zeros((0, 2), np.int32), alternating=False) is None
    assert same_tables(game, before, "n_iters = 0")


# ---- 6: the host loop -------------------------------------------------------------------------------------------------------------------------------------
def test_solve_with_sampled_deals(game_of):
    from scopa_amd.algorithms import schedule, team_chance
    from scopa_amd.algorithms.chance import sample_deals
    from test_gpu_team_chance import PACKETS
    perms = team_chance.packet_deals(PACKETS, fix_seat0=True)
    solved, iters, curve = team_chance.solve(perms, "dcfr", max_iters=6, check_every=3, sample=3, seed=7)
    try:
        assert iters == 6 and [t for t, _ in curve] == [3, 6] and all(np.isfinite(e) for _, e in curve)
        want = (*solved.tables_get(), solved.sigma_get())
    finally:
        solved.close()
    game = game_of(perms)
    for t in (0, 3):
        lists = sample_deals(6, 3, t, 3, 7)
        assert lists.shape == (3, 3)
        game.cfr_iterate_sampled(lists, schedule("dcfr", t, 3))
    assert same_tables(game, want, "solve")
    assert float(game.exploitability()[0]) == curve[-1][1]
