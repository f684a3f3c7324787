"""GPU checks of Team MiniScopa over a set of deals (scopa_team_chance.hip, scopa_team_chance_mccfr.hip) on deal sets whose rows are shared BELOW
depth 1 (tests/team_chance_sets.py: both4, reordered, hidden6).  The packet deals of tests/test_gpu_team_chance.py and
tests/test_gpu_team_chance_mccfr.py share rows at depths 0 and 1 only; here a row of any depth has up to 6 occurrences, so the reduce's fixed-order
sum runs on the rows the subtree kernel writes, the best response's choice adds q over several deals at every responder level, MCCFR delta rows of
depth 5 or more take float64 atomics from the workgroups of several deals and the LDS accumulator of depths 0..4 is flushed into shared rows.

The restatements (tests/team_chance_ref.py, tests/team_chance_mccfr_ref.py) are pinned on these sets by tests/test_team_chance_ref.py and
tests/test_team_chance_mccfr_ref.py.  The comparisons are those of the two existing files, imported from them: bit for bit for everything with one
writer per row and a fixed order, the project's reorder budget for the MCCFR regrets.  References are computed once per process, read-only."""
import numpy as np
import pytest

import cfr_edges as E
import team_chance_mccfr_ref as CM
import team_chance_sets as TS
import test_gpu_team_chance as GC
import test_gpu_team_chance_mccfr as GM
from test_gpu_team_chance import bits, random_policy, uniform_policy
from test_gpu_team_chance_mccfr import SEED, check_iteration, in_budget, state_of

pytestmark = pytest.mark.gpu

DRAWS, TERMINALS = CM.DRAWS, CM.TERMINALS


@pytest.fixture()
def game_of(sl, ctx, oracle):
    games = []
    ctx.mccfr_seed(SEED)

    def make(name):
        games.append(sl.TeamChanceGame(TS.deal_set(name), ctx))
        return games[-1]
    yield make
    for g in games:
        g.close()


def same_tables(game, want, what=""):
    R, S = game.tables_get()
    sig = game.sigma_get()
    cells = [int(np.count_nonzero(bits(a) != bits(b))) for a, b in ((R, want[0]), (S, want[1]), (sig, want[2]))]
    print(what, "cells that differ (R, S, sigma):", cells)
    return cells == [0, 0, 0]


# ---- 1: the index and the exact iterations ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,variant", [("both4", "vanilla"), ("both4", "cfr+"), ("both4", "dcfr"), ("hidden6", "vanilla"), ("hidden6", "cfr+"), ("hidden6", "dcfr"),
                                          ("reordered", "dcfr")])
def test_iterations_against_the_restatement(game_of, name, variant):
    from scopa_amd.algorithms import schedule
    cr = TS.chance_ref(name)
    R_want, S_want, sig_want, rv_want = TS.ref_run(name, variant)
    game = game_of(name)
    keys, mp = game.index()
    assert (game.n, game.G, game.n_occurrences) == (cr.n, TS.ROWS[name], cr.n * 321365)
    assert np.array_equal(keys, cr.gkey) and np.array_equal(mp, cr.map)
    rv = game.cfr_iterate(schedule(variant, 0, 3), root_values=True)
    assert same_tables(game, (R_want, S_want, sig_want), f"{name} {variant}")
    assert np.array_equal(bits(rv), bits(rv_want))


# ---- 2: every shared row of `reordered` is twice the one-deal solver's row ---------------------------------------------------------------------
def test_reordered_against_the_one_deal_solver(ctx, game_of):
    """The two deals of `reordered` are one deal stored twice, seat 0's hand in another order: seats 1, 2 and 3 own rows with 2 occurrences whose
    increments are those of the one-deal solver (scopa_team_cfr.hip) on the base deal, added twice; seat 0's rows, one occurrence each, are its rows.
    Not bit for bit: in the second deal seat 0's slots name other cards, so its 4-term dot products add in another order and everything above them
    differs in its last bits.  Measured on the CPU, the restatement against 2 * team_cfr_ref.Ref after 3 unweighted iterations: the largest
    |difference| is 1.78e-15 in the shared regrets (values up to 7.8), 3.4e-16 in the shared strategy sums (up to 3.0), 2.3e-16 in sigma, 6.7e-16 in seat
    0's regrets, 0 in seat 0's strategy sums and in the root values; no regret-matching tie amplifies it (after 1 iteration 2.3e-16, after 2 1.9e-16).
    The bounds are 4 x those figures, the margin for the device's fused multiply-adds; an unmeasured 0 is held to 4 x 2^-52."""
    cr, game = TS.chance_ref("reordered"), game_of("reordered")
    _, mp = game.index()
    assert np.array_equal(mp, cr.map)
    rv = game.cfr_iterate(3, root_values=True)
    R, S = game.tables_get()
    sig = game.sigma_get()
    ctx.team_set_deal(TS.deal_set("reordered")[0])
    rv1 = ctx.team_cfr_iterate(3, None)
    R1, S1, L1, _ = ctx.team_tables_get()
    twice = np.diff(cr.occ_off) == 2
    shared = twice[mp[0]]
    assert shared.sum() == 321365 - (1 + 256 + 20736)                          # all but seat 0's rows, depths 0, 4 and 8
    # the second deal reaches the same shared rows through other local rows
    assert np.array_equal(np.sort(mp[0][shared]), np.sort(mp[1][twice[mp[1]]])) and np.count_nonzero(mp[0][shared] != mp[1][shared]) > 1000
    eps = 2.0 ** -52
    worst = {}
    for what, got, want, tol in (("R shared", R[mp[0]][shared], 2.0 * R1[shared], 4 * 1.78e-15), ("S shared", S[mp[0]][shared], 2.0 * S1[shared], 4 * 3.4e-16),
                                 ("sigma shared", sig[mp[0]][shared], L1[shared], 4 * 2.3e-16), ("R seat 0", R[mp[0]][~shared], R1[~shared], 4 * 6.7e-16),
                                 ("S seat 0", S[mp[0]][~shared], S1[~shared], 4 * eps), ("sigma seat 0", sig[mp[0]][~shared], L1[~shared], 4 * 2.3e-16),
                                 ("root values", rv, rv1, 4 * eps)):
        worst[what] = (float(np.abs(got - want).max()), tol)
    print(worst)
    assert all(err <= tol for err, tol in worst.values()), worst


# ---- 3: edge tables, on all rows, on the shared rows only, on the single rows only ---------------------------------------------------------------
@pytest.mark.parametrize("case,w,occurrences", [("allneg", (1.0, 0.0, 1.0), None), ("onehot", (0.0, 1.0, 0.0), None), ("nan", (1.0, 1.0, 1.0), None), ("inf", (0.5, 0.0, 1.0), None),
                                                ("neginf", (1.0, 0.0, 0.0), None), ("big", None, None), ("nan", (1.0, 1.0, 1.0), 2), ("nan", (1.0, 1.0, 1.0), 1)])
def test_edge_tables_one_iteration(game_of, case, w, occurrences):
    """tests/test_gpu_team_chance.py::test_edge_tables_one_iteration's cases on both4, whose rows of 2 occurrences lie at every depth; `occurrences`:
    the edge values only in the rows with that many occurrences, zero tables elsewhere"""
    cr, game = TS.chance_ref("both4"), game_of("both4")
    R0, S0 = GC.edge_tables(case, cr)
    if occurrences is not None:
        keep = (np.diff(cr.occ_off) == occurrences)[:, None]
        assert 1000 < keep.sum() < cr.G - 1000
        R0, S0 = np.where(keep, R0, 0.0), np.where(keep, S0, 0.0)
    game.tables_set(R0, S0)
    R, S = R0.copy(), S0.copy()
    sig = cr.sigma(R)
    nonfinite = case in ("nan", "inf", "neginf")
    same = E.same_bits_or_same_nonfinite if nonfinite else E.same_bits
    assert same(game.sigma_get(), sig), "sigma after tables_set"
    rv_want = cr.iterate(R, S, sig, 1) if w is None else cr.iterate(R, S, sig, weights=[w])
    rv = game.cfr_iterate(1 if w is None else [w], root_values=True)
    Rg, Sg = game.tables_get()
    assert same(Rg, R) and same(Sg, S) and same(game.sigma_get(), sig) and same(rv, rv_want)


# ---- 4: exploitability ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["both4", "hidden6"])
def test_exploitability_against_the_restatement(ctx, game_of, name):
    from scopa_amd.algorithms import schedule
    cr, game = TS.chance_ref(name), game_of(name)
    _, S_want, _, _ = TS.ref_run(name, "cfr+")
    game.cfr_iterate(schedule("cfr+", 0, 3))
    perms = TS.deal_set(name)
    for what, pol in (("average", None), ("caller", random_policy(cr, 3)), ("uniform", uniform_policy(cr))):
        want4, brs, per_deal = TS.cached(("expl", name, what), lambda: cr.exploitability(cr.average_policy(S_want) if pol is None else pol))
        out4, evaluated, br = game.exploitability(pol, return_policy=True, return_br=True)
        print(name, what, out4, want4)
        assert np.array_equal(bits(evaluated), bits(cr.average_policy(S_want) if pol is None else pol))
        assert np.array_equal(bits(out4), bits(want4))
        for t in (0, 1):
            differ = np.nonzero((bits(br[t]) != bits(brs[t])).any(1))[0]
            assert differ.size == 0, (what, t, differ.size, np.bincount(cr.depth[differ], minlength=12), np.bincount(np.diff(cr.occ_off)[differ]))
        assert np.array_equal(bits(game.exploitability(pol)), bits(out4))          # without the optional outputs
        # the value, deal by deal, is the one-deal policy value of the scattered table; following a returned table reproduces its best response
        vals = []
        for d in range(game.n):
            local = game.policy_for_deal(evaluated, d, as_tensor=True)
            assert np.array_equal(local.cpu().numpy(), evaluated[cr.map[d]])
            ctx.team_set_deal(perms[d])
            vals.append(ctx.team_policy_value(local.data_ptr(), local.data_ptr()))
        assert np.array_equal(bits(vals), bits(per_deal))
        s = vals[0]
        for v in vals[1:]:
            s = s + v
        assert s / float(game.n) == out4[3]
        assert game.exploitability(br[0])[3] == out4[1] and -game.exploitability(br[1])[3] == out4[2]


# ---- 5: the image holds the CFR increment rows and the best response's q rows ----------------------------------------------------------------------
def test_evaluations_between_iterations_leave_the_iterations_alone(game_of):
    """cfr, exploitability of a caller's policy with tables, cfr, exploitability, cfr: the best response's q rows overwrite the first half of shared
    and unshared increment rows of both teams; the three iterations are the restatement's three with no evaluation in between"""
    cr, game = TS.chance_ref("both4"), game_of("both4")
    want = TS.ref_run("both4", "vanilla")
    rv = [game.cfr_iterate(1, root_values=True)]
    game.exploitability(random_policy(cr, 7), return_br=True)
    rv.append(game.cfr_iterate(1, root_values=True))
    game.exploitability()
    rv.append(game.cfr_iterate(1, root_values=True))
    assert same_tables(game, want[:3]) and np.array_equal(bits(np.concatenate(rv)), bits(want[3]))


def test_sampled_iterations_between_exact_ones(game_of):
    """cfr, exploitability, MCCFR at batch 3, cfr: the first iteration is the restatement's; the last is the restatement's from the device's own tables
    after the sampled iteration, with sigma recomputed on the host"""
    cr, game = TS.chance_ref("both4"), game_of("both4")
    want = TS.ref_run("both4", "vanilla", 1)
    rv = game.cfr_iterate(1, root_values=True)
    assert same_tables(game, want[:3], "first") and np.array_equal(bits(rv), bits(want[3]))
    game.exploitability(random_policy(cr, 7), return_br=True)
    game.mccfr_iterate(3)
    R, S = game.tables_get()
    changed = (bits(R) != bits(want[0])).any(1), (bits(S) != bits(want[1])).any(1)
    assert changed[0].sum() > 100 and changed[1].sum() > 1000                    # the sampled iteration did change the tables
    sig = cr.sigma(R)
    assert np.array_equal(bits(game.sigma_get()), bits(sig))
    rv_want = cr.iterate(R, S, sig, 1)
    rv = game.cfr_iterate(1, root_values=True)
    assert same_tables(game, (R, S, sig), "last") and np.array_equal(bits(rv), bits(rv_want))


# ---- 6: MCCFR iterations -----------------------------------------------------------------------------------------------------------------------
class Witness(CM.ChanceMCRef):
    """the restatement, which also notes the rows an iteration's walks visit from more than one deal and asserts -- inside iterate, so before
    check_iteration calls the device -- that some are of depth 5 or more (float64 atomics from several deals' workgroups) and, from iteration
    `shallow_from` on, some of depths 2..4 (the LDS accumulator flushed into a shared row below depth 1)"""

    def __init__(self, name, shallow_from=0):
        super().__init__(TS.deal_set(name), TS.chance_ref(name))
        self.shallow_from, self.seen, self.log = shallow_from, None, []

    def deal_delta(self, R, seed, iteration, deal, first, nb):
        out = super().deal_delta(R, seed, iteration, deal, first, nb)
        if self.seen is not None:
            self.seen[self.cr.map[deal][out[1] > 0]] += 1
        return out

    def iterate(self, R, S, sig, batch, seed, iteration, deals=None):
        self.seen = np.zeros(self.G, np.int64)
        out = super().iterate(R, S, sig, batch, seed, iteration, deals)
        depth = self.cr.depth[self.seen > 1]
        self.seen = None
        deep, shallow = int((depth >= 5).sum()), int(((depth >= 2) & (depth <= 4)).sum())
        self.log.append((iteration, deep, shallow))
        print("iteration", iteration, "rows visited from several deals: depth 5 or more", deep, "depths 2..4", shallow)
        assert deep > 0 and (shallow > 0 or iteration < self.shallow_from)
        return out


@pytest.mark.parametrize("name,batch,shallow_from", [("both4", 1, 0), ("both4", 3, 0), ("both4", 64, 0), ("hidden6", 3, 0), ("reordered", 3, 1)])
def test_mccfr_iterations_against_the_restatement(game_of, name, batch, shallow_from):
    """three iterations from the device's own tables.  Measured with the restatement, rows visited from several deals (depth 5 or more / depths 2..4):
    both4 at batch 1: 22 / 4, 17 / 2, 40 / 9; at batch 3: 113 / 21, 102 / 21, 238 / 21; at batch 64: 13 782 / 382, 1 176 / 42, 942 / 32; hidden6 at
    batch 3: 209 / 94, 436 / 98, 809 / 73; reordered at batch 3: 192 / 0, 858 / 5, 872 / 10.  In `reordered` depth 4 is seat 0's, whose rows are not
    shared, and the six traversals of the uniform first iteration meet in none of the 80 rows of depths 2 and 3: its shallow condition holds from
    the second iteration on"""
    cm, game = Witness(name, shallow_from), game_of(name)
    for it in range(3):
        check_iteration(game, cm, batch, None, f"{name}, batch {batch}, iteration {it + 1}")
    assert [x[0] for x in cm.log] == [0, 1, 2]
    assert game.mccfr_counters() == (3 * game.n * batch * DRAWS, 3 * game.n * batch * TERMINALS, 3)


# ---- 7: deal lists and split walks -----------------------------------------------------------------------------------------------------------------
def test_deal_lists(game_of):
    """tests/test_gpu_team_chance_mccfr.py::test_deal_lists on hidden6, where listed and unlisted deals share rows of every even depth"""
    cm, game = TS.chance_mc_ref("hidden6"), game_of("hidden6")
    rng = np.random.default_rng(11)
    legal = np.arange(4)[None, :] < cm.cr.nleg[:, None]
    R0, S0 = np.where(legal, rng.standard_normal((cm.G, 4)), 0.0), np.where(legal, rng.random((cm.G, 4)), 0.0)
    listed = np.zeros(cm.G, bool)
    listed[cm.cr.map[[0, 3, 5]].reshape(-1)] = True
    shared = np.diff(cm.cr.occ_off) > 1
    print("shared rows with only unlisted occurrences:", int((shared & ~listed).sum()), "by depth", np.bincount(cm.cr.depth[shared & ~listed], minlength=12))
    assert (shared & ~listed & (cm.cr.depth >= 2)).sum() > 0                  # rows shared among the unlisted deals 1, 2 and 4 alone
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
    assert (cnt[shared & (cm.cr.depth >= 5)] > 0).sum() > 0


def test_split_independence(game_of):
    """traverse(9, 1, 0, 64) against traverse(9, 1, 0, 17) + traverse(9, 1, 17, 47) before one apply, on deal 1 of both4"""
    cm, game = TS.chance_mc_ref("both4"), game_of("both4")
    R, S, sig = cm.tables()
    dR, cnt, A = cm.traverse(R, SEED, 9, 1, 0, 64)
    cm.apply(R, S, sig, dR, cnt)
    assert (cnt[(np.diff(cm.cr.occ_off) == 2) & (cm.cr.depth >= 5)] > 0).sum() > 100
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


# ---- 8: edge regret tables under MCCFR ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["allneg", "onehot", "nan", "inf", "neginf"])
def test_edge_regret_tables(game_of, case):
    cm, game = TS.chance_mc_ref("both4"), game_of("both4")
    R0 = GM.edge_regrets(case, cm.cr.nleg)
    S0 = (1.0 + np.arange(R0.size, dtype=np.float64).reshape(-1, 4) % 7) * (np.arange(4)[None, :] < cm.cr.nleg[:, None])
    game.tables_set(R0, S0)
    cnt, A = check_iteration(game, cm, 3, None, case, exact=E.same_bits_or_same_nonfinite)
    assert (cnt[np.diff(cm.cr.occ_off) == 2] > 0).sum() > 0
    if case == "onehot":
        assert (A.sum(1)[cnt > 0] == 0).sum() > 0                      # visited rows below a probability-0 loop child: weight 0, nothing added
    if case in ("nan", "inf"):
        assert not np.isfinite(game.tables_get()[0][cnt > 0]).all()
