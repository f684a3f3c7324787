"""GPU checks of policy against policy on Team MiniScopa (scopa_team_xplay.hip): the exact cross-play matrix and the sampled match, on one deal and
over a set of deals, against tests/team_xplay_ref.py bit for bit (float64 compared as uint64; the match's integers exactly) and against the entry
points that already compute some of the same numbers.  K = 3 on one deal, `reordered` (2 deals, a map that permutes local rows) and `hidden6` (6
deals, rows with 1, 2, 3 or 6 occurrences, an order-sensitive sum over deals).  tests/test_team_xplay_ref.py pins the restatement and guards that these
expectations separate.  References are computed once per process, read-only."""
import ctypes as C

import numpy as np
import pytest

import philox_words as W
import team_chance_sets as TS
import team_xplay_ref as X

pytestmark = pytest.mark.gpu

SETS = ("reordered", "hidden6")
BASE = TS.deal_set("reordered")[0]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def world(sl, oracle):
    """one context for the module, the games of the deal sets made at first use"""
    import torch
    try:
        ctx = sl.Context(0)
    except sl.ScopaError as e:
        if e.status == sl.SCOPA_ENODEV:
            pytest.skip("no GPU on this box")
        raise

    class World:
        games = {}
        dev = torch.device("cuda", ctx.device)

        def game(self, name, perms=None):
            if name not in self.games:
                self.games[name] = sl.TeamChanceGame(TS.deal_set(name) if perms is None else perms, ctx)
            return self.games[name]

        def put(self, a, dtype=None):
            return torch.as_tensor(np.array(a, dtype=dtype or np.float64, order="C"), device=self.dev)

        def cross(self, game, stack, per_deal=True):
            """-> (out [K][K][4], per_deal [n][K][K][4] or None) of a device stack [K][G][4]"""
            k = stack.shape[0]
            out = torch.full((k, k, 4), -7.0, dtype=torch.float64, device=self.dev)
            img = torch.full((game.n, k, k, 4), -7.0, dtype=torch.float64, device=self.dev) if per_deal else None
            torch.cuda.synchronize()
            game.cross_play(k, stack.data_ptr(), out.data_ptr(), img.data_ptr() if per_deal else 0)
            ctx.synchronize()
            return out.cpu().numpy(), (img.cpu().numpy() if per_deal else None)

        def cross_one(self, stack):
            k = stack.shape[0]
            out = torch.full((k, k, 4), -7.0, dtype=torch.float64, device=self.dev)
            torch.cuda.synchronize()
            ctx.team_cross_play(k, stack.data_ptr(), out.data_ptr())
            ctx.synchronize()
            return out.cpu().numpy()

    w = World()
    w.ctx, w.torch = ctx, torch
    yield w
    for g in w.games.values():
        g.close()
    ctx.close()


# ---- cross-play -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SETS)
def test_chance_cross_play_is_the_restatement_bit_for_bit(world, name):
    game = world.game(name)
    want_out, want_img = X.reference(name)
    stack = world.put(X.stack(name))
    out, img = world.cross(game, stack)
    print(name, "cells that differ (per deal, out):", int((bits(img) != bits(want_img)).sum()), int((bits(out) != bits(want_out)).sum()))
    assert np.array_equal(bits(img), bits(want_img)) and np.array_equal(bits(out), bits(want_out))
    again, img2 = world.cross(game, stack)
    assert np.array_equal(bits(again), bits(out)) and np.array_equal(bits(img2), bits(img))          # run to run
    scratch, none = world.cross(game, stack, per_deal=False)                                           # d_per_deal = NULL: the handle's own image
    assert none is None and np.array_equal(bits(scratch), bits(out))


def test_one_deal_and_a_one_deal_handle_give_the_same_bits(world):
    cr, ctx = TS.chance_ref("reordered"), world.ctx
    loc = [cr.policy_for_deal(p, 0) for p in X.stack("reordered")]
    want = X.reference("reordered")[1][0]                         # test_team_xplay_ref.py: equal to XRef.one(BASE) on these tables
    ctx.team_set_deal(BASE)
    out = world.cross_one(world.put(loc))
    assert np.array_equal(bits(out), bits(want))
    assert np.array_equal(bits(world.cross_one(world.put(loc))), bits(out))
    game = world.game("base alone", BASE.reshape(1, 16))
    _, mp = game.index()
    tabs = []
    for p in loc:
        t = np.zeros((game.G, 4))
        t[mp[0]] = p
        tabs.append(t)
    one, img = world.cross(game, world.put(tabs))
    assert np.array_equal(bits(one), bits(out)) and np.array_equal(bits(img[0]), bits(out))


@pytest.mark.parametrize("name", SETS)
def test_per_deal_image_is_the_one_deal_call_on_that_deal(world, name):
    """... with the policy_for_deal tables; scopa_team_set_deal between the calls rebuilds the leaf scopas, so every deal's scopa quantities are its own"""
    game, ctx, torch = world.game(name), world.ctx, world.torch
    stack = world.put(X.stack(name))
    _, img = world.cross(game, stack)
    want = X.reference(name)[1]
    for d in range(game.n):
        ctx.team_set_deal(TS.deal_set(name)[d])
        loc = torch.stack([game.policy_for_deal(stack[k], d, as_tensor=True) for k in range(3)]).contiguous()
        out = world.cross_one(loc)
        assert np.array_equal(bits(out), bits(img[d])) and np.array_equal(bits(out), bits(want[d])), d
    if name == "hidden6":
        assert not np.array_equal(bits(want[0][..., 2:]), bits(want[5][..., 2:]))       # the deals' scopas differ: a stale leaf table would show


@pytest.mark.parametrize("name", SETS)
def test_diagonal_and_best_response_entries_are_those_of_exploitability(world, name):
    game, t = world.game(name), X.tables(name)
    out4, br0, br1 = game.best_response(np.array(t["cfr"]))
    ex4, br = game.exploitability(np.array(t["cfr"]), return_br=True)
    assert np.array_equal(bits(out4), bits(ex4)) and np.array_equal(bits(br0), bits(br[0])) and np.array_equal(bits(br1), bits(br[1]))
    assert np.array_equal(bits(br0), bits(t["br0"]))
    out, _ = world.cross(game, world.put([t["cfr"], br0]))
    assert out[0, 0, 0].tobytes() == np.float64(out4[3]).tobytes()
    assert out[1, 0, 0].tobytes() == np.float64(out4[1]).tobytes()
    assert out[0, 1, 0].tobytes() == out[0, 0, 0].tobytes()      # br0 holds the policy's rows for team 1: [cfr][br0] is the policy against itself


def test_a_nan_reaches_exactly_the_pairs_that_play_its_table_for_its_team(world):
    cr, game, t = TS.chance_ref("hidden6"), world.game("hidden6"), X.tables("hidden6")
    clean = [t["cfr"], t["br0"], t["adv"]]
    want, _ = world.cross(game, world.put(clean))
    rows8 = cr.map[3, X.OFFSET[8]:X.OFFSET[8] + X.WIDTH[8]]
    team0_row = int(rows8[np.nonzero(np.diff(cr.occ_off)[rows8] == 2)[0][0]])      # a depth-8 row (team 0) that deal 3 shares with one other deal
    team1_row = int(cr.map[5, X.OFFSET[10] + 4242])     # a depth-10 row (team 1, 2 legal slots) of deal 5
    assert cr.team[team0_row] == 0 and cr.team[team1_row] == 1 and cr.nleg[team1_row] == 2
    tabs = [a.copy() for a in clean]
    tabs[0][team1_row, 3] = np.nan                      # padding: never read
    tabs[1][team0_row, 1] = np.nan                      # table 1 poisons team 0's play: row [1][*]
    tabs[2][team1_row, 1] = np.nan                      # table 2 poisons team 1's play: column [*][2]
    out, img = world.cross(game, world.put(tabs))
    nan = np.isnan(out).all(axis=2)
    assert np.array_equal(nan, np.array([[False, False, True], [True, True, True], [False, False, True]]))
    assert np.array_equal(bits(out[~nan]), bits(want[~nan]))
    holds = np.zeros(game.n, bool)                      # per deal, only the deals in which the poisoned team-0 row occurs
    holds[cr.occ[cr.occ_off[team0_row]:cr.occ_off[team0_row + 1]] // X.N_CHOICE] = True
    assert holds[3] and not holds.all()
    assert np.array_equal(np.isnan(img[:, 1, 0]).all(axis=1), holds) and np.array_equal(np.isnan(img[:, 1, 0]).any(axis=1), holds)


# ---- the match --------------------------------------------------------------------------------------------------------------------------------
def run_match(world, game, a, b, n, n_team0, stream):
    torch = world.torch
    deal = torch.full((max(n, 1),), -1, dtype=torch.int32, device=world.dev)
    leaf = torch.full((max(n, 1),), -1, dtype=torch.int32, device=world.dev)
    pa, pb = world.put(a), world.put(b)
    torch.cuda.synchronize()
    st = game.match(pa.data_ptr(), pb.data_ptr(), n, n_team0, stream, deal.data_ptr(), leaf.data_ptr())
    return deal.cpu().numpy()[:n], leaf.cpu().numpy()[:n], st


@pytest.mark.parametrize("seed,stream", X.MATCH_CASES, ids=W.case_id)
def test_chance_match_is_the_restatement_episode_by_episode(world, seed, stream):
    game, t = world.game("hidden6"), X.tables("hidden6")
    world.ctx.mccfr_seed(seed)
    want = X.xref("hidden6").match(t["adv"], t["cfr"], X.MATCH_N, X.MATCH_TEAM0, seed, stream)
    deal, leaf, st = run_match(world, game, t["adv"], t["cfr"], X.MATCH_N, X.MATCH_TEAM0, stream)
    print("episodes that differ (deal, leaf):", int((deal != want.deal).sum()), int((leaf != want.leaf).sum()))
    assert np.array_equal(deal, want.deal) and np.array_equal(leaf, want.leaf) and np.array_equal(st, want.stats)
    pa, pb = world.put(t["adv"]), world.put(t["cfr"])
    world.torch.cuda.synchronize()
    st2 = game.match(pa.data_ptr(), pb.data_ptr(), X.MATCH_N, X.MATCH_TEAM0, stream)     # no per-episode outputs
    assert np.array_equal(st2, st)


def test_an_episode_that_drew_deal_d_ends_where_the_one_deal_match_ends(world):
    cr, game, t, ctx, torch = TS.chance_ref("reordered"), world.game("reordered"), X.tables("reordered"), world.ctx, world.torch
    ctx.mccfr_seed(W.WIDE_SEED)
    deal, leaf, st = run_match(world, game, t["adv"], t["uniform"], X.MATCH_N, X.MATCH_TEAM0, 16)
    total = np.zeros((2, 5), np.int64)
    for d in range(2):
        ctx.team_set_deal(TS.deal_set("reordered")[d])
        pa, pb = world.put(cr.policy_for_deal(t["adv"], d)), world.put(cr.policy_for_deal(t["uniform"], d))
        out = torch.full((X.MATCH_N,), -1, dtype=torch.int32, device=world.dev)
        torch.cuda.synchronize()
        st1 = ctx.team_match(pa.data_ptr(), pb.data_ptr(), X.MATCH_N, X.MATCH_TEAM0, 16, out.data_ptr())
        one = out.cpu().numpy()
        sel = deal == d
        assert sel.sum() > 1000 and np.array_equal(one[sel], leaf[sel])
        want = X.XRef.one(TS.deal_set("reordered")[d]).match(cr.policy_for_deal(t["adv"], d), cr.policy_for_deal(t["uniform"], d), X.MATCH_N, X.MATCH_TEAM0, W.WIDE_SEED, 16)
        assert np.array_equal(one, want.leaf) and np.array_equal(st1, want.stats)
        assert st1[:, 0].tolist() == [X.MATCH_TEAM0, X.MATCH_N - X.MATCH_TEAM0]


def test_no_episodes_give_zeros(world):
    game, t, ctx = world.game("reordered"), X.tables("reordered"), world.ctx
    _, _, st = run_match(world, game, t["adv"], t["cfr"], 0, 0, 16)
    assert st.shape == (2, 5) and not st.any()
    ctx.team_set_deal(BASE)
    p = world.put(TS.chance_ref("reordered").policy_for_deal(t["cfr"], 0))
    assert not ctx.team_match(p.data_ptr(), p.data_ptr(), 0, 0, 16).any()


@pytest.mark.parametrize("name", SETS)
def test_long_match_means_within_five_standard_errors_of_the_device_cross_play(world, name):
    """the pair is (the rows a match plays from adv, cfr): normalised tables, on which the exact cross-play is the match's law (test_team_xplay_ref.py
    holds the restatement to the same check); the standard error comes from the second moment the device's cross-play reports"""
    game, t = world.game(name), X.tables(name)
    played = X.normalised(TS.chance_ref(name), t["adv"])
    exact, _ = world.cross(game, world.put([played, t["cfr"]]))
    world.ctx.mccfr_seed(X.LONG_SEED)
    n, first = X.LONG_N, X.LONG_N // 2
    _, _, st = run_match(world, game, played, t["cfr"], n, first, X.LONG_STREAM)
    for mean, target, se in X.standard_error_check(st, exact, first, n):
        print(name, "mean", mean, "target", target, "standard error", se)
        assert se > 0 and abs(mean - target) <= 5 * se


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(world, sl):
    """every refusal is followed by a cross-play that must give the bits of the one before it"""
    L, ctx, torch = sl.lib(), world.ctx, world.torch
    game = world.game("reordered")
    stack = world.put(X.stack("reordered"))
    before, _ = world.cross(game, stack)
    out = torch.zeros((3, 3, 4), dtype=torch.float64, device=world.dev)
    spare = torch.zeros((game.G + 1, 4), dtype=torch.float64, device=world.dev)
    vp, st = C.c_void_p, (C.c_int64 * 10)(*([5] * 10))
    g, h, P, O, odd = game._h, ctx._h, vp(stack.data_ptr()), vp(out.data_ptr()), vp(spare.data_ptr() + 8)
    torch.cuda.synchronize()

    def refused(same, status, call, *args):
        rc = call(*args)
        assert rc == status, (call.__name__, args[1:], rc, status)
        assert list(st) == [5] * 10, (call.__name__, args[1:])            # a refused match does not touch the sums
        if same is not None:
            assert same(), (call.__name__, args[1:])

    same = lambda: np.array_equal(bits(world.cross(game, stack)[0]), bits(before))
    for n_pol in (0, -1, 257):
        refused(same, sl.SCOPA_EINVAL, L.scopa_team_chance_cross_play, g, n_pol, P, None, O)
    refused(same, sl.SCOPA_EINVAL, L.scopa_team_chance_cross_play, g, 3, None, None, O)
    refused(same, sl.SCOPA_EINVAL, L.scopa_team_chance_cross_play, g, 3, P, None, None)
    refused(same, sl.SCOPA_EINVAL, L.scopa_team_chance_cross_play, g, 1, odd, None, O)
    refused(same, sl.SCOPA_EINVAL, L.scopa_team_chance_cross_play, None, 3, P, None, O)
    # SCOPA_ELIMIT: the limit of 2^31 workgroups needs 128 deals at n_pol = 256, so the test hook lowers it to this call's own count -- 256 * n * K * K
    # reaches it, one more does not (the checking cross-play runs once the limit is back)
    ctx.team_debug_xplay_group_limit(256 * game.n * 9)
    refused(None, sl.SCOPA_ELIMIT, L.scopa_team_chance_cross_play, g, 3, P, None, O)
    ctx.team_debug_xplay_group_limit(256 * game.n * 9 + 1)
    refused(None, sl.SCOPA_OK, L.scopa_team_chance_cross_play, g, 3, P, None, O)
    ctx.team_debug_xplay_group_limit(0)
    ctx.synchronize()
    assert same() and np.array_equal(bits(out.cpu().numpy()), bits(before))
    for n, n0 in ((-1, 0), (5, 6), (5, -1)):
        refused(same, sl.SCOPA_EINVAL, L.scopa_team_chance_match, g, P, P, n, n0, 16, None, None, st)
    refused(same, sl.SCOPA_EINVAL, L.scopa_team_chance_match, g, None, P, 5, 2, 16, None, None, st)
    refused(same, sl.SCOPA_EINVAL, L.scopa_team_chance_match, g, P, None, 5, 2, 16, None, None, st)
    refused(same, sl.SCOPA_EINVAL, L.scopa_team_chance_match, g, P, P, 5, 2, 16, None, None, None)
    refused(same, sl.SCOPA_EINVAL, L.scopa_team_chance_match, g, P, odd, 5, 2, 16, None, None, st)

    # one deal: no team deal yet on a fresh context is SCOPA_ESTATE; then the same argument checks
    fresh = sl.Context(0)
    try:
        refused(same, sl.SCOPA_ESTATE, L.scopa_team_cross_play, fresh._h, 1, P, O)
        refused(same, sl.SCOPA_ESTATE, L.scopa_team_match, fresh._h, P, P, 5, 2, 16, None, st)
    finally:
        fresh.close()
    ctx.team_set_deal(BASE)
    loc = world.put([TS.chance_ref("reordered").policy_for_deal(p, 0) for p in X.stack("reordered")])
    Q = vp(loc.data_ptr())
    first = world.cross_one(loc)
    same = lambda: np.array_equal(bits(world.cross_one(loc)), bits(first))
    for n_pol in (0, 257):
        refused(same, sl.SCOPA_EINVAL, L.scopa_team_cross_play, h, n_pol, Q, O)
    refused(same, sl.SCOPA_EINVAL, L.scopa_team_cross_play, h, 3, None, O)
    refused(same, sl.SCOPA_EINVAL, L.scopa_team_cross_play, h, 3, Q, None)
    refused(same, sl.SCOPA_EINVAL, L.scopa_team_cross_play, h, 1, vp(loc.data_ptr() + 8), O)
    ctx.team_debug_xplay_group_limit(256 * 9)
    refused(None, sl.SCOPA_ELIMIT, L.scopa_team_cross_play, h, 3, Q, O)
    ctx.team_debug_xplay_group_limit(0)
    assert same()
    for n, n0 in ((-1, 0), (5, 6), (5, -1)):
        refused(same, sl.SCOPA_EINVAL, L.scopa_team_match, h, Q, Q, n, n0, 16, None, st)
    refused(same, sl.SCOPA_EINVAL, L.scopa_team_match, h, Q, vp(loc.data_ptr() + 8), 5, 2, 16, None, st)


# ---- shapes past 2^24 workgroups ----------------------------------------------------------------------------------------------------------------------
def test_shapes_past_two_to_the_24_workgroups_launch(world):
    """256 lanes x 2^24 workgroups is 2^32 work-items, which no single grid dimension may reach: the documented maximum n_pol = 256 on one deal (exactly
    2^24 workgroups) and K = 182 on the two deals of `reordered` (2 * 256 * 182^2 > 2^24) must launch all the same, below the 2^31 limit.  The tables are
    the three of the stack repeated, table k = stack[k % 3], so entry [a][b] must be the K = 3 entry [a % 3][b % 3] bit for bit."""
    cr, ctx, torch = TS.chance_ref("reordered"), world.ctx, world.torch
    ctx.team_set_deal(BASE)
    loc = world.put([cr.policy_for_deal(p, 0) for p in X.stack("reordered")])
    small = world.cross_one(loc)
    k = 256
    big = loc[torch.arange(k, device=world.dev) % 3].contiguous()
    out = world.cross_one(big)
    idx = np.arange(k) % 3
    assert np.array_equal(bits(out), bits(small[idx][:, idx]))
    del big
    game, k = world.game("reordered"), 182
    assert 256 * game.n * k * k > 1 << 24
    stack = world.put(X.stack("reordered"))
    want, want_img = world.cross(game, stack)
    big = stack[torch.arange(k, device=world.dev) % 3].contiguous()
    out, img = world.cross(game, big)
    idx = np.arange(k) % 3
    assert np.array_equal(bits(out), bits(want[idx][:, idx])) and np.array_equal(bits(img), bits(want_img[:, idx][:, :, idx]))


# ---- the Python surface ----------------------------------------------------------------------------------------------------------------------------
def test_python_surface_returns_what_the_raw_calls_return(world):
    from scopa_amd.algorithms import team_chance as A
    game, t, ctx = world.game("reordered"), X.tables("reordered"), world.ctx
    raw, _ = world.cross(game, world.put(X.stack("reordered")))
    got = A.cross_play(game, X.stack("reordered"))
    assert got.shape == (3, 3, 4) and np.array_equal(bits(got), bits(raw))
    assert np.array_equal(bits(A.cross_play(game, world.put(X.stack("reordered")))), bits(raw))       # a device stack is taken as it is
    played = X.normalised(TS.chance_ref("reordered"), t["adv"])
    rep = A.evaluate(game, played, t["cfr"], episodes=4099, seed=W.WIDE_SEED, stream_id=W.ITER_B31)
    _, _, st = run_match(world, game, played, t["cfr"], 4099, 2050, W.ITER_B31)                    # the seed evaluate set is still the context's
    exact, _ = world.cross(game, world.put([played, t["cfr"]]))
    assert np.array_equal(rep["sums"], st) and rep["episodes"] == 4099
    assert rep["exact_by_team"] == (float(exact[0, 1, 0]), float(-exact[1, 0, 0]))
    assert rep["reward"] == 0.5 * int(st[:, 1].sum()) / 4099
    assert rep["exact_reward"] == (2050 * rep["exact_by_team"][0] + 2049 * rep["exact_by_team"][1]) / 4099
    for half, (mean, target, se) in enumerate(X.standard_error_check(st, exact, 2050, 4099)):
        h = rep["by_team"][half]
        assert (h["reward"], h["exact_reward"]) == (mean, target) and abs(h["exact_std_error"] - se) <= 1e-15 * se
    assert 0 < rep["exact_std_error"] < max(h["exact_std_error"] for h in rep["by_team"])
    with pytest.raises(ValueError):
        A.cross_play(game, np.zeros((2, game.G - 1, 4)))


def test_trainer_pair_on_one_deal(world, sl):
    from scopa_amd.algorithms import TeamCFRTrainer
    from scopa_amd.envs.openspiel_team_mini_scopa import TPIMiniScopaGame
    tr = TeamCFRTrainer(TPIMiniScopaGame(seed=42))
    try:
        tr.train(2)
        _, S, _, _ = tr.ctx.team_tables_get()
        import team_chance_ref as TC
        xr = X.XRef.one(tr._perm)
        avg = TC.ref_of(tr._perm).average_policy(S)
        uni = np.zeros((X.N_CHOICE, 4))
        for d in range(12):
            uni[X.OFFSET[d]:X.OFFSET[d] + X.WIDTH[d], :X.branch(d)] = 1.0 / X.branch(d)
        got = tr.cross_play([avg, uni])
        assert np.array_equal(bits(got), bits(xr.cross_play([avg, uni])[0]))
        rep = tr.evaluate(avg, uni, episodes=4099, seed=0x5C09A, stream_id=3)
        want = xr.match(avg, uni, 4099, 2050, 0x5C09A, 3)
        assert np.array_equal(rep["sums"], want.stats) and rep["exact_by_team"] == (float(got[0, 1, 0]), float(-got[1, 0, 0]))
    finally:
        tr.ctx.close()
