"""GPU checks of Team MiniScopa over a set of deals (scopa_team_chance.hip) against the one-deal solver (scopa_team_cfr.hip) and against the float64
restatement tests/team_chance_ref.py, which tests/test_team_chance_ref.py pins to team_cfr_ref.Ref.  Comparisons are exact unless a test says
otherwise: every row has one writer and every float64 sum a fixed order.  References are computed once per module and handed out read-only.
The sets here share rows at depths 0 and 1 (`swap`, `six`), at every depth with equal values in both occurrences (`copies`) or nowhere (`one`,
`disjoint`); distinct deals that share rows at depths 2..11 are tests/test_gpu_team_chance_shared.py's (both4, reordered, hidden6)."""
import numpy as np
import pytest

import cfr_edges as E
import team_chance_ref as TC

pytestmark = pytest.mark.gpu

PACKETS = [[0, 5, 10, 15], [1, 4, 11, 14], [2, 7, 8, 13], [3, 6, 9, 12]]
_CACHE = {}


def deal_set(name):
    from scopa_amd.algorithms.team_chance import packet_deals
    six, all24 = packet_deals(PACKETS, fix_seat0=True), packet_deals(PACKETS)
    if name == "one":
        return six[:1]
    if name == "copies":
        return six[[0, 0]]
    if name == "swap":          # seats 2 and 3 swap their hands: the rows of depths 0 and 1 are shared
        return six[:2]
    if name == "disjoint":      # the cyclic shifts of the packets: pairwise disjoint seat-0 hands, no shared row
        return np.array([d for d in all24 if [int(d[4 * s]) for s in range(4)] in ([0, 1, 2, 3], [1, 2, 3, 0], [2, 3, 0, 1], [3, 0, 1, 2])])
    assert name == "six"
    return six


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def ref_of(name):
    return cached(("ref", name), lambda: TC.ChanceRef(deal_set(name)))


def ref_run(name, variant, n_iters=3):
    """(R, S, sigma, root values) of the restatement after n_iters iterations of `variant` from reset, read-only"""
    def make():
        from scopa_amd.algorithms import schedule
        cr = ref_of(name)
        R, S, sig = cr.tables()
        rv = cr.iterate(R, S, sig, weights=schedule(variant, 0, n_iters))
        for a in (R, S, sig, rv):
            a.setflags(write=False)
        return R, S, sig, rv
    return cached(("run", name, variant, n_iters), make)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def random_policy(cr, seed):
    rng = np.random.default_rng(seed)
    pol = np.where(np.arange(4)[None, :] < cr.nleg[:, None], rng.random((cr.G, 4)) + 0.05, 0.0)
    return pol / pol.sum(1, keepdims=True)


def uniform_policy(cr):
    return np.where(np.arange(4)[None, :] < cr.nleg[:, None], 1.0 / cr.nleg[:, None], 0.0)


@pytest.fixture()
def game_of(sl, ctx):
    games = []

    def make(name):
        games.append(sl.TeamChanceGame(deal_set(name), ctx))
        return games[-1]
    yield make
    for g in games:
        g.close()


# ---- iterations ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [None, "dcfr"])
def test_one_deal_gives_the_one_deal_solvers_bits(ctx, game_of, variant):
    from scopa_amd.algorithms import schedule
    game = game_of("one")
    keys, mp = game.index()
    assert (game.n, game.G, game.n_occurrences) == (1, 321365, 321365) and np.array_equal(mp[0], np.argsort(np.argsort(keys[mp[0]])))
    w = None if variant is None else schedule(variant, 0, 3)
    rv = game.cfr_iterate(3 if w is None else w, root_values=True)
    R, S = game.tables_get()
    ctx.team_set_deal(deal_set("one")[0])
    rv1 = ctx.team_cfr_iterate(3, w)
    R1, S1, L1, _ = ctx.team_tables_get()
    assert np.array_equal(bits(rv), bits(rv1))
    assert np.array_equal(bits(R[mp[0]]), bits(R1)) and np.array_equal(bits(S[mp[0]]), bits(S1)) and np.array_equal(bits(game.sigma_get()[mp[0]]), bits(L1))


def test_two_copies_of_a_deal_double_the_tables(ctx, game_of):
    from scopa_amd.algorithms import schedule
    game = game_of("copies")
    assert game.G == 321365 and game.n_occurrences == 2 * 321365
    _, mp = game.index()
    assert np.array_equal(mp[0], mp[1])
    w = schedule("dcfr", 0, 3)
    rv = game.cfr_iterate(w, root_values=True)
    R, S = game.tables_get()
    ctx.team_set_deal(deal_set("one")[0])
    rv1 = ctx.team_cfr_iterate(3, w)
    R1, S1, L1, _ = ctx.team_tables_get()
    # x + x = 2 x exactly, the weights multiply 2 x as they multiply x, and regret matching is scale-free
    assert np.array_equal(rv, rv1) and np.array_equal(R[mp[0]], 2.0 * R1) and np.array_equal(S[mp[0]], 2.0 * S1) and np.array_equal(game.sigma_get()[mp[0]], L1)


@pytest.mark.parametrize("variant", ["vanilla", "cfr+", "dcfr"])
@pytest.mark.parametrize("name", ["swap", "disjoint", "six"])
def test_iterations_against_the_restatement(game_of, name, variant):
    from scopa_amd.algorithms import schedule
    cr = ref_of(name)
    R_want, S_want, sig_want, rv_want = ref_run(name, variant)
    game = game_of(name)
    keys, mp = game.index()
    assert game.G == cr.G and np.array_equal(keys, cr.gkey) and np.array_equal(mp, cr.map)
    rv = game.cfr_iterate(schedule(variant, 0, 3), root_values=True)
    R, S = game.tables_get()
    sig = game.sigma_get()
    print(name, variant, "cells that differ:", [int(np.count_nonzero(bits(a) != bits(b))) for a, b in ((R, R_want), (S, S_want), (sig, sig_want), (rv, rv_want))])
    assert np.array_equal(bits(rv), bits(rv_want))
    assert np.array_equal(bits(R), bits(R_want)) and np.array_equal(bits(S), bits(S_want)) and np.array_equal(bits(sig), bits(sig_want))
    if name == "six" and variant == "dcfr":   # a second run from reset gives the same bits
        game.tables_reset()
        rv2 = game.cfr_iterate(schedule(variant, 0, 3), root_values=True)
        R2, S2 = game.tables_get()
        assert np.array_equal(bits(rv2), bits(rv)) and np.array_equal(bits(R2), bits(R)) and np.array_equal(bits(S2), bits(S)) and np.array_equal(bits(game.sigma_get()), bits(sig))


def edge_tables(case, cr):
    """regret and strategy tables over the global rows: oracle/cfr_edges.py's cases, and `neginf` = its `inf` case with -inf in slot 1 of every 5th row"""
    R, S, _ = E.tables("inf" if case == "neginf" else case, cr.nleg)
    if case == "neginf":
        R[::5, 1] = -np.inf
    return R, S


@pytest.mark.parametrize("case,w", [("allneg", (1.0, 0.0, 1.0)), ("onehot", (0.0, 1.0, 0.0)), ("nan", (1.0, 1.0, 1.0)), ("inf", (0.5, 0.0, 1.0)), ("neginf", (1.0, 0.0, 0.0)),
                                    ("big", None)])
def test_edge_tables_one_iteration(game_of, case, w):
    cr, game = ref_of("swap"), game_of("swap")
    R0, S0 = edge_tables(case, cr)
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


# ---- exploitability ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["swap", "six"])
def test_exploitability_against_the_restatement(ctx, game_of, name):
    from scopa_amd.algorithms import schedule
    cr, game = ref_of(name), game_of(name)
    _, S_want, _, _ = ref_run(name, "cfr+")
    game.cfr_iterate(schedule("cfr+", 0, 3))
    perms = deal_set(name)
    for what, pol in (("average", None), ("caller", random_policy(cr, 3)), ("uniform", uniform_policy(cr))):
        want4, brs, per_deal = cached(("expl", name, what), lambda: cr.exploitability(cr.average_policy(S_want) if pol is None else pol))
        out4, evaluated, br = game.exploitability(pol, return_policy=True, return_br=True)
        print(name, what, out4, want4)
        assert np.array_equal(bits(evaluated), bits(cr.average_policy(S_want) if pol is None else pol))
        assert np.array_equal(bits(out4), bits(want4))
        assert np.array_equal(bits(br[0]), bits(brs[0])) and np.array_equal(bits(br[1]), bits(brs[1]))
        assert np.array_equal(bits(game.exploitability(pol)), bits(out4))          # without the optional outputs
        if what != "caller" and name == "six":
            continue
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


def test_one_deal_best_responses_agree_with_the_one_deal_solver(ctx, game_of):
    import torch
    game = game_of("one")
    cr = ref_of("one")
    _, mp = game.index()
    game.cfr_iterate(3)
    for pol in (None, random_policy(cr, 9)):
        out4, evaluated = game.exploitability(pol, return_policy=True)
        ctx.team_set_deal(deal_set("one")[0])
        local = torch.from_numpy(np.ascontiguousarray(evaluated[mp[0]])).cuda()
        want = ctx.team_exploitability(local.data_ptr())
        assert out4[3] == want[3]
        np.testing.assert_allclose(out4[:3], want[:3], rtol=0, atol=1e-12)   # opp * u may round a near-tie differently from the per-node maximum


def test_cfr_plus_lowers_the_exploitability_of_the_six_deal_game(ctx):
    from scopa_amd.algorithms import team_chance
    game, iters, curve = team_chance.solve(deal_set("six"), "cfr+", eps=0.0, max_iters=40, check_every=10, device=ctx)
    print(curve)
    assert iters == 40 and [t for t, _ in curve] == [10, 20, 30, 40]
    assert curve[-1][1] < curve[0][1] and curve[-1][1] >= 0.0
    by_key = team_chance.policy_by_key(game)
    assert len(by_key) == game.G and all(abs(r.sum() - 1.0) < 1e-12 for r in list(by_key.values())[:100])
    game.close()


# ---- contracts -------------------------------------------------------------------------------------------------------------------------------
def test_contracts(sl, ctx, game_of):
    import ctypes as C
    import torch
    L = sl.lib()
    perms = deal_set("swap")
    h = C.c_void_p()
    assert L.scopa_team_chance_create(ctx._h, 0, perms.ctypes.data_as(C.c_void_p), C.byref(h)) == sl.SCOPA_EINVAL and not h.value
    bad = perms.copy()
    bad[1, 3] = bad[1, 2]
    with pytest.raises(sl.ScopaError) as e:
        sl.TeamChanceGame(bad, ctx)
    assert e.value.status == sl.SCOPA_EINVAL
    assert L.scopa_team_chance_create(ctx._h, 6683, None, C.byref(h)) == sl.SCOPA_EINVAL     # no deals given
    big = np.tile(perms[:1], (6683, 1))                                                           # 6 683 * 321 365 >= 2^31
    assert L.scopa_team_chance_create(ctx._h, 6683, big.ctypes.data_as(C.c_void_p), C.byref(h)) == sl.SCOPA_ELIMIT and not h.value
    ctx.team_chance_debug_image_budget(2 * 321365 * 64 - 1)
    with pytest.raises(sl.ScopaError) as e:
        sl.TeamChanceGame(perms, ctx)
    assert e.value.status == sl.SCOPA_ELIMIT
    ctx.team_chance_debug_image_budget(2 * 321365 * 64)
    sl.TeamChanceGame(perms, ctx).close()
    ctx.team_chance_debug_image_budget(0)

    game = game_of("swap")
    for badw in (1.5, -0.25, float("nan"), float("inf")):
        with pytest.raises(sl.ScopaError) as e:
            game.cfr_iterate([[1.0, 1.0, 1.0], [1.0, badw, 1.0]])
        assert e.value.status == sl.SCOPA_EINVAL
    assert L.scopa_team_chance_cfr_iterate(game._h, -1, None, None) == sl.SCOPA_EINVAL
    assert L.scopa_team_chance_cfr_iterate(game._h, (1 << 20) + 1, None, None) == sl.SCOPA_EINVAL
    R0, S0 = game.tables_get()
    assert not R0.any() and not S0.any()                                                        # nothing was launched by the refused calls
    assert game.cfr_iterate(0, root_values=True).shape == (0, 2)
    assert not game.tables_get()[0].any()
    buf = torch.zeros(game.G * 4 + 4, dtype=torch.float64, device="cuda")
    out = (C.c_double * 4)()
    off = buf.data_ptr() + 8                                                                     # 8-byte aligned only
    assert buf.data_ptr() % 32 == 0
    assert L.scopa_team_chance_exploitability(game._h, C.c_void_p(off), C.byref(out), None, None) == sl.SCOPA_EINVAL
    assert L.scopa_team_chance_exploitability(game._h, None, C.byref(out), C.c_void_p(off), None) == sl.SCOPA_EINVAL
    assert L.scopa_team_chance_policy_for_deal(game._h, C.c_void_p(buf.data_ptr()), 2, C.c_void_p(buf.data_ptr())) == sl.SCOPA_EINVAL
    # create, destroy, create again on one context
    game.cfr_iterate(2)
    first = game.tables_get()
    game.close()
    again = game_of("swap")
    again.cfr_iterate(2)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(again.tables_get(), first))
