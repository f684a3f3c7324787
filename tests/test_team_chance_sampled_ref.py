"""CPU checks that pin the restatement of the deal-sampled and simultaneous iterations of Team MiniScopa over a set of deals
(tests/team_chance_sampled_ref.py) to tests/team_chance_ref.py's ChanceRef, and of the host-side argument handling of
algorithms.team_chance.solve and TeamChanceGame.cfr_iterate_sampled that is reachable without a device."""
import types

import numpy as np
import pytest

import team_chance_sampled_ref as SR
import team_chance_sets as TS

W = np.array([[0.5, 0.25, 0.75], [1.0, 0.0, 0.5]])


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def run(sr, deals, weights=None, alternating=True, tables=None):
    R, S, sig = sr.cr.tables() if tables is None else tables
    rv = sr.iterate(R, S, sig, deals, weights, alternating)
    return R, S, sig, rv


def same(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def refs(oracle):
    return {name: SR.SampledRef(TS.chance_ref(name)) for name in ("reordered", "both4")}


def test_a_full_list_is_the_exact_iteration(refs):
    sr = refs["reordered"]
    cr = sr.cr
    for weights in (None, W):
        R, S, sig = cr.tables()
        rv = cr.iterate(R, S, sig, 2, weights) if weights is None else cr.iterate(R, S, sig, weights=weights)
        for deals in ([[0, 1], [0, 1]], [[1, 0], [0, 1]], [None, None]):
            assert same(run(sr, deals, weights), (R, S, sig, rv)), deals


def test_list_order_changes_nothing(refs):
    sr = refs["both4"]
    a = run(sr, [[1, 3], [2, 0]], W)
    b = run(sr, [[3, 1], [0, 2]], W)
    assert same(a, b)
    c = run(sr, [[1, 3], [0, 2]], W, alternating=False)
    d = run(sr, [[3, 1], [2, 0]], W, alternating=False)
    assert same(c, d) and not np.array_equal(bits(a[0]), bits(c[0]))


def test_sum_starts_at_the_first_listed_occurrence(refs):
    """both4, list [1, 3]: a row shared by deals 0 and 1 takes deal 1's increments as they are, not 0.0 + them; one shared by deals 1 and 3 takes
    deal 1's value + deal 3's; a row of deals 0 and 2 alone takes +0.0 and is discounted"""
    sr = refs["both4"]
    cr = sr.cr
    rng = np.random.default_rng(5)
    legal = np.arange(4)[None, :] < cr.nleg[:, None]
    R0, S0 = np.where(legal, rng.standard_normal((cr.G, 4)), 0.0), np.where(legal, rng.random((cr.G, 4)), 0.0)
    sig0 = cr.sigma(R0)
    img, roots = cr.sweep(sig0, 0)                                                 # all four deals
    img = img.reshape(cr.n, -1, 8)
    R, S, sig = R0.copy(), S0.copy(), sig0.copy()
    w = (0.5, 0.25, 0.75)
    rv = sr.iterate(R, S, sig, [[3, 1]], [w], alternating=True)
    assert rv[0, 0] == (roots[1] + roots[3]) / 2.0
    cnt = np.zeros(cr.G, np.int64)
    want = np.zeros((cr.G, 8))
    for deal in (1, 3):                                                             # ascending; the first listed value is copied
        g = cr.map[deal]
        first = cnt[g] == 0
        want[g[first]] = img[deal][first]
        want[g[~first]] = want[g[~first]] + img[deal][~first]
        cnt[g] += 1
    t0 = cr.team == 0
    assert {0, 1, 2} <= set(np.unique(cnt[t0]).tolist())
    Rn = R0 + want[:, :4]
    Rn = np.where(~(Rn <= 0.0), Rn * w[0], Rn * w[1])
    Sn = (S0 + want[:, 4:]) * w[2]
    assert np.array_equal(bits(R[t0]), bits(np.where(legal, Rn, 0.0)[t0])) and np.array_equal(bits(S[t0]), bits(np.where(legal, Sn, 0.0)[t0]))
    unlisted = t0 & (cnt == 0)
    assert np.array_equal(bits(R[unlisted]), bits(np.where(~(R0 <= 0.0), R0 * w[0], R0 * w[1])[unlisted])) and unlisted.sum() > 1000


def test_an_unlisted_regret_of_minus_zero_becomes_plus_zero(refs):
    """reordered, list [0]: seat 0's rows of deal 1 have no listed occurrence; -0.0 + +0.0 is +0.0, with and without weights"""
    sr = refs["reordered"]
    cr = sr.cr
    listed = np.zeros(cr.G, bool)
    listed[cr.map[0]] = True
    target = ~listed & (cr.team == 0)
    assert target.sum() == 1 + 256 + 20736
    for w in (None, [(1.0, 0.5, 1.0)]):
        R = np.full((cr.G, 4), -0.0)
        S = np.full((cr.G, 4), -0.0)
        sig = cr.sigma(R)
        assert np.signbit(R).all()
        sr.iterate(R, S, sig, [[0]], w)
        legal = np.arange(4)[None, :] < cr.nleg[:, None]
        assert not np.signbit(R[target][legal[target]]).any() and not np.signbit(S[target][legal[target]]).any()
        assert np.all(R[target] == 0.0) and np.all(S[target] == 0.0)
        assert np.array_equal(bits(sig[target]), bits(cr.sigma(np.zeros((cr.G, 4)))[target]))


def test_simultaneous_sweeps_read_one_sigma(refs):
    """alternating=0 on a full list: team 0's rows are the exact iteration's, team 1's are those of a sweep against the sigma of the start"""
    sr = refs["reordered"]
    cr = sr.cr
    R, S, sig = cr.tables()
    cr.iterate(R, S, sig, 1)                                                       # a non-uniform start
    start = (R.copy(), S.copy(), sig.copy())
    a = run(sr, [None], None, alternating=False, tables=tuple(x.copy() for x in start))
    b = run(sr, [None], None, alternating=True, tables=tuple(x.copy() for x in start))
    t0 = cr.team == 0
    assert same([x[t0] for x in a[:3]], [x[t0] for x in b[:3]]) and a[3][0, 0] == b[3][0, 0]
    assert not np.array_equal(bits(a[0][~t0]), bits(b[0][~t0]))
    R1, S1, sig1 = (x.copy() for x in start)
    v1 = cr.traverse(R1, S1, sig1, 1)                                              # traverser 1 alone against the start
    assert same([x[~t0] for x in a[:3]], [x[~t0] for x in (R1, S1, sig1)]) and a[3][0, 1] == v1 == -a[3][0, 0]


# ---- argument handling that needs no device ------------------------------------------------------------------------------------------------------
def test_solve_refuses_a_bad_sample_before_it_opens_a_device():
    from scopa_amd.algorithms import team_chance
    perms = TS.deal_set("reordered")
    for sample in (0, -1):
        with pytest.raises(ValueError):
            team_chance.solve(perms, "dcfr", sample=sample, device="no such device")


def test_solve_keeps_its_defaults():
    import inspect
    from scopa_amd.algorithms import team_chance
    p = inspect.signature(team_chance.solve).parameters
    assert (p["alternating"].default, p["sample"].default, p["seed"].default) == (True, None, 0)
    assert list(p)[:6] == ["perms", "variant", "eps", "max_iters", "check_every", "device"] and p["eps"].default == 1e-3


def test_cfr_iterate_sampled_checks_shapes_before_the_call(sl):
    """the ValueErrors are raised before the handle is touched: a stand-in object serves"""
    f = sl.TeamChanceGame.cfr_iterate_sampled
    nobody = types.SimpleNamespace()
    for deals, weights in (([0, 1, 2], None), (np.zeros((2, 2, 2), np.int32), None), ([[0, 1], [1, 0]], np.ones((3, 3))), ([[0, 1]], np.ones((2, 3))), (None, None)):
        with pytest.raises(ValueError):
            f(nobody, deals, weights)
    p = __import__("inspect").signature(f).parameters
    assert (p["weights"].default, p["alternating"].default, p["root_values"].default) == (None, True, False)
