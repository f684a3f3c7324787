"""The restatement of Team MiniScopa's cross-play and matches (tests/team_xplay_ref.py) anchored to what already exists -- ChanceRef's value pass and
best response, team_cfr_ref's policy_value, the oracle's TeamState -- and the guards that the expectations of tests/test_gpu_team_xplay.py separate:
a kernel that swapped the teams, read the padding, summed the deals in another order or lost part of a Philox word could not pass there."""
import os
import re

import numpy as np
import pytest

import philox_words as W
import team_chance_ref as TC
import team_chance_sets as TS
import team_xplay_ref as X

@pytest.fixture(autouse=True)
def _oracle_built(oracle):
    """the restatements ask the oracle's library for the rules"""


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = ("reordered", "hidden6")
BASE = TS.deal_set("reordered")[0]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_leaf_scopas_by_the_walk_equal_the_oracle_enumeration():
    """three depth-4 subtrees of the base deal and one of a hidden6 deal, leaf by leaf through the oracle's TeamState; r2 and the scopas are consistent:
    r2 = captured cards of team 0 - of team 1 + 2 x (scopas of team 0 - of team 1), the card difference within the deck's 16"""
    sc = X.leaf_scopas(BASE)
    assert sc.shape == (X.N_LEAVES,) and sc.dtype == np.uint8
    for g in (0, 100, 255):
        assert np.array_equal(X.leaf_scopas_enum(BASE, g * 1296, 1296), sc[g * 1296:(g + 1) * 1296]), g
    other = TS.deal_set("hidden6")[4]
    assert np.array_equal(X.leaf_scopas_enum(other, 77 * 1296, 1296), X.leaf_scopas(other)[77 * 1296:78 * 1296])
    r2 = TC.walk(BASE)[1].astype(np.int64)
    cards = r2 - 2 * ((sc & 15).astype(np.int64) - (sc >> 4).astype(np.int64))      # captured cards of team 0 - of team 1
    assert int(np.abs(cards).max()) <= 16 and (sc & 15).max() >= 2 and (sc >> 4).max() >= 2


@pytest.mark.parametrize("name", SETS)
def test_diagonal_is_the_value_pass_and_br0_against_the_policy_is_the_br0_value(name):
    cr, t = TS.chance_ref(name), X.tables(name)
    out, img = X.reference(name)
    assert np.array_equal(bits(img[:, 0, 0, 0]), bits(t["cfr_value_per_deal"]))
    for k, key in enumerate(X.STACK):
        if key != "cfr":
            assert np.array_equal(bits(img[:, k, k, 0]), bits(cr.value_pass(t[key], None)[0])), key
    assert out[0, 0, 0].tobytes() == np.float64(t["cfr_out4"][3]).tobytes()
    assert out[1, 0, 0].tobytes() == np.float64(t["cfr_out4"][1]).tobytes()        # [br0][cfr]: the BR0 value of ChanceRef.exploitability
    assert np.array_equal(bits(out), bits(X.deal_mean(img)))


def test_one_deal_is_policy_value():
    cr, ref, xr = TS.chance_ref("reordered"), TC.ref_of(BASE), X.XRef.one(BASE)
    loc = [cr.policy_for_deal(p, 0) for p in X.stack("reordered")]
    out, img = xr.cross_play(loc)
    assert np.array_equal(bits(out), bits(X.reference("reordered")[1][0]))        # the chance form's deal 0 is the one-deal form on the scattered tables
    for a in range(3):
        for b in range(3):
            assert out[a, b, 0].tobytes() == np.float64(ref.policy_value(loc[a], loc[b])).tobytes(), (a, b)


@pytest.mark.parametrize("name", SETS)
def test_expectations_separate(name):
    out, img = X.reference(name)
    for a in range(3):
        for b in range(a + 1, 3):
            assert not np.any(bits(out[a, b]) == bits(out[b, a])), (a, b)                   # who is team 0 matters, in all four quantities
    assert np.all(np.isfinite(out))
    xr = X.xref(name)
    wrong = xr.per_deal(X.stack(name)[1:], read_padding=True)                              # br0 (padding 0.0) and adv (padding garbage)
    assert np.array_equal(bits(wrong[:, 0, 0]), bits(img[:, 1, 1]))
    for cell in ((0, 1), (1, 0), (1, 1)):
        assert not np.any(bits(wrong[:, cell[0], cell[1]]) == bits(img[:, 1 + cell[0], 1 + cell[1]])), cell


def test_hidden6_mean_depends_on_the_deal_order():
    """team_chance_sets promises an order-sensitive a + b + c on hidden6; the cross-play mean inherits it"""
    out, img = X.reference("hidden6")
    other = X.deal_mean(img, order=[5, 4, 3, 2, 1, 0])
    assert not np.array_equal(bits(other), bits(out))
    np.testing.assert_allclose(other, out, rtol=1e-12)


@pytest.mark.parametrize("seed,stream", X.MATCH_CASES, ids=W.case_id)
def test_match_sums_follow_from_the_leaves_and_wide_words_separate(seed, stream):
    xr, t = X.xref("hidden6"), X.tables("hidden6")
    m = xr.match(t["adv"], t["cfr"], X.MATCH_N, X.MATCH_TEAM0, seed, stream)
    assert m.deal.min() == 0 and m.deal.max() == 5 and m.leaf.min() >= 0 and m.leaf.max() < X.N_LEAVES
    assert np.array_equal(m.stats, X.sums_of(xr.r2[m.deal, m.leaf], xr.sc[m.deal, m.leaf], X.MATCH_TEAM0))
    assert m.stats[0, 0] == X.MATCH_TEAM0 and m.stats[1, 0] == X.MATCH_N - X.MATCH_TEAM0
    variants = W.narrowed(seed, stream, 0, 1)              # the stream id in the place of the iteration word; episode ids start at 0
    assert variants or (seed, stream) == X.MATCH_CASES[0]
    for what, s, it, _ in variants:
        got = xr.match(t["adv"], t["cfr"], X.MATCH_N, X.MATCH_TEAM0, s, it)
        assert not np.array_equal(got.deal, m.deal) and not np.array_equal(got.leaf, m.leaf) and not np.array_equal(got.stats, m.stats), what


def test_one_deal_match_is_the_chance_match_of_that_deal():
    """an episode that drew deal d ends where the one-deal match ends on d with the scattered tables"""
    cr, xr, t = TS.chance_ref("reordered"), X.xref("reordered"), X.tables("reordered")
    m = xr.match(t["adv"], t["uniform"], X.MATCH_N, X.MATCH_TEAM0, W.WIDE_SEED, 16)
    for d in range(2):
        one = X.XRef.one(cr.perms[d]).match(cr.policy_for_deal(t["adv"], d), cr.policy_for_deal(t["uniform"], d), X.MATCH_N, X.MATCH_TEAM0, W.WIDE_SEED, 16)
        sel = m.deal == d
        assert sel.sum() > 1000 and np.array_equal(one.leaf[sel], m.leaf[sel])
    assert np.all(one.deal == 0)


@pytest.mark.parametrize("name", SETS)
def test_long_match_means_within_five_standard_errors_of_the_exact_targets(name):
    """adv is unnormalised: a match plays its rows normalised by the thresholds' cdf / cdf_last while the exact pass uses rows as given, so the pair
    is (the rows a match plays from adv, cfr): tables on which the cross-play is the match's own law"""
    xr, t = X.xref(name), X.tables(name)
    played = X.normalised(TS.chance_ref(name), t["adv"])
    exact = xr.cross_play([played, t["cfr"]])[0]
    n, first = X.LONG_N, X.LONG_N // 2
    m = xr.match(played, t["cfr"], n, first, X.LONG_SEED, X.LONG_STREAM)
    for mean, target, se in X.standard_error_check(m.stats, exact, first, n):
        assert se > 0 and abs(mean - target) <= 5 * se, (mean, target, se)


def test_header_binding_and_library_agree():
    hdr = open(os.path.join(ROOT, "include", "scopa.h")).read()
    names = {"scopa_team_cross_play", "scopa_team_match", "scopa_team_chance_cross_play", "scopa_team_chance_match", "scopa_team_debug_xplay_group_limit"}
    declared = set(re.findall(r"^int32_t (scopa_team_[a-z_]+)\s*\(", hdr, re.M))
    assert names <= declared
    import scopa_amd._lib as sl
    assert names <= set(sl.SYMBOLS)
    L = sl.lib()
    for name in names:
        assert hasattr(L, name)
