"""CPU checks that hold the level-by-level restatement of the response to the nets (tests/full_chance_respond_nets_ref.py) to the depth-first
restatement of the response to a store (tests/full_chance_respond_ref.py), which tests/test_full_chance_respond_ref.py holds to exact enumeration:
with the opponent a planted Rows read by F.average_probs the two must meet the same pairs with the same counts and counters and add the same d_regret
bits, and one traversal per deck from zero tables must have the exact counterfactual regret as its expectation."""
import numpy as np
import pytest

import full_chance_ref as X
import full_mccfr_ref as F
import full_chance_respond_nets_ref as N
import full_chance_respond_ref as Q
import test_full_chance_respond_ref as TR
import test_gpu_full_chance as G                   # (fixture builders are plain CPU code; only the modules' tests carry the gpu mark)
import test_gpu_full_chance_respond as GR
from test_gpu_full_chance_sdcfr import SHAPES, packet

SEED = G.SEED
_CASES = {}


def case(oracle, R):
    """(root state, decks, the planted opponent, the responder's planted regrets by pair) of SHAPES[R]: X.rows_for on every pair of the sub-game, so
    neither the opponent's policy nor the responder's sigma is uniform"""
    if R not in _CASES:
        r0, n, fix = SHAPES[R]
        decks, _, st = packet(oracle, r0, n, fix)
        keys = X.subgame_keys(st, decks)
        Rr, S = X.rows_for(keys)
        _CASES[R] = (st, decks, GR.planted_rows(keys, Rr, S), (keys, Rr))
    return _CASES[R]


def assert_same_rows(a, b, what):
    assert (a.choice, a.terminal) == (b.choice, b.terminal), what
    assert a.count == b.count and len(a.count) > 3, what
    for k in a.count:
        assert np.array(a.dR[k]).tobytes() == np.array(b.dR[k]).tobytes(), (what, X.key_to_string(k))
        assert np.array(a.A[k]).tobytes() == np.array(b.A[k]).tobytes() and not any(b.dS[k]), what
        assert GR.player_of(k) == what[1]


@pytest.mark.parametrize("nb", [1, 5])
@pytest.mark.parametrize("resp", [0, 1])
@pytest.mark.parametrize("R", [1, 2])
def test_level_by_level_equals_the_depth_first_walk_on_bits(oracle, R, resp, nb):
    st, decks, opp, (keys, Rr) = case(oracle, R)
    probs_at = N.rows_probs_at(opp)
    lists = [None, (2, 0)] if nb == 5 else [None]                          # a list with m < n in permuted order
    for listed in lists:
        for planted in (False, True):                                      # zero tables, and regrets that make sigma non-uniform
            a = GR.planted_rows(keys, Rr, np.zeros_like(Rr)) if planted else X.Rows()
            b = GR.planted_rows(keys, Rr, np.zeros_like(Rr)) if planted else X.Rows()
            Q.traverse(st, decks, resp, 3, 5, nb, SEED, a, opp, 0, listed)
            vals = N.traverse(st, decks, resp, 3, 5, nb, SEED, b, probs_at, listed)
            assert_same_rows(a, b, (R, resp, nb, listed, planted))
            m = len(decks) if listed is None else len(listed)
            assert vals.shape == (m * nb,) and (a.choice, a.terminal) == (m * nb * F.shape_counts(6 - R)[resp], m * nb * 6 ** R)
    # uniform play: zero rows are the opponent None
    a, b = X.Rows(), X.Rows()
    Q.traverse(st, decks, resp, 0, 0, nb, SEED, a)
    N.traverse(st, decks, resp, 0, 0, nb, SEED, b, N.uniform_probs_at)
    assert_same_rows(a, b, (R, resp, nb, "uniform"))
    # ... and the opponent matters
    c = X.Rows()
    N.traverse(st, decks, resp, 0, 0, nb, SEED, c, probs_at)
    assert c.count != b.count or any(c.dR[k] != b.dR[k] for k in c.count)


def test_iterate_equals_the_depth_first_iterate(oracle):
    st, decks, opp, _ = case(oracle, 1)
    a, b = X.Rows(), X.Rows()
    ca = cb = 0
    for _ in range(2):
        ca = Q.iterate(st, decks, 3, SEED, a, ca, opp, 0)
        cb = N.iterate(st, decks, 3, SEED, b, cb, N.rows_probs_at(opp))
    assert ca == cb == 4 and a.R.keys() == b.R.keys()
    for k in a.R:
        assert np.array(a.R[k]).tobytes() == np.array(b.R[k]).tobytes()


@pytest.mark.parametrize("resp", [0, 1])
def test_walk_is_unbiased_under_a_planted_opponent(oracle, resp):
    """test_full_chance_respond_ref's case (R = 1 on 3 decks, its edge opponent): sample t is traversal id t's d_regret rows over the decks from zero
    tables; its mean over 4 096 ids is held, cell by cell, to the exact counterfactual regret under the opponent's probabilities, within 5
    standard errors"""
    st, decks, keys = GR.bound_case(oracle)[:3]
    opp = TR.edge_opponent(keys)
    exact = Q.exact_regret(st, decks, resp, opp, 0)
    probs_at = N.rows_probs_at(opp)
    n = 4096
    cells = sorted(exact)
    col = {k: i for i, k in enumerate(cells)}
    inc = np.zeros((n, len(cells), 3))
    for t in range(n):
        rows = X.Rows()
        N.traverse(st, decks, resp, 0, t, 1, SEED, rows, probs_at)
        assert not any(any(v) for v in rows.dS.values()) and all(GR.player_of(k) == resp for k in rows.count)
        for k, dr in rows.dR.items():
            inc[t, col[k]] = dr                                                # (a pair outside `exact` would be a KeyError)
    mean, se = inc.mean(0), inc.std(0, ddof=1) / np.sqrt(n)
    want = np.array([exact[k] for k in cells])
    err = np.abs(mean - want)
    sure = se == 0.0
    assert (err[sure] <= 1e-12).all()
    ratio = err[~sure] / se[~sure]
    print("rows", len(cells), "largest |mean - exact| / se:", ratio.max())
    assert len(cells) >= 10 and (~sure).sum() >= 20
    assert (ratio <= 5.0).all()
