"""tests/chance_xplay_ref.py against tests/chance_ref.py on the six-deal set of tests/test_gpu_chance.py, on the CPU: the restatement the GPU tests hold
scopa_chance_cross_play, scopa_chance_best_response and scopa_chance_match to is itself anchored to ChanceRef.exploitability, which
tests/test_chance_ref.py anchors to the C oracle."""
import numpy as np
import pytest

import chance_xplay_ref as X
from cfr_edges import same_bits


def test_set_preconditions(oracle):
    s = X.six(oracle)
    c = s["cref"]
    assert (c.n, c.G, c.n_occ) == (6, 3522, 3860)
    assert len(c.shared_hand_sizes(0)) >= 3 and len(c.shared_hand_sizes(1)) >= 3
    uniform, solved, dirichlet, onehot = s["pols"]
    for P in s["pols"]:
        assert (P[~c.legal] == 0.0).all() and np.abs(P.sum(1) - 1.0).max() <= 1e-12
    assert ((onehot == 1.0).sum(1) == 1).all() and np.abs(solved - uniform).max() > 0.1


def test_cross_play_diagonal_is_the_exploitability_value(oracle):
    s = X.six(oracle)
    per, out = X.six_cross(oracle)
    assert per.shape == (6, 4, 4, 4) and out.shape == (4, 4, 4)
    for k, P in enumerate(s["pols"]):
        assert same_bits(out[k, k, 0], s["cref"].exploitability(P)[3]), s["names"][k]
    assert len({per[d, 1, 2, 0] for d in range(6)}) == 6                                   # the deals differ: the mean is a mean of six numbers


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_best_response_values_and_tables(oracle, k):
    s = X.six(oracle)
    c, x, P = s["cref"], s["xref"], s["pols"][k]
    out4, (br0, br1) = X.six_best(oracle, k)
    want = c.exploitability(P)
    assert same_bits(out4, want), s["names"][k]
    for p, br in enumerate((br0, br1)):
        mine = c.player == p
        assert same_bits(br[~mine], P[~mine])
        assert ((br[mine] == 1.0).sum(1) == 1).all() and ((br[mine] == 0.0).sum(1) == 3).all()      # one-hot ...
        assert (br[mine].argmax(1) < c.nlegal[mine]).all()                                           # ... and legal
    # the tables played back: the orders of summation differ (cross-play sums children per node, the response sums nodes per cell), so not bit-equal
    v0 = x.mean(x.cross_per_deal([br0, P]))[0, 1, 0]
    v1 = x.mean(x.cross_per_deal([P, br1]))[0, 1, 0]
    print(f"{s['names'][k]}: BR0 {out4[1]!r} played {v0!r}; BR1 {out4[2]!r} played {-v1!r}")
    assert abs(v0 - out4[1]) <= 1e-12 and abs(-v1 - out4[2]) <= 1e-12
    assert out4[1] >= out4[3] - 1e-12 and out4[3] >= -out4[2] - 1e-12


def test_match_draws_every_deal_and_its_mean_is_near_the_exact_reward(oracle):
    """n = 20 001 episodes, 10 001 with the solved policy in seat 0, against the Dirichlet table; stream 16 under the default seed 0x5C09A, chosen on
    the CPU as the first pair tried: the reference's mean sits z = -1.26 standard errors from the exact reward (the condition is 4)."""
    s = X.six(oracle)
    x = s["xref"]
    per, out = X.six_cross(oracle)
    n, first = X.MATCH_N, X.MATCH_SEAT0
    deal, idx, st = X.six_match(oracle, 1, 2)
    assert sorted(set(deal.tolist())) == list(range(6)) and np.bincount(deal, minlength=6).min() > n // 12
    assert st[:, 0].tolist() == [first, n - first]
    # the exact mean and second moment of the solved policy's reward, seat halves weighted as played
    exact = (first * out[1, 2, 0] - (n - first) * out[2, 1, 0]) / n
    m2 = (first * out[1, 2, 1] + (n - first) * out[2, 1, 1]) / n
    var = (first * (out[1, 2, 1] - out[1, 2, 0] ** 2) + (n - first) * (out[2, 1, 1] - out[2, 1, 0] ** 2)) / n      # within the halves
    se = np.sqrt(var / n)
    mean = st[:, 1].sum() / 2 / n
    z = (mean - exact) / se
    print(f"sampled {mean:+.6f}, exact {exact:+.6f}, second moment {m2:.6f}, standard error {se:.6f}, z = {z:+.2f}")
    assert se > 0.0 and abs(z) <= 3.0                                                      # the reference itself; the GPU test allows the issue's 4
    # the integer sums are the sums over the episodes' terminals
    r2 = np.array([x.x[d].term_r2[i] for d, i in zip(deal, idx)])
    seat = (np.arange(n) >= first).astype(np.int64)
    mine = r2[np.arange(n), seat]
    assert st[:, 1].sum() == mine.sum() and st[:, 2].sum() == (mine * mine).sum()
