"""The restatement of Deep CFR's traversal on Team MiniScopa (tests/team_sdcfr_ref.py) against the reference's own run (tests/golden/team_sdcfr.npz,
written by tests/tools/gen_team_sdcfr_golden.py from DeepCFR(TPIMiniScopaGame)), and the CPU guards of tests/test_gpu_team_chance_sdcfr.py: features
are a function of the key, the threshold rule on hand-made rows, the conditioning of the nets the GPU policy test uses, the separation of the wide
Philox words.  No GPU."""
import os

import numpy as np
import pytest

import philox_words as W
import team_chance_sets as TS
import team_sdcfr_ref as S
from team_cfr_ref import N_CHOICE, OFFSET

ATOL = 1e-5


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(S.GOLDEN, "team_sdcfr.npz"))


# ---- the reference's own traversal ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("traverser", [0, 1])
def test_mode_a_reproduces_the_reference_fixture(golden, traverser):
    """the other team's cards scripted from the fixture, the policies the restatement's own float64 forward: rows in the reference's append order with
    features and masks exact, regrets and the root value to 1e-5, 1 653 rows, the visit counts of the tree's shape"""
    perm, nets, t = golden["perm"], S.golden_nets(), traverser
    xbits, hand, fx, _ = S.node_info(perm)
    own = S.own_policy(nets)

    def policy(depth, node, xb, cards):   # the state the recursion stands on has the bits the level-wise walk gives its (depth, node)
        assert xb == (int(xbits[OFFSET[depth] + node]) if depth < 12 else int(fx[depth - 12][node]))
        if depth < 12:
            assert cards == [(int(hand[OFFSET[depth] + node]) >> (4 * k)) & 15 for k in range(len(cards))]
        return own(depth, node, xb, cards)

    sampled = golden[f"t{t}_draw_action"][golden[f"t{t}_draw_options"] > 1]
    tr = S.Traversal(perm, t, policy, S.scripted(sampled))
    bits, reg, mask = tr.arrays()
    assert len(tr.rows) == S.ROWS == golden[f"t{t}_row_bits"].shape[0]
    assert np.array_equal(bits, golden[f"t{t}_row_bits"]) and np.array_equal(mask, golden[f"t{t}_row_mask"])
    assert np.array_equal(mask, (bits & 0xFFFF).astype(np.uint16))                       # the mask is the hand's one-hot
    np.testing.assert_allclose(reg, golden[f"t{t}_row_regret"], atol=ATOL, rtol=0)
    assert abs(float(tr.value) - float(golden[f"t{t}_value"][0])) <= ATOL and bool(golden[f"t{t}_value_is_f32"][0])
    assert np.array_equal(tr.visits, golden[f"t{t}_visits_by_depth"]) and len(tr.sampled) == len(sampled)
    assert int(tr.visits.sum()) == S.VISITS[t] and int(tr.visits[:12].sum()) == S.CHOICE_VISITS[t] and int(tr.visits[12]) == S.ARRIVALS


def test_fixture_counts_and_forced_rows(golden):
    """1 653 = 501 choice rows + 1 152 forced rows; a forced row's fifteen illegal slots hold -value and its legal slot 0 -- except where the net's
    advantage of the one legal card is not positive: then the policy is 0, the node's value 0 and the legal slot holds the child's value.  The
    fixture has such rows for both traversers, which is why the forced nodes' nets are evaluated"""
    for t in (0, 1):
        mask, reg = golden[f"t{t}_row_mask"], golden[f"t{t}_row_regret"]
        nl = np.array([bin(int(m)).count("1") for m in mask])
        assert (nl == 1).sum() == 1152 and (nl > 1).sum() == 501
        forced = np.nonzero(nl == 1)[0]
        legal = reg[forced, np.log2(mask[forced].astype(np.float64)).astype(np.int64)]
        off = np.array([np.delete(reg[i], int(np.log2(mask[i]))) for i in forced])
        assert (off == off[:, :1]).all()                                                 # fifteen equal slots
        zero_policy = legal != 0
        assert 0 < zero_policy.sum() < len(forced)
        assert (off[zero_policy] == 0).all()                                             # value 0: the illegal slots hold -0
        assert golden[f"t{t}_visits_by_depth"].sum() == S.VISITS[t]
        assert golden[f"t{t}_draw_uniform"].sum() > 0                                    # the zero-sum fall-back occurs in the reference's run


def test_mode_c_runs_on_its_own_policies(golden):
    tr = S.Traversal(golden["perm"], 1, S.own_policy(S.golden_nets()), S.numpy_chooser(np.random.default_rng(5)))
    assert len(tr.rows) == S.ROWS and int(tr.visits.sum()) == S.VISITS[1]


# ---- features are a function of the key -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["reordered", "both4"])
def test_features_are_a_function_of_the_key(name):
    cr, perms = TS.chance_ref(name), TS.deal_set(name)
    info = [S.node_info(p) for p in perms]
    xb = np.concatenate([i[0] for i in info])
    hand = np.concatenate([i[1] for i in info])
    first = cr.occ[cr.occ_off[cr.map.reshape(-1)]]                                       # every occurrence's key's first occurrence
    assert (np.diff(cr.occ_off) > 1).any()
    assert np.array_equal(xb, xb[first]) and np.array_equal(hand, hand[first])
    assert np.array_equal(xb & 0xFFFF, sum((1 << ((hand.astype(np.uint32) >> (4 * k)) & 15)) * (k < S.legal_count_of_rows()[np.arange(len(hand)) % N_CHOICE])
                                           for k in range(4)))


# ---- the threshold rule --------------------------------------------------------------------------------------------------------------------------------
def test_threshold_rule_on_hand_made_rows():
    f = np.float32
    rows = np.array([[0, 0, 0, 0], [0, 1, 0, 0], [0.5, 0.5, 0, 0], [0.25, 0.25, 0.5, 0], [0.25, 0.25, 0.25, 0.25], [0, 0, 1, 0], [1, 0, 0, 0]], f)
    nl = np.array([4, 4, 2, 3, 4, 3, 2])
    thr = S.thresholds(rows, nl)
    T = 1 << 53
    assert thr.tolist() == [[int(S.ZERO_SUM), T, T], [0, T, T], [T // 2, T, T], [T // 4, T // 2, T], [T // 4, T // 2, 3 * T // 4], [0, 0, T], [T, T, T]]
    # the draw N = 0 .. 2^53 - 1 picks #{k : thr[k] <= N}: a single positive entry is always taken, equal halves split at 2^52
    assert [S.action_of(thr[1], N, 4) for N in (0, T - 1)] == [1, 1] and [S.action_of(thr[5], N, 3) for N in (0, T - 1)] == [2, 2]
    assert [S.action_of(thr[2], N, 2) for N in (0, T // 2 - 1, T // 2, T - 1)] == [0, 0, 1, 1]
    assert [S.action_of(thr[0], N, 4) for N in (0, T // 4 - 1, T // 4, T - 1)] == [0, 0, 1, 3]   # a zero sum: numpy's (int)(u * 4)
    # float32 rounding of p / sum enters: the rule is sd_thresholds' (scopa_sdcfr_tile.h), on the float32 row, not the exact ratio
    row = np.array([[0.1, 0.2, 0.3, 0]], f)
    s = f(f(row[0, 0] + row[0, 1]) + row[0, 2])
    q = (row[0] / s).astype(f).astype(np.float64)
    exp = [int(np.ceil(q[0] / (q[0] + q[1] + q[2]) * 2.0 ** 53)), int(np.ceil((q[0] + q[1]) / (q[0] + q[1] + q[2]) * 2.0 ** 53)), T]
    assert S.thresholds(row, [3]).tolist() == [exp]


# ---- the nets of the GPU policy test ---------------------------------------------------------------------------------------------------------------------
def test_gpu_policy_nets_keep_the_reference_well_conditioned():
    """tests/test_gpu_team_chance_sdcfr.py compares policies only at rows whose float64 positive-advantage sum z is at least 1e-3 and lets at most 2 %
    of the rows fall below: the fixture's nets on `reordered` stay inside that (choice rows and each traverser's forced nodes), and the zero-sum nets
    (head bias -10) have z = 0 everywhere, so that every row takes the marker"""
    perms, nets = TS.deal_set("reordered"), S.golden_nets()
    zero = [S.with_head_bias(n, -10.0) for n in nets]
    for d in range(2):
        pol, z, fpol, fz = TS.cached(("tsd64", "reordered", d), lambda: S.float64_tables(perms[d], nets, None))
        assert (z < 1e-3).mean() <= 0.02
        assert np.abs(pol.sum(1) - 1.0)[z >= 1e-3].max() <= 1e-12
    for t in (0, 1):
        assert (S.forced64(perms[0], nets, t, stride=8)[1] < 1e-3).mean() <= 0.02
    xb = S.node_info(perms[0])[0][::97]
    for t in (0, 1):
        assert (S.policy64(zero[t], xb)[1] == 0).all()


# ---- the Philox words -----------------------------------------------------------------------------------------------------------------------------------
def test_wide_words_separate():
    """every (seed, iteration, b0) of the GPU walk test's wide cases gives other sampled cards than the same words narrowed (philox_words.narrowed):
    the GPU test compares features exactly, and the features of a traversal's rows follow from the sampled cards"""
    perm = TS.deal_set("reordered")[0]
    xbits, hand, _, _ = S.node_info(perm)
    pol = np.zeros((N_CHOICE, 4), np.float32)                                           # zero sums: the uniform arithmetic, a draw at every visit
    thr = S.thresholds(pol, S.legal_count_of_rows())
    fp = np.ones((2, 1), np.float32)
    policy = lambda depth, node, xb, cards: np.ones(len(cards), np.float32) / np.float32(len(cards)) if depth < 12 else fp[0]

    def cards(seed, iteration, trav_id):
        return S.Traversal(perm, 1, policy, S.philox_chooser(thr, 1, trav_id, iteration, seed)).sampled

    for seed, iteration, b0 in S.word_cases(2, 2):
        ids = W.ids_of(b0, 2)
        want = [cards(seed, iteration, i) for i in ids]
        for what, s2, it2, ids2 in W.narrowed(seed, iteration, b0, 2):
            assert [cards(s2, it2, i) for i in ids2] != want, (what, hex(seed), hex(iteration), hex(b0))


# ---- the average policy's definition --------------------------------------------------------------------------------------------------------------------
def test_average_policy_definition():
    cr, perms, nets = TS.chance_ref("reordered"), TS.deal_set("reordered"), S.golden_nets()
    rows, tab, _ = S.average_policy(cr, perms, 0, [], [])
    nl = cr.nleg[rows]
    assert (cr.team[rows] == 0).all() and np.array_equal(tab, np.where(np.arange(4)[None, :] < nl[:, None], 1.0 / nl[:, None], 0.0))
    rows, tab, z = S.average_policy(cr, perms, 1, [nets[1]], [1.0])
    assert np.abs(tab.sum(1) - 1.0).max() <= 1e-12 and (tab[np.arange(4)[None, :] >= cr.nleg[rows][:, None]] == 0).all()
    rows2, nan_tab, _ = S.average_policy(cr, perms, 1, [nets[1], nets[0]], [0.5, float("nan")])   # a slot outside the store: NaN, hence uniform
    assert np.array_equal(nan_tab, np.where(np.arange(4)[None, :] < cr.nleg[rows2][:, None], 1.0 / cr.nleg[rows2][:, None], 0.0))
