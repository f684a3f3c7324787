"""GPU checks of the sampled best response of FullScopa over a set of decks (k_full_chance_respond, k_full_chance_harden; respond_traverse,
respond_iterate and harden of include/scopa.h; FullChanceMCCFRTrainer.sampled_response and full_chance.sampled_exploitability) against the restatement
tests/full_chance_respond_ref.py, which tests/test_full_chance_respond_ref.py holds to exact enumeration under a planted opponent, to
full_chance_ref.traverse on bits, and to the exact sweeps' best response.

The standard is tests/test_gpu_full_chance.py's (assert_delta): pair set, visit counts and counters exact, d_strategy exact (all zero here: the response
walk never writes it), a d_regret row met once bit-identical, the rest within the reorder budget (in_budget).  Fixtures are that module's: solver_of,
4 decks, capacity_log2 14.  The builders below are plain CPU code; only the tests carry the gpu mark."""
import numpy as np
import pytest

import full_chance_ref as X
import full_chance_respond_ref as Q
import full_mccfr_ref as F
import philox_words as W
import test_gpu_full_chance as G
import test_gpu_full_chance_depth as GD
from test_gpu_full_chance import N_DECKS, SEED, assert_delta, cuts_of, deck_set, solver_of
from test_gpu_full_mccfr import same_bits

pytestmark = pytest.mark.gpu

# the bound case (6): round-5 root of deck 7, 3 decks of its packet with no seat fixed, the opponent X.rows_for on every pair of the sub-game
BOUND = dict(deck_seed=7, r0=5, n=3, fix_seat=None, iterations=8, batch=48)
_CACHE = {}


def rows_of(h):
    """a handle's tables as the restatement reads an opponent: Rows with R and S planted"""
    keys, _, R, S = h.tables_get()
    rows = X.Rows()
    rows.plant(keys, R, S)
    return rows


def planted_rows(keys, R, S):
    rows = X.Rows()
    rows.plant(keys, R, S)
    return rows


def player_of(key):
    return (int(key[0]) >> 62) & 1


def opponent_of(ctx, sl, oracle, kind, deck_seed, r0):
    """(handle or None, which, the restatement's view of it) for a kind of fixed opponent: `planted` G.planted's four edge rows (a zero-sum strategy
    row, a one-hot, a mixed one; regrets with one positive, negatives only, two positives, zeros), read as the average policy (0) or by regret
    matching (1); `trained` 3 iterate calls at batch 4; `empty` a store without rows; `null` no store"""
    name, _, which = kind.partition("-")
    which = int(which or 0)
    if name == "null":
        return None, which, None
    h, _, _ = solver_of(ctx, sl, oracle, deck_seed, r0)
    if name == "planted":
        _, _, K, n_act, R, S = G.planted(oracle, deck_seed, r0)
        h.tables_set(K, n_act, R, S)
    elif name == "trained":
        for _ in range(3):
            h.iterate(4, 1)
    return h, which, rows_of(h)


def bound_case(oracle):
    """(root state, decks, pairs, n_act, regret, strategy of the planted opponent) of BOUND"""
    if "bound" not in _CACHE:
        b = BOUND
        decks, _, st = deck_set(oracle, b["deck_seed"], b["r0"], b["n"], b["fix_seat"])
        keys = X.subgame_keys(st, decks)
        R, S = X.rows_for(keys)
        _CACHE["bound"] = (st, decks, keys, np.array([X.key_actions(k) for k in keys], np.int32), R, S)
    return _CACHE["bound"]


def deal2(oracle, resp):
    """(decks [2][40], root, the planted opponent's pairs, n_act, regret, strategy) for the deal's root: the first two decks of
    test_gpu_full_chance_depth's DEAL3; the opponent holds X.rows_for on every pair of player 1 - resp that DEAL3's reference traversal of that
    player met (tens of thousands of rows from every round), so the response walk probes a full store at every depth"""
    if ("deal2", resp) not in _CACHE:
        decks, root = GD.deal3(oracle)
        met = GD.deal3_ref(oracle, 1 - resp)[0].count
        keys = np.array(sorted(k for k in met if player_of(k) == 1 - resp), np.uint64).reshape(-1, 2)
        R, S = X.rows_for(keys)
        _CACHE["deal2", resp] = (decks[:2], root, keys, np.array([X.key_actions(k) for k in keys], np.int32), R, S)
    return _CACHE["deal2", resp]


def deal2_ref(oracle, resp):
    if ("deal2_ref", resp) not in _CACHE:
        decks, root, keys, _, R, S = deal2(oracle, resp)
        rows = X.Rows()
        Q.traverse(root, decks, resp, 0, 0, 1, SEED, rows, planted_rows(keys, R, S), resp)      # which = resp: both rules are walked
        _CACHE["deal2_ref", resp] = rows
    return _CACHE["deal2_ref", resp]


def assert_response_delta(h, rows, resp, what, hidden=()):
    keys, counts = assert_delta(h, rows, what, hidden)
    assert not h.delta_get()[3].any(), f"{what}: d_strategy written"
    assert all(player_of(k) == resp for k in keys.tolist()), f"{what}: a pair of the opponent claimed"
    return keys, counts


# ---- 1. one launch against the restatement, by every cut, from zero tables ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["planted-0", "planted-1", "trained-0", "trained-1", "empty", "null"])
@pytest.mark.parametrize("nb", [1, 5])
@pytest.mark.parametrize("resp", [0, 1])
@pytest.mark.parametrize("r0", [4, 3])
def test_one_launch_vs_restatement_by_every_cut(ctx, sl, oracle, r0, resp, nb, kind):
    h, st, decks = solver_of(ctx, sl, oracle, 42, r0)
    opp, which, opp_rows = opponent_of(ctx, sl, oracle, kind, 42, r0)
    rows = X.Rows()
    Q.traverse(st, decks, resp, 0, 0, nb, SEED, rows, opp_rows, which)
    assert (rows.choice, rows.terminal) == (N_DECKS * nb * F.shape_counts(r0)[resp], N_DECKS * nb * F.shape_counts(r0)[2])
    for n, cut in enumerate(cuts_of(r0)):
        h.reset()
        h.cut(cut)
        h.respond_traverse(opp, which, resp, 0, 0, nb)
        keys, counts = assert_response_delta(h, rows, resp, f"round {r0}, responder {resp}, nb {nb}, {kind}, cut {cut}")
        c = h.counters()
        assert (c["choice_visits"], c["terminal_visits"]) == ((n + 1) * rows.choice, (n + 1) * rows.terminal)
        assert (c["rows"], c["dropped"], c["iterations"]) == (counts.size, 0, 0) and counts.sum() == sum(rows.count.values())
        got = h.tables_get()
        assert not got[2].any() and not got[3].any()                      # respond_traverse writes increments only


# ---- 2. batch 1, cut 0, one deck listed: two respond_iterate calls on bits ----------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1])
def test_two_respond_iterate_calls_bit_for_bit(ctx, sl, oracle, which):
    st, decks, K, n_act, R, S = G.planted(oracle)
    h, _, _ = solver_of(ctx, sl, oracle, 42, 4)
    opp, _, _ = solver_of(ctx, sl, oracle, 42, 4)
    opp.tables_set(K, n_act, R, S)
    h.cut(0)
    rows, counter = X.Rows(), 0
    for deck in (2, 1):                                                   # ONE lane makes every add of a launch in the restatement's own depth-first order
        counter = Q.iterate(st, decks, 1, SEED, rows, counter, planted_rows(K, R, S), which, listed=[deck])
        h.respond_iterate(opp, which, 1, 1, lists=[[deck]])
        assert h.counters()["iterations"] == counter
        keys, _, R2, S2 = h.tables_get()
        assert np.array_equal(keys, rows.arrays("R")[0]) and same_bits(R2, rows.arrays("R")[1]) and not S2.any()
        assert not h.delta_get()[1].any()
    assert counter == 4 and R2.any()


# ---- 3. the opponent is untouched ---------------------------------------------------------------------------------------------------------------------------
def test_opponent_is_untouched_and_an_empty_one_is_uniform_play(ctx, sl, oracle):
    h, _, _ = solver_of(ctx, sl, oracle, 42, 4)
    opp, _, _ = solver_of(ctx, sl, oracle, 42, 4)
    opp.iterate(4, 2)
    opp.traverse(0, 4, 0, 3)                                              # increments and visit counts left standing in the opponent's store
    before = (opp.tables_get(), opp.delta_get(), opp.counters())
    assert before[1][1].any() and before[1][2].any()
    for which in (0, 1):
        for cut in cuts_of(4):
            h.cut(cut)
            h.respond_traverse(opp, which, 1, 0, 0, 3)
        h.respond_iterate(opp, which, 2, 2)
        h.harden()
    after = (opp.tables_get(), opp.delta_get(), opp.counters())
    assert before[2] == after[2]
    for a, b in zip(before[0] + before[1], after[0] + after[1]):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    # an empty store and no store: the same bits (cut 0, nb 1, one deck listed: one lane, one order of adds)
    empty, _, _ = solver_of(ctx, sl, oracle, 42, 4)
    got = []
    for o in (empty, None):
        for which in (0, 1):
            h.reset()
            h.cut(0)
            h.respond_traverse(o, which, 0, 7, 3, 1, [2])
            got.append(h.delta_get())
    assert got[0][1].any()
    for g in got[1:]:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[0], g))
    assert empty.counters()["rows"] == 0


# ---- 4. lists and wide words ----------------------------------------------------------------------------------------------------------------------------------
def test_lists(ctx, sl, oracle):
    deck_seed, r0, resp, nb = 42, 3, 1, 3
    h, st, decks = solver_of(ctx, sl, oracle, deck_seed, r0)
    opp, which, opp_rows = opponent_of(ctx, sl, oracle, "trained-0", deck_seed, r0)
    rows, full = X.Rows(), X.Rows()
    Q.traverse(st, decks, resp, 0, 0, nb, SEED, rows, opp_rows, which, listed=(0, 2, 3))
    Q.traverse(st, decks, resp, 0, 0, nb, SEED, full, opp_rows, which)
    assert set(rows.count) < set(full.count)
    got = []
    for listed in ([0, 2, 3], [3, 0, 2]):                                 # a permuted list, m < n: no draw of a listed deck changes
        for cut in (0, -1):
            h.reset()
            h.cut(cut)
            h.respond_traverse(opp, which, resp, 0, 0, nb, listed)
            assert_response_delta(h, rows, resp, f"list {listed}, cut {cut}")
            got.append(h.delta_get())
    assert all(np.array_equal(got[0][0], g[0]) and np.array_equal(got[0][1], g[1]) for g in got)
    h.respond_traverse(opp, which, resp, 0, 0, nb, [])                    # an empty list is a no-op
    assert h.counters()["choice_visits"] == 4 * rows.choice
    # respond_iterate with a list per iteration = the respond_traverse / apply sequence
    lists = [[1, 3], [0, 2], [2, 1]]
    h1, _, _ = solver_of(ctx, sl, oracle, deck_seed, r0)
    h2, _, _ = solver_of(ctx, sl, oracle, deck_seed, r0)
    h1.respond_iterate(opp, which, 2, 3, lists=lists)
    for t, lst in enumerate(lists):
        for r in range(2):
            h2.respond_traverse(opp, which, r, 2 * t + r, 0, 2, lst)
            h2.apply()
    assert h1.counters() == h2.counters() and h1.counters()["iterations"] == 6
    assert np.array_equal(h1.tables_get()[0], h2.tables_get()[0])
    assert h1.counters()["choice_visits"] == 3 * 2 * 2 * sum(F.shape_counts(r0)[:2])


def test_wide_words_and_a_deck_index_above_255(ctx, sl, oracle):
    """b0 = 2^32 - nb, iteration bit 31, both seed words, deck indices 297..299 of a handle of 300 decks below a round-5 root, against an opponent that
    holds X.rows_for on every pair of the listed decks' sub-games"""
    w = G.WIDE
    seed, iteration, b0 = W.WIDE_SEED, W.ITER_B31, (1 << 32) - w["nb"]
    decks, _, st = deck_set(oracle, w["deck_seed"], w["r0"], w["n"], None)
    keys = X.subgame_keys(st, decks[list(w["listed"])])
    R, S = X.rows_for(keys)
    for resp in range(2):
        rows = X.Rows()
        Q.traverse(st, decks, resp, iteration, b0, w["nb"], seed, rows, planted_rows(keys, R, S), resp, listed=w["listed"])
        h, _, _ = solver_of(ctx, sl, oracle, w["deck_seed"], w["r0"], seed=seed, n=w["n"], fix_seat=None)
        opp, _, _ = solver_of(ctx, sl, oracle, w["deck_seed"], w["r0"], seed=seed, n=w["n"], fix_seat=None)
        opp.tables_set(keys, [X.key_actions(k) for k in keys], R, S)
        with pytest.raises(sl.ScopaError) as e:
            h.respond_traverse(opp, resp, resp, iteration, b0 + 1, w["nb"], list(w["listed"]))   # b0 + nb overflows
        assert e.value.status == sl.SCOPA_EINVAL and h.counters()["rows"] == 0
        for cut in cuts_of(w["r0"]):
            h.reset()
            h.cut(cut)
            h.respond_traverse(opp, resp, resp, iteration, b0, w["nb"], list(w["listed"]))
            assert_response_delta(h, rows, resp, f"wide words, responder {resp}, cut {cut}")
        h.close()
        opp.close()


# ---- 5. harden --------------------------------------------------------------------------------------------------------------------------------------------------
def chain_for(oracle, resp=0, nb=2):
    """G.deep_chain for a response launch against uniform play: 64 fillers before the root pair's home, in the smallest store of 2^16 .. 2^20 slots in
    which no other pair of the launch lies near the chain -> (capacity_log2, fillers, root pair, the launch's restatement)"""
    decks, _, st = deck_set(oracle, 42, 4)
    root_pair = X.wide_key(X.root_on(st, decks[0]), 0)
    rows = X.Rows()
    Q.traverse(st, decks, resp, 0, 0, nb, SEED, rows)
    others = np.array([k for k in rows.count if k != root_pair], np.uint64)
    for capacity_log2 in range(16, 21):
        mask = (1 << capacity_log2) - 1
        g = (int(X.home_of(root_pair[0], root_pair[1], capacity_log2)[0]) - 1) & mask
        d = (X.home_of(others[:, 0], others[:, 1], capacity_log2) - g + 64) & mask
        if not bool((d < 193).any()):
            return capacity_log2, X.fillers(g, 64, capacity_log2), root_pair, rows
    raise AssertionError("no store size isolates the chain")


def test_harden(ctx, sl, oracle):
    decks, _, st = deck_set(oracle, 42, 4)
    keys = [tuple(k) for k in X.subgame_keys(st, decks).tolist()]
    three = [k for k in keys if X.key_actions(k) == 3][:4]
    two = [k for k in keys if X.key_actions(k) == 2][:3]
    K = np.array(three + two, np.uint64)
    R = np.array([[1.0, 1.0, 0.5],            # a tie: the first
                  [0.0, 0.0, 0.0],            # all zero: slot 0
                  [-1.0, -2.0, -0.5],         # negatives only: the least negative
                  [0.25, 0.5, 0.5],           # a tie behind a smaller cell: slot 1
                  [-1.0, -2.0, 0.0],          # two cards: the third word (0.0, larger than both) is no slot
                  [-3.0, -2.0, 0.0],
                  [2.0, 2.0, 0.0]])
    want = [0, 0, 2, 1, 0, 1, 0]
    S = np.full((7, 3), 3.0) * (np.arange(3)[None, :] < np.array([3, 3, 3, 3, 2, 2, 2])[:, None])
    h, _, _ = solver_of(ctx, sl, oracle, 42, 4)
    h.tables_set(K, [X.key_actions(k) for k in K], R, S)
    h.harden()
    got = h.tables_get()
    order = np.lexsort((K[:, 1], K[:, 0]))
    assert np.array_equal(got[0], K[order]) and same_bits(got[2], R[order])          # regrets untouched
    assert same_bits(got[3], np.eye(3)[np.array(want)[order]])
    ref = planted_rows(K, R, S)
    Q.harden(ref)
    assert same_bits(got[3], ref.arrays("S")[1])
    # a pair behind 64 fillers, claimed there by a response launch; harden again after more training: every row is the restatement's
    cap, fill, root_pair, rows = chain_for(oracle)
    h, _, _ = solver_of(ctx, sl, oracle, 42, 4, capacity_log2=cap)
    G.set_rows(h, fill)
    h.respond_traverse(None, 0, 0, 0, 0, 2)
    assert_response_delta(h, rows, 0, "behind 64 fillers", hidden=fill)
    h.apply()
    for again in range(2):
        before = h.tables_get()
        h.harden()
        keys2, _, R2, S2 = h.tables_get()
        assert np.array_equal(keys2, before[0]) and same_bits(R2, before[2]) and h.counters()["dropped"] == 0
        ref = planted_rows(keys2, R2, before[3])
        Q.harden(ref)
        assert same_bits(S2, ref.arrays("S")[1]) and (S2.sum(1) == 1.0).all()
        at = [tuple(k) for k in keys2.tolist()].index(root_pair)
        assert R2[at].any() and S2[at].tolist() == np.eye(3)[int(np.argmax(R2[at]))].tolist()
        h.respond_iterate(None, 0, 2, 1)                                  # regrets are kept: training goes on


# ---- 6. the bound at one round to go ----------------------------------------------------------------------------------------------------------------------------
def test_response_attains_the_best_response_at_one_round_to_go(ctx, sl, oracle):
    """Round-5 root of deck 7, 3 decks of its packet (no seat fixed: 77 pairs), the opponent X.rows_for on every pair: a full-support policy that is
    not uniform.  With one round to go the sweep's response is THE best response, so what the hardened responder wins, exactly (cross_play), is at
    most BR0 / BR1 of opp.exploitability() after every iteration, and equals them to 1e-9 after N = 8 iterations at batch B = 48.

    N and B come from the restatement (tests/test_full_chance_respond_ref.py::test_bound_case_is_what_the_gpu_test_needs): over batches 8, 16, 24,
    32, 48, 64 and up to 48 iterations, the first N per batch at which the restatement's hardened response attains both values AND no argmax can
    turn on the order of the device's adds is none / 32 / 32 / 13 / 8 / 6; (8, 48) and (6, 64) have the fewest traversals (384 a deck and
    responder) and (8, 48) the smaller batch.  There the smallest positive gap between a row's best and second regret is 0.5 (bound 1e-6).
    FullScopa has rows whose best two regrets are EQUAL (two cards of one rank that score alike; the last two-card choice, where the round's last
    capture takes the table either way): 29 of the 75 rows here, so "every gap above 1e-6" cannot be had.  Each tied row is one of two kinds, held
    on the CPU: every add into the two cells was exactly 0.0, so any order gives 0.0 and the same first slot; or the two slots have equal exact
    response values (within 1e-12), so a flip between them changes no value.  (At (8, 32) the values are attained too, but one row ties by
    coincidence between slots whose values differ: that pair is not used.)"""
    b = BOUND
    st, decks, keys, n_act, R, S = bound_case(oracle)
    opp, _, _ = solver_of(ctx, sl, oracle, b["deck_seed"], b["r0"], n=b["n"], fix_seat=b["fix_seat"])
    resp, _, _ = solver_of(ctx, sl, oracle, b["deck_seed"], b["r0"], n=b["n"], fix_seat=b["fix_seat"])
    opp.tables_set(keys, n_act, R, S)
    e = opp.exploitability()
    for n in range(1, b["iterations"] + 1):
        resp.respond_iterate(opp, 0, b["batch"], 1)
        if n <= 4 or n == b["iterations"]:
            resp.harden()
            v0 = sl.FullChanceMCCFR.cross_play([resp, opp])[0][1][0]
            v1 = -sl.FullChanceMCCFR.cross_play([opp, resp])[0][1][0]
            print(f"iteration {n}: response wins {v0} of {e['br0']} in seat 0, {v1} of {e['br1']} in seat 1")
            assert v0 <= e["br0"] + 1e-12 and v1 <= e["br1"] + 1e-12
    assert abs(v0 - e["br0"]) <= 1e-9 and abs(v1 - e["br1"]) <= 1e-9


# ---- 7. the deal's root -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resp", [0, 1])
def test_deal_one_response_traversal_at_cut_3_and_cut_0(ctx, sl, oracle, resp):
    """nb = 1 on the first two decks of DEAL3 from the deal against a store of tens of thousands of planted rows, read as the average policy
    (responder 0) or by regret matching (responder 1): as test_gpu_full_chance_depth holds traverse there"""
    decks, root, keys, n_act, R, S = deal2(oracle, resp)
    rows = deal2_ref(oracle, resp)
    ctx.mccfr_seed(SEED)
    h = sl.FullChanceMCCFR(ctx, decks, None, GD.CAP)
    opp = sl.FullChanceMCCFR(ctx, decks, None, GD.CAP)
    opp.tables_set(keys, n_act, R, S)
    for n, cut in enumerate((3, 0)):
        h.reset()
        h.cut(cut)
        h.respond_traverse(opp, resp, resp, 0, 0, 1)
        got, _ = assert_response_delta(h, rows, resp, f"deal on 2 decks, responder {resp}, cut {cut}")
        c = h.counters()
        assert (c["choice_visits"], c["terminal_visits"], c["dropped"], c["rows"]) == ((n + 1) * rows.choice, (n + 1) * rows.terminal, 0, got.shape[0])
    assert opp.counters()["rows"] == len(keys)


# ---- 8. sampled_exploitability ------------------------------------------------------------------------------------------------------------------------------------
def test_sampled_exploitability(ctx, sl, oracle):
    from scopa_amd.algorithms import FullChanceMCCFRTrainer
    from scopa_amd.algorithms.full_chance import sampled_exploitability
    decks, acts, _ = deck_set(oracle, 42, 4)
    ctx.mccfr_seed(SEED)
    t = FullChanceMCCFRTrainer(decks=decks, root_actions=acts, capacity_log2=13, batch=8, ctx=ctx)
    t.train(4)
    before = t.solver.tables_get()
    n = 1 << 14                                                           # ceil(n / 2) is a multiple of the 4 decks: the match's law is the exact target's
    rep = sampled_exploitability(t, 20, n, batch=16)
    assert rep["lower_bound"] is True and rep["episodes"] == n
    e = t.exploitability()
    print("sampled", rep["reward"], "+-", rep["std_error"], "exact value of the response", rep["exact_reward"], "+-", rep["exact_std_error"], "by seat",
          [s["reward"] for s in rep["by_seat"]], rep["exact_by_seat"], "exploitability", e)
    assert abs(rep["reward"] - rep["exact_reward"]) <= 5.0 * rep["exact_std_error"]
    for s in rep["by_seat"]:
        assert abs(s["reward"] - s["exact_reward"]) <= 5.0 * s["exact_std_error"]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, t.solver.tables_get()))
    assert t.sampled_exploitability(1, 64, batch=1)["lower_bound"] is True
    # the response trainer itself: a pure policy on the trainer's root, held-out decks allowed
    r = t.sampled_response(3, batch=4, sample=2, seed=1, current=True, capacity_log2=12, decks=G.held_out(oracle))
    S = r.tables()["strategy"]
    assert r.counters()["iterations"] == 6 and len(S) and (S.sum(1) == 1.0).all() and ((S == 0.0) | (S == 1.0)).all()
    assert r.solver.capacity_log2 == 12 and r.decks.shape == (3, 40) and r.root_actions == t.root_actions
    r.close()
    t.close()
    # from the deal nothing exact exists
    deal = FullChanceMCCFRTrainer(decks=GD.deal3(oracle)[0][:2], capacity_log2=GD.CAP, batch=1, ctx=ctx)
    deal.train(1)
    rep = sampled_exploitability(deal, 1, 256)
    assert rep["lower_bound"] is True and rep["exact_reward"] is None and rep["exact_by_seat"] is None and rep["exact_std_error"] is None
    assert all(s["exact_reward"] is None for s in rep["by_seat"]) and abs(rep["reward"]) <= 21
    deal.close()


def test_deep_cfr_sampled_exploitability_outside_the_sweeps_raises(sl, oracle):
    """nets on the deal's root (frontier traversal): no store of their policy fits, and the call says so with policy_store's own ValueError"""
    from scopa_amd.algorithms.deep_cfr import FullChanceDeepCFR
    d = FullChanceDeepCFR(GD.deal3(oracle)[0][:2], root_actions=(), traversal="frontier", batch=1, decks_per_iteration=1, seed=SEED)
    try:
        with pytest.raises(ValueError, match="exact sweeps cover at most 4 rounds"):
            d.sampled_exploitability(1, 64)
    finally:
        d.close()


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx, sl, oracle):
    h, _, _ = solver_of(ctx, sl, oracle, 42, 4)
    opp, _, _ = solver_of(ctx, sl, oracle, 42, 4)
    other_ctx = sl.Context(0)
    far, _, _ = solver_of(other_ctx, sl, oracle, 42, 4)
    ctx.mccfr_seed(SEED)
    bad = [lambda: h.respond_traverse(h, 0, 0, 0, 0, 1), lambda: h.respond_iterate(h, 0, 1, 1),              # h_opp == h_resp
           lambda: h.respond_traverse(far, 0, 0, 0, 0, 1), lambda: h.respond_iterate(far, 0, 1, 1),          # another context
           lambda: h.respond_traverse(opp, 2, 0, 0, 0, 1), lambda: h.respond_iterate(opp, -1, 1, 1),         # which outside {0, 1}
           lambda: h.respond_traverse(None, 2, 0, 0, 0, 1),
           lambda: h.respond_traverse(opp, 0, 2, 0, 0, 1),                                                   # responder outside {0, 1}
           lambda: h.respond_traverse(opp, 0, 0, 0, 0, 1, [0, 2, 2]), lambda: h.respond_traverse(opp, 0, 0, 0, 0, 1, [0, 4]),
           lambda: h.respond_iterate(opp, 0, 1, 2, lists=[[0, 1], [2, 2]]), lambda: h.respond_iterate(opp, 0, 0, 1)]
    for call in bad:
        with pytest.raises(sl.ScopaError) as e:
            call()
        assert e.value.status == sl.SCOPA_EINVAL
    c = h.counters()
    assert (c["rows"], c["choice_visits"], c["iterations"]) == (0, 0, 0)  # nothing launched
    far.close()
    other_ctx.close()
    # a too-small response store (the model is test_too_small_store_under_traversal: rows are dropped and counted, nothing faults)
    r0, nb = 3, 4
    rows = X.Rows()
    decks, _, st = deck_set(oracle, 42, r0)
    Q.traverse(st, decks, 0, 0, 0, nb, SEED, rows)
    want = dict(zip([tuple(k) for k in rows.arrays("count")[0].tolist()], rows.arrays("count")[1].tolist()))
    assert len(want) > (1 << 8)
    small, _, _ = solver_of(ctx, sl, oracle, 42, r0, capacity_log2=8)
    with pytest.raises(sl.ScopaError) as e:
        small.respond_traverse(None, 0, 0, 0, 0, nb)
    assert e.value.status == sl.SCOPA_ENOMEM
    c = small.counters()                                                  # the process goes on
    assert c["dropped"] > 0 and c["rows"] <= (1 << 8) and c["choice_visits"] == rows.choice
    keys, counts, _, dS = small.delta_get()
    assert keys.shape[0] == c["rows"] and not dS.any()
    for k, n in zip(keys.tolist(), counts.tolist()):
        assert n <= want[tuple(k)]                                        # (a pair the restatement never met is a KeyError)
    assert counts.sum() + c["dropped"] == sum(want.values())              # every visit of a responder's node either updated its row or was dropped
    small.harden()
    assert small.counters()["rows"] == c["rows"]
