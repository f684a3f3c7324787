"""GPU checks of the FullScopa sampling solver (scopa_amd/csrc/scopa_full_mccfr.hip) against the restatement tests/full_mccfr_ref.py, which
tests/test_full_mccfr_ref.py holds to the reference's infoset strings, to the shape counts and to exact enumeration.

Exact on the device: the key set, the visit counts, the counters, and d_strategy (every add into one cell of a launch is the same number, sigma of a
frozen row, so the sum does not depend on the order).  A d_regret row the launch meets once is bit-identical; a row met more than once is a sum of
float64 atomics in arrival order and is held to the project's reorder budget (oracle/mccfr_edges.py, as tests/test_gpu_team_mccfr.py::in_budget):
|R_gpu - R_ref| <= K_REORDER * eps * A_row + 2 * eps * |R_ref|, A_row = the sum of |increment| the restatement added into the row."""
import numpy as np
import pytest

import full_mccfr_ref as F
import mccfr_edges as E
import philox_words as W

pytestmark = pytest.mark.gpu

SEED = 0x5C09A
DECK_SEEDS = (42, 7)
_ROOTS, _REF = {}, {}


def root_of(oracle, deck_seed, r0):
    """(deck, actions, oracle state) of a fixed root at the start of round r0: random play under the first RandomState seed whose root gives a first
    traversal (traverser 0, id 0, iteration 0) that meets a key more than once, so the atomics of one row are exercised even at nb = 1"""
    if (deck_seed, r0) not in _ROOTS:
        deck = oracle.full_deal_py_seed(deck_seed)
        for k in range(40):
            st, acts = F.random_root(deck, r0, np.random.RandomState(1000 * r0 + k))
            rows = F.Rows()
            F.walk(st, 0, 0, 0, SEED, rows)
            if max(rows.count.values()) > 1:
                break
        else:
            raise AssertionError("no root whose first traversal meets a key twice")
        _ROOTS[deck_seed, r0] = (deck, acts, st)
    return _ROOTS[deck_seed, r0]


def solver_of(ctx, sl, oracle, deck_seed, r0, capacity_log2=14, seed=SEED):
    deck, acts, st = root_of(oracle, deck_seed, r0)
    ps = sl.FullState(deck=deck)
    for a in acts:
        ps.step(a)
    ctx.mccfr_seed(seed)
    return sl.FullMCCFR(ctx, deck, ps.s, capacity_log2), st


def ref_delta(oracle, deck_seed, r0, trav, iteration, b0, nb, seed):
    """the restatement's increments of one launch from zero tables, computed once: Rows (read only)"""
    key = (deck_seed, r0, trav, iteration, b0, nb, seed)
    if key not in _REF:
        rows = F.Rows()
        F.traverse(root_of(oracle, deck_seed, r0)[2], trav, iteration, b0, nb, seed, rows)
        _REF[key] = rows
    return _REF[key]


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def in_budget(R_gpu, R_ref, A, what):
    bound = (E.K_REORDER * E.EPS * A.sum(1))[:, None] + 2.0 * E.EPS * np.abs(R_ref)
    err = np.abs(R_gpu - R_ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = np.where(err == 0.0, 0.0, err / bound).max() if err.size else 0.0
    print(what, "largest regret error / budget:", worst)
    return bool((err <= bound).all())


def assert_delta(h, rows, what):
    """the device's increments against the restatement's: keys, counts, d_strategy exact; d_regret bit-identical on rows met once, else in the budget"""
    keys, counts, dR, dS = h.delta_get()
    k_ref, c_ref = rows.arrays("count")
    assert np.array_equal(keys, k_ref), f"{what}: key sets differ ({keys.size} rows against {k_ref.size})"
    assert np.array_equal(counts, c_ref), what
    assert same_bits(dS, rows.arrays("dS")[1]), f"{what}: d_strategy differs"
    want, A = rows.arrays("dR")[1], rows.arrays("A")[1]
    once = c_ref == 1
    assert same_bits(dR[once], want[once]), f"{what}: a d_regret row met once differs"
    assert in_budget(dR, want, A, what), what
    assert [F.key_actions(k) for k in keys] == list(h.tables_get()[1])
    return keys, counts


# ---- 1. one traversal --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cut", [0, -1])
@pytest.mark.parametrize("trav", [0, 1])
@pytest.mark.parametrize("r0", [4, 3])
@pytest.mark.parametrize("deck_seed", DECK_SEEDS)
def test_one_traversal_vs_restatement(ctx, sl, oracle, deck_seed, r0, trav, cut):
    h, _ = solver_of(ctx, sl, oracle, deck_seed, r0)
    h.cut(cut)
    rows = ref_delta(oracle, deck_seed, r0, trav, 0, 0, 1, SEED)
    h.traverse(trav, 0, 0, 1)
    _, counts = assert_delta(h, rows, f"deck {deck_seed}, round {r0}, traverser {trav}, cut {cut}")
    assert trav == 1 or counts.max() > 1                                  # the root was chosen for it
    c = h.counters()
    assert (c["choice_visits"], c["terminal_visits"]) == (F.shape_counts(r0)[trav], F.shape_counts(r0)[2]) == (rows.choice, rows.terminal)
    assert (c["rows"], c["dropped"], c["iterations"]) == (counts.size, 0, 0) and counts.sum() == c["choice_visits"]
    R, S = h.tables_get()[2:]
    assert not R.any() and not S.any()                                    # traverse writes increments only


# ---- 2. batches, wide words, every cut ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r0,nb,trav,deck_seed", [(3, 64, 0, 42), (3, 257, 1, 7), (2, 64, 1, 7)])
def test_batch_at_wide_words_by_every_cut(ctx, sl, oracle, r0, nb, trav, deck_seed):
    """nonzero b0 (the last one accepted: ids up to 2^32 - 1), iteration bit 31, both key words: counts exact by every cut, sums in the budget"""
    seed, iteration, b0 = W.WIDE_SEED, W.ITER_B31, (1 << 32) - nb
    rows = ref_delta(oracle, deck_seed, r0, trav, iteration, b0, nb, seed)
    assert rows.choice == nb * F.shape_counts(r0)[trav]
    h, _ = solver_of(ctx, sl, oracle, deck_seed, r0, capacity_log2=16, seed=seed)
    with pytest.raises(sl.ScopaError) as e:
        h.traverse(trav, iteration, b0 + 1, nb)                           # b0 + nb overflows
    assert e.value.status == sl.SCOPA_EINVAL and h.counters()["rows"] == 0
    with pytest.raises(sl.ScopaError):
        h.cut(min(3, 6 - r0) + 1)
    for n, cut in enumerate([-1] + list(range(0, min(3, 6 - r0) + 1))):
        h.reset()
        h.cut(cut)
        h.traverse(trav, iteration, b0, nb)
        assert_delta(h, rows, f"round {r0}, nb {nb}, cut {cut}")
        c = h.counters()
        assert (c["choice_visits"], c["terminal_visits"], c["dropped"]) == ((n + 1) * rows.choice, (n + 1) * rows.terminal, 0)


def test_words_separate(oracle):
    """CPU guard of the wide words above: with the seed, the iteration or b0 narrowed the restatement's visit counts differ, so the exact comparison
    of counts would catch a kernel that lost part of a word"""
    r0, nb, trav, deck_seed = 3, 64, 0, 42
    seed, iteration, b0 = W.WIDE_SEED, W.ITER_B31, (1 << 32) - nb
    want = ref_delta(oracle, deck_seed, r0, trav, iteration, b0, nb, seed).arrays("count")
    root = root_of(oracle, deck_seed, r0)[2]
    for what, s2, it2, ids in W.narrowed(seed, iteration, b0, nb):
        rows = F.Rows()
        for t in ids[:8]:
            F.walk(root, trav, t, it2, s2, rows)
        full = F.Rows()
        for t in W.ids_of(b0, nb)[:8]:
            F.walk(root, trav, t, iteration, seed, full)
        got, ref = rows.arrays("count"), full.arrays("count")
        assert not (np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])), what
    assert want[0].size > 0


# ---- 3. planted tables, apply, two iterations ----------------------------------------------------------------------------------------------------
def planted(oracle, deck_seed=42, r0=4):
    """keys of the restatement's first traversals and edge rows for them: the root (3 cards) with ONE positive regret, a 3-card row of the other
    player with negatives only (uniform sigma), a 2-card row with two positives, and strategy rows with a zero sum, a one-hot row, a mixed row"""
    root = root_of(oracle, deck_seed, r0)[2]
    seen = F.Rows()
    for trav in range(2):
        F.traverse(root, trav, 0, 0, 4, SEED, seen)
    keys = sorted(seen.count)
    k_root = F.key_of(root, 0)
    k_neg = next(k for k in keys if (k >> 62) & 1 == 1 and F.key_actions(k) == 3)
    k_two = next(k for k in keys if (k >> 62) & 1 == 0 and F.key_actions(k) == 2)
    k_one = next(k for k in keys if (k >> 62) & 1 == 1 and F.key_actions(k) == 2)
    K = np.array([k_root, k_neg, k_two, k_one], np.uint64)
    R = np.array([[0.0, 2.5, -1.0], [-1.0, -2.0, -0.5], [3.0, 1.0, 0.0], [0.0, 0.0, 0.0]])
    S = np.array([[0.25, 0.5, 2.0], [0.0, 0.0, 0.0], [0.0, 4.0, 0.0], [1.0, 3.0, 0.0]])
    return root, K, np.array([3, 3, 2, 2], np.int32), R, S


def rows_from_device(h):
    keys, _, R, S = h.tables_get()
    rows = F.Rows()
    rows.plant(keys, R, S)
    return rows


def assert_tables(h, rows, A, what):
    keys, n_act, R, S = h.tables_get()
    k_ref, R_ref = rows.arrays("R")
    assert np.array_equal(keys, k_ref), what
    assert same_bits(S, rows.arrays("S")[1]), f"{what}: strategy differs"
    A_rows = np.array([A.get(int(k), [0.0] * 3) for k in keys]).reshape(-1, 3)
    assert in_budget(R, R_ref, A_rows, what), what
    _, counts, dR, dS = h.delta_get()
    assert not counts.any() and not dR.any() and not dS.any(), f"{what}: increments left after apply"


def test_planted_tables_apply_and_two_iterations(ctx, sl, oracle):
    root, K, n_act, R, S = planted(oracle)
    h, _ = solver_of(ctx, sl, oracle, 42, 4)
    for bad in ((K, [3, 3, 2, 3], R, S), (K & np.uint64((1 << 63) - 1), n_act, R, S), (np.array([K[0]] * 4, np.uint64), [3] * 4, R, S)):
        with pytest.raises(sl.ScopaError) as e:
            h.tables_set(*bad)
        assert e.value.status == sl.SCOPA_EINVAL and h.counters()["rows"] == 0
    h.tables_set(K, n_act, R, S)
    order = np.argsort(K)
    got = h.tables_get()
    assert np.array_equal(got[0], K[order]) and np.array_equal(got[1], n_act[order]) and same_bits(got[2], R[order]) and same_bits(got[3], S[order])
    # (a) batch 24, the default cut, two iterations as their four (traverse, apply) halves.  Each half is restated FROM THE DEVICE'S OWN TABLES: regrets
    # that differ in their last bits (arrival order of the half before) give sigmas that do, so only a common start makes strategy sums comparable bit for bit
    batch = 24
    probe = rows_from_device(h)
    F.traverse(root, 1, 0, 0, batch, SEED, probe)                        # the one-positive row: the opponent always plays its slot 1
    assert probe.dS[int(K[0])] == [0.0, float(batch), 0.0]
    for counter in range(4):
        rows = rows_from_device(h)
        F.traverse(root, counter & 1, counter, 0, batch, SEED, rows)
        A = dict(rows.A)
        rows.apply()
        h.traverse(counter & 1, counter, 0, batch)
        h.apply()
        assert_tables(h, rows, A, f"half {counter}")
        assert h.counters()["iterations"] == counter + 1
    c = h.counters()
    assert (c["choice_visits"], c["terminal_visits"], c["dropped"]) == (2 * batch * (13 + 8) * 7, 2 * 2 * batch * 36, 0)
    keys_stepwise = h.tables_get()[0]
    # (b) iterate itself, batch 1 at cut 0: ONE lane makes every add of a launch in the restatement's own depth-first order, so two whole iterations
    # (alternation, the iteration words 0..3 from the handle's counter) come out bit for bit with no common restart in between
    h2, _ = solver_of(ctx, sl, oracle, 42, 4)
    h2.cut(0)
    h2.tables_set(K, n_act, R, S)
    rows = F.Rows()
    rows.plant(K, R, S)
    counter = F.iterate(root, 1, SEED, rows, 0)
    counter = F.iterate(root, 1, SEED, rows, counter)
    h2.iterate(1, 2)
    assert h2.counters()["iterations"] == counter == 4
    keys, _, R2, S2 = h2.tables_get()
    assert np.array_equal(keys, rows.arrays("R")[0]) and same_bits(R2, rows.arrays("R")[1]) and same_bits(S2, rows.arrays("S")[1])
    assert not h2.delta_get()[1].any()
    # ... and at batch 24 by the default cut: the same launches as (a), so the same rows (the draws are the same unless a regret's last bits move a
    # uniform across a threshold) and the same counters
    h3, _ = solver_of(ctx, sl, oracle, 42, 4)
    h3.tables_set(K, n_act, R, S)
    h3.iterate(batch, 2)
    assert h3.counters() == c and np.array_equal(h3.tables_get()[0], keys_stepwise)


# ---- 4. the deal's root: exact invariants only ---------------------------------------------------------------------------------------------------
def test_full_root_invariants(ctx, sl):
    deck = sl.full_deal_py_seed(42)
    ctx.mccfr_seed(SEED)
    h = sl.FullMCCFR(ctx, deck, None, 20)
    visits, total = (121303, 74648), 0
    for trav in range(2):
        h.traverse(trav, trav, 0, 2)
        keys, counts, _, _ = h.delta_get()
        c = h.counters()
        assert counts.sum(dtype=np.uint64) == 2 * visits[trav] and c["rows"] == keys.size == np.unique(keys).size
        total += 2 * visits[trav]
        assert (c["choice_visits"], c["terminal_visits"], c["dropped"]) == (total, 2 * (trav + 1) * 46656, 0)
        h.apply()
    assert h.counters()["iterations"] == 2 and not h.delta_get()[1].any()
    h2 = sl.FullMCCFR(ctx, deck, None, 20)
    h2.iterate(2, 1)
    c = h2.counters()
    assert (c["choice_visits"], c["terminal_visits"], c["dropped"], c["iterations"]) == (2 * sum(visits), 2 * 2 * 46656, 0, 2)
    assert c["rows"] == h2.tables_get()[0].size


# ---- 5. a store that is too small ----------------------------------------------------------------------------------------------------------------
def test_overflow_is_an_error_not_a_hang(ctx, sl, oracle):
    r0, nb = 3, 8
    rows = ref_delta(oracle, 42, r0, 0, 0, 0, nb, SEED)
    want = dict(zip(*[x.tolist() for x in rows.arrays("count")]))
    assert len(want) > (1 << 8)
    h, _ = solver_of(ctx, sl, oracle, 42, r0, capacity_log2=8)
    with pytest.raises(sl.ScopaError) as e:
        h.traverse(0, 0, 0, nb)
    assert e.value.status == sl.SCOPA_ENOMEM
    c = h.counters()                                                      # the process goes on
    assert c["dropped"] > 0 and c["rows"] <= (1 << 8) and c["choice_visits"] == rows.choice
    keys, counts, _, _ = h.delta_get()
    assert keys.size == c["rows"]
    for k, n in zip(keys.tolist(), counts.tolist()):
        assert n <= want[k]                                               # (a key the restatement never met is a KeyError)
    assert counts.sum() + c["dropped"] == rows.choice                     # every choice visit either updated its row or was dropped
    h.reset()
    try:
        h.traverse(1, 0, 0, 1)                                            # up to 344 rows may not fit 256 slots either: the call returns either way
    except sl.ScopaError as e2:
        assert e2.status == sl.SCOPA_ENOMEM
    assert h.counters()["choice_visits"] == rows.choice + F.shape_counts(r0)[1]


def test_overflowing_traversal_reports_each_time(ctx, sl, oracle):
    h, _ = solver_of(ctx, sl, oracle, 7, 3, capacity_log2=6)
    for _ in range(2):
        with pytest.raises(sl.ScopaError) as e:
            h.traverse(0, 0, 0, 4)
        assert e.value.status == sl.SCOPA_ENOMEM
    h.apply()                                                             # an apply on a full store is an ordinary launch
    assert h.counters()["rows"] == 1 << 6


# ---- 6. the match ----------------------------------------------------------------------------------------------------------------------------------
def test_match_vs_restatement_and_exact_value(ctx, sl, oracle):
    root, K, n_act, R, S = planted(oracle)
    h, _ = solver_of(ctx, sl, oracle, 42, 4, seed=W.WIDE_SEED)
    h.tables_set(K, n_act, R, S)
    table = {int(k): [float(x) for x in s] for k, s in zip(K, S)}
    n, stream = 4096, 5
    sums, r2 = h.match(n, stream, per_episode=True)
    want_sums, want_r2 = F.match(root, table, n, W.WIDE_SEED, stream)
    assert np.array_equal(r2, want_r2) and np.array_equal(sums, want_sums)
    assert np.array_equal(h.match(n, stream), sums) and not np.array_equal(h.match(n, stream + 1), sums)
    exact = 0.5 * (F.exact_match_value(root, table, 0) + F.exact_match_value(root, table, 1))
    rewards = r2.astype(np.float64) / 2.0
    se = rewards.std(ddof=1) / np.sqrt(n)
    print("match mean", rewards.mean(), "exact", exact, "se", se)
    assert abs(rewards.mean() - exact) <= 5.0 * se
    assert h.counters()["rows"] == 4                                      # the match never inserts
    assert not h.match(0).any()


# ---- 7. the Python trainer -------------------------------------------------------------------------------------------------------------------------
def test_trainer_save_load_info_sets_and_separate_handles(ctx, sl, oracle, tmp_path):
    from scopa_amd.algorithms import FullMCCFRTrainer
    from scopa_amd.envs import load_game
    deck, acts, st = root_of(oracle, 42, 4)
    ctx.mccfr_seed(SEED)
    a = FullMCCFRTrainer(seed=42, root_actions=acts, capacity_log2=12, batch=16, ctx=ctx)
    b = FullMCCFRTrainer(seed=42, root_actions=acts, capacity_log2=13, batch=16, ctx=ctx)
    a.train(2)
    assert a.counters()["iterations"] == 4 and b.counters() == dict(choice_visits=0, terminal_visits=0, rows=0, dropped=0, iterations=0)
    t = a.tables()
    assert t["keys"].size == a.counters()["rows"] > 50 and np.all(np.diff(t["keys"].astype(object)) > 0)
    path = str(tmp_path / "full.npz")
    a.save(path)
    b.load(path)
    u = b.tables()
    assert np.array_equal(t["keys"], u["keys"]) and np.array_equal(t["n_act"], u["n_act"]) and same_bits(t["regret"], u["regret"]) and same_bits(t["strategy"], u["strategy"])
    a.iteration()
    assert same_bits(b.solver.tables_get()[3], u["strategy"]) and not same_bits(a.tables()["strategy"][:u["keys"].size], u["strategy"])
    # info_sets: the decoded strings are the states' own, along random play from the root
    state = load_game("full_scopa").new_initial_state()
    for x in acts:
        state.apply_action(x)
    info, rng, found = b.info_sets, np.random.RandomState(3), 0
    assert len(info) == u["keys"].size
    root_key = (0, state.information_state_string(0))
    assert root_key in info and list(info[root_key].legal_actions) == state.legal_actions()
    for _ in range(50):
        s = state.clone()
        while not s.is_terminal():
            p, legal = s.current_player(), s.legal_actions()
            node = info.get((p, s.information_state_string(p)))
            if len(legal) > 1 and node is not None:
                found += 1
                assert list(node.legal_actions) == legal
                probs = b.average_policy(s)
                total = node.strategy_sum.sum()
                want = node.strategy_sum / total if total > 1e-12 else np.full(len(legal), 1.0 / len(legal))
                assert list(probs) == legal and np.array_equal(np.array(list(probs.values())), want)
            s.apply_action(legal[rng.randint(len(legal))])
    assert found > 100
    strings = {F.key_to_string(k, deck) for k in u["keys"].tolist()}
    assert strings == {k[1] for k in info}
    mean, se, scopas = b.evaluate_vs_random(2048)
    assert abs(mean) <= 21 and se > 0 and scopas["data_collected"] and scopas["difference"] == scopas["trained_avg"] - scopas["opponent_avg"]
    tiny = FullMCCFRTrainer(seed=42, root_actions=acts[:18], capacity_log2=5, batch=4, ctx=ctx)
    with pytest.raises(RuntimeError, match="dropped"):
        tiny.train(1)
    with pytest.raises(ValueError):
        FullMCCFRTrainer(seed=42, root_actions=acts[:5], ctx=ctx)
    for x in (tiny, a, b):
        x.close()
