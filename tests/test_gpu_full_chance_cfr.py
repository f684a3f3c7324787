"""GPU checks of the exact weighted CFR iteration of FullScopa across a set of decks (scopa_amd/csrc/scopa_full_chance_cfr.hip:
scopa_full_chance_cfr_iterate) against the restatement tests/full_chance_cfr_ref.py, which tests/test_full_chance_cfr_ref.py holds to a depth-first
recursive CFR per deck, to the exploitability restatement's value pass, to cfr_variants_ref's weighting rule and to the best response at R = 1.

Every sum of the device code has one order, the restatement's, so everything is compared on bits: the pair set, every regret and strategy word
(the unused third slot included) and every sweep value.  Shapes, as the exploitability suite's: R = 1 on 3 decks (a root level of 3 lanes), R = 2 on
5 decks (no level size a multiple of 256) and R = 3 on 2 decks (segments longer than a wavefront, pairs whose segments add nodes of both decks)."""
import numpy as np
import pytest

import full_chance_cfr_ref as CFR
import full_chance_exploit_ref as X
import full_chance_ref as W
import full_mccfr_ref as F

pytestmark = pytest.mark.gpu

SEED = 0x5C09A
SHAPES = {1: (5, 3, None), 2: (4, 5, 0), 3: (3, 2, 0)}      # R -> (round of the root, decks, the seat whose root hand the packet fixes)
VARIANTS = {"vanilla": {}, "cfr+": {}, "linear": {}, "dcfr": dict(alpha=1.5, beta=0.0, gamma=2.0)}
_SETS, _TREES, _REFS = {}, {}, {}


# ---- helpers (copies of tests/test_gpu_full_chance_exploit.py's, which stays as it is) ------------------------------------------------------------
def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def packet(oracle, r0, n, fix_seat, deck_seed=42, shared_rounds=None):
    """(decks [n][40], actions to the root, oracle root state): n decks that share deck `deck_seed`'s first `shared_rounds` rounds (default r0) below a
    fixed random root at the start of round r0 of that deck"""
    from scopa_amd.algorithms import packet_decks
    key = (r0, n, fix_seat, deck_seed, shared_rounds)
    if key not in _SETS:
        deck = oracle.full_deal_py_seed(deck_seed)
        st, acts = F.random_root(deck, r0, np.random.RandomState(100 * r0 + deck_seed))
        _SETS[key] = (packet_decks(deck, r0 if shared_rounds is None else shared_rounds, n, 5, fix_seat=fix_seat), acts, st)
    return _SETS[key]


def shape(oracle, R):
    r0, n, fix_seat = SHAPES[R]
    return packet(oracle, r0, n, fix_seat)


def tree_of(st, decks, R):
    """the restatement's forest, expanded once per (root, decks)"""
    key = (bytes(st.s), np.ascontiguousarray(decks, np.uint8).tobytes())
    if key not in _TREES:
        _TREES[key] = X.tree_of(st, decks, R)
    return _TREES[key]


def state_of(sl, deck, acts):
    ps = sl.FullState(deck=deck)
    for a in acts:
        ps.step(a)
    return ps.s


def solver_of(ctx, sl, oracle, R, capacity_log2=16):
    decks, acts, st = shape(oracle, R)
    ctx.mccfr_seed(SEED)
    return sl.FullChanceMCCFR(ctx, decks, state_of(sl, decks[0], acts), capacity_log2), tree_of(st, decks, R), decks


def out4_of(e):
    return np.array([e["exploitability"], e["br0"], e["br1"], e["value"]])


def tables_of(h):
    keys, _, R, S = h.tables_get()
    return X.table_of(keys, R), X.table_of(keys, S)


def level_pairs(tree):
    return sorted(set(k for _, n, ks in tree[0] if n > 1 for k in ks))


def plant(h, table_R, table_S):
    keys = sorted(set(table_R) | set(table_S))
    n_act = np.array([W.key_actions(k) for k in keys], np.int32)
    R = np.array([table_R.get(k, [0.0] * 3) for k in keys]).reshape(-1, 3)
    S = np.array([table_S.get(k, [0.0] * 3) for k in keys]).reshape(-1, 3)
    h.tables_set(np.array(keys, np.uint64).reshape(-1, 2), n_act, R, S)


def raises(sl, status, fn, *args):
    with pytest.raises(sl.ScopaError) as e:
        fn(*args)
    assert e.value.status == status, e.value


# ---- helpers of this file ---------------------------------------------------------------------------------------------------------------------------
def weights_of(variant, t0, n):
    from scopa_amd.algorithms import schedule
    return schedule(variant, t0, n, **VARIANTS[variant])


def ref_of(tree, tR, tS, weights, alternating, key=None):
    """the restatement's (R, S, values) from tables tR, tS; computed once where a key is given, and left unchanged"""
    if key is None:
        return CFR.iterate(tree, tR, tS, weights, alternating)
    if key not in _REFS:
        _REFS[key] = CFR.iterate(tree, tR, tS, weights, alternating)
    return _REFS[key]


def assert_tables(h, R_ref, S_ref, what):
    """the device's tables against the restatement's: the pair set and every word of the regret and strategy rows, on bits"""
    keys, n_act, R, S = h.tables_get()
    k_ref = sorted(R_ref)
    assert sorted(S_ref) == k_ref
    assert keys.shape == (len(k_ref), 2) and keys.tolist() == [list(k) for k in k_ref], f"{what}: pair sets differ ({keys.shape[0]} rows against {len(k_ref)})"
    assert n_act.tolist() == [W.key_actions(k) for k in k_ref]
    assert same_bits(R, np.array([R_ref[k] for k in k_ref]).reshape(-1, 3)), f"{what}: regret rows differ"
    assert same_bits(S, np.array([S_ref[k] for k in k_ref]).reshape(-1, 3)), f"{what}: strategy rows differ"


def step_and_check(h, tree, n_iters, weights, alternating, what, root=None):
    """one cfr_iterate call checked against the restatement fed with tables_get taken just before it -> the values"""
    tR, tS = tables_of(h)
    values = h.cfr_iterate(n_iters, weights, alternating, root)
    R_ref, S_ref, v_ref = ref_of(tree, tR, tS, np.ones((n_iters, 3)) if weights is None else weights, alternating)
    assert same_bits(values, v_ref), f"{what}: sweep values {values} against {v_ref}"
    assert_tables(h, R_ref, S_ref, what)
    return values


def planted_tables(tree, kind="mixed"):
    """regret and strategy tables over the forest's pairs.  mixed: one-hot rows, rows with negative, exactly-zero and -0.0 cells, rows that are absent
    and full rows, chosen by the pair's bits; hot: every row one-hot (most histories then have w = 0); first_hand: of the pairs that share word A
    only the one with the lowest hand word (the others are claimed past a slot that holds their word A)"""
    pairs = level_pairs(tree)
    R, S = {}, {}
    if kind == "first_hand":
        first = {}
        for k in pairs:
            first.setdefault(k[0], k)
        kept = sorted(first.values())
        assert len(kept) < len(pairs)
        rows_R, rows_S = W.rows_for(np.array(kept, np.uint64))
        for k, r, s in zip(kept, rows_R, rows_S):
            R[k], S[k] = [float(x) - 40.0 if x > 60.0 else float(x) for x in r], [float(x) for x in s]
            R[k] = [x if a < W.key_actions(k) else 0.0 for a, x in enumerate(R[k])]
        return R, S
    full_R, full_S = W.rows_for(np.array(pairs, np.uint64))
    for i, k in enumerate(pairs):
        n = W.key_actions(k)
        sel = 0 if kind == "hot" else ((k[0] >> 16) ^ k[1] ^ (k[1] >> 7)) % 5
        if sel == 0:
            row = [0.0] * 3
            row[((k[0] >> 16) ^ k[1]) % n] = 2.5
            R[k], S[k] = row, list(row)
        elif sel == 1:
            R[k], S[k] = [-1.5, 0.0, 3.0 if n == 3 else 0.0], [0.5, 0.25, 1.0 if n == 3 else 0.0]
        elif sel == 2:
            R[k], S[k] = [-0.0, -2.0, 0.0], [0.0, 0.0, 0.0]
        elif sel == 4:
            R[k], S[k] = [float(x) for x in full_R[i]], [float(x) for x in full_S[i]]
    return R, S


# ---- 1. from the empty store: every variant, alternating and simultaneous ---------------------------------------------------------------------------
CASES = [(R, v, alt, 3) for R in (1, 2) for v in VARIANTS for alt in (1, 0)] + [(3, "dcfr", 1, 2), (3, "vanilla", 0, 2)]


@pytest.mark.parametrize("R,variant,alternating,n_iters", CASES)
def test_empty_store_vs_restatement(ctx, sl, oracle, R, variant, alternating, n_iters):
    h, tree, decks = solver_of(ctx, sl, oracle, R, capacity_log2=18 if R == 3 else 14)
    w = weights_of(variant, 0, n_iters)
    R_ref, S_ref, v_ref = ref_of(tree, {}, {}, w, alternating, key=(R, variant, alternating, n_iters))
    values = h.cfr_iterate(n_iters, None if variant == "vanilla" else w, alternating)
    assert same_bits(values, v_ref), (values, v_ref)
    assert_tables(h, R_ref, S_ref, f"R {R}, {variant}, alternating {alternating}")
    c = h.counters()
    assert (c["rows"], c["dropped"], c["iterations"], c["choice_visits"], c["terminal_visits"]) == (len(level_pairs(tree)), 0, 2 * n_iters, 0, 0)
    assert any(min(r) < 0.0 for r in R_ref.values()) or variant == "cfr+"
    first = h.tables_get()
    h2, _, _ = solver_of(ctx, sl, oracle, R, capacity_log2=18 if R == 3 else 14)              # a second run: identical bits
    assert same_bits(h2.cfr_iterate(n_iters, w, alternating), values)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(first, h2.tables_get()))
    sizes = [len(ks) for _, n, ks in tree[0] if n > 1]
    assert sizes[:4] == [len(decks) * m for m in (1, 3, 9, 18)] and len(tree[1]) == len(decks) * 36 ** R
    assert R != 2 or all(m % 256 for m in sizes)
    if R == 3:
        counts, spans = {}, {}
        for d, (_, n, ks) in enumerate(tree[0]):
            for g, k in enumerate(ks or ()):
                counts[k] = counts.get(k, 0) + 1
                spans.setdefault(k, set()).add(X.deck_of(tree, d, g))
        assert max(counts.values()) > 64                                            # a pair's segment longer than a wavefront
        assert any(len(v) == 2 for v in spans.values())                             # pairs whose segments add nodes of both decks


# ---- 2. from a trained store and from planted tables ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 2])
@pytest.mark.parametrize("alternating", [1, 0])
def test_trained_store_vs_restatement(ctx, sl, oracle, R, alternating):
    h, tree, _ = solver_of(ctx, sl, oracle, R)
    h.iterate(16, 3)
    before = h.exploitability(None, 1)["value"]
    values = step_and_check(h, tree, 3, weights_of("dcfr", 0, 3), alternating, f"trained store, R {R}")
    assert same_bits(values[0, 0], before)                                          # the first sweep IS the value pass of the current sigma
    tR, tS = tables_of(h)
    for which in (0, 1):
        assert same_bits(out4_of(h.exploitability(None, which)), X.solve(tree, tR, tS, which)["out4"])
    assert h.counters()["iterations"] == 6 + 6


@pytest.mark.parametrize("kind", ["mixed", "hot", "first_hand"])
@pytest.mark.parametrize("neg", [0.0, 0.5])
def test_planted_tables_vs_restatement(ctx, sl, oracle, kind, neg):
    h, tree, _ = solver_of(ctx, sl, oracle, 2)
    R0, S0 = planted_tables(tree, kind)
    plant(h, R0, S0)
    n_planted = h.counters()["rows"]
    assert n_planted == len(set(R0) | set(S0)) and (kind == "hot") == (n_planted == len(level_pairs(tree)))
    w = np.array([[1.0, neg, 0.5], [0.75, neg, 1.0], [1.0, neg, 0.0]])
    before = h.exploitability(None, 1)["value"]
    values = step_and_check(h, tree, 3, w, 1, f"planted {kind}, neg {neg}")
    assert same_bits(values[0, 0], before) and h.counters()["rows"] == len(level_pairs(tree))
    if kind == "hot":                                                               # rows no history with w > 0 holds: dS = 0, still discounted
        R1, S1, _ = CFR.iterate(tree, R0, S0, w[:1], 1)
        assert any(S1[k] == [0.5 * x for x in S0[k]] and R1[k] == R0[k] for k in R0)
    if kind == "mixed":
        assert any(min(r) < 0.0 for r in R0.values()) and any(0.0 in r[:W.key_actions(k)] for k, r in R0.items())
    if kind == "first_hand":
        held = {k[0] for k in R0}
        assert any(k[0] in held and k not in R0 for k in level_pairs(tree))
    tR, tS = tables_of(h)
    for which in (0, 1):
        assert same_bits(out4_of(h.exploitability(None, which)), X.solve(tree, tR, tS, which)["out4"])


# ---- 3. one call of 4 iterations is two calls of 2 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alternating", [1, 0])
def test_one_call_is_two_calls_with_the_weights_split(ctx, sl, oracle, alternating):
    a, tree, _ = solver_of(ctx, sl, oracle, 2)
    b, _, _ = solver_of(ctx, sl, oracle, 2)
    w = weights_of("dcfr", 0, 4)
    va = a.cfr_iterate(4, w, alternating)
    vb = np.concatenate([b.cfr_iterate(2, w[:2], alternating), b.cfr_iterate(2, w[2:], alternating)])
    assert same_bits(va, vb) and all(x.tobytes() == y.tobytes() for x, y in zip(a.tables_get(), b.tables_get()))
    assert a.counters() == b.counters() and a.counters()["iterations"] == 8
    R_ref, S_ref, v_ref = ref_of(tree, {}, {}, w, alternating)
    assert same_bits(va, v_ref)
    assert_tables(a, R_ref, S_ref, "4 iterations")


# ---- 4. nothing of a call's set-up outlives it ---------------------------------------------------------------------------------------------------------
def test_no_stale_state_across_calls(ctx, sl, oracle):
    """decks that share their first five rounds below a round-4 root (R = 2; the decks part in round 5), so that the round-5 boundary is another root
    every deck fits; each call is checked against the restatement fed with tables_get taken before it"""
    decks, acts5, st5 = packet(oracle, 5, 6, None)
    train, held = decks[:3], decks[3:]
    st4 = F.root_of(decks[0], acts5[:24])
    tree = tree_of(st4, train, 2)
    ctx.mccfr_seed(SEED)
    h = sl.FullChanceMCCFR(ctx, train, state_of(sl, decks[0], acts5[:24]), 14)
    w = weights_of("dcfr", 0, 10)
    step_and_check(h, tree, 2, w[:2], 1, "first call")
    tR, tS = tables_of(h)
    assert same_bits(out4_of(h.exploitability(None, 0, held)), X.solve(tree_of(st4, held, 2), tR, tS, 0)["out4"])       # held-out decks
    assert same_bits(out4_of(h.exploitability(state_of(sl, decks[0], acts5), 1)), X.solve(tree_of(st5, train, 1), tR, tS, 1)["out4"])   # another root
    step_and_check(h, tree, 2, w[2:4], 0, "after exploitability calls")
    h.reset()
    assert h.counters()["rows"] == 0
    step_and_check(h, tree, 2, w[4:6], 1, "after reset")
    R0, S0 = planted_tables(tree, "mixed")
    plant(h, R0, S0)
    step_and_check(h, tree, 2, w[6:8], 1, "after tables_set")
    it = h.counters()["iterations"]
    h.traverse(0, it, 0, 8)
    h.apply()
    step_and_check(h, tree, 2, w[8:], 1, "after traverse and apply")
    step_and_check(h, tree_of(st5, train, 1), 2, w[:2], 1, "another root", root=state_of(sl, decks[0], acts5))
    assert h.counters()["iterations"] == it + 1 + 8


def test_descendant_root_leaves_earlier_rounds_alone(ctx, sl, oracle):
    """a handle at the start of round 3 over decks that share their first five rounds, trained there, then solved on the round-5 descendant that every
    deck fits: rows of rounds below 5 keep their bits, and so do the increments and the counts"""
    decks, acts5, st5 = packet(oracle, 5, 3, None)
    ctx.mccfr_seed(SEED)
    h = sl.FullChanceMCCFR(ctx, decks, state_of(sl, decks[0], acts5[:18]), 18)
    h.iterate(8, 2)
    h.traverse(0, 4, 0, 8)                                                          # increments left unapplied
    keys0, n0, R0, S0 = h.tables_get()
    dk0, cnt0, dR0, dS0 = h.delta_get()
    c0 = h.counters()
    assert dR0.any() and cnt0.any() and np.array_equal(keys0, dk0)
    tree = tree_of(st5, decks, 1)
    pairs = set(level_pairs(tree))
    held = {tuple(k) for k in keys0.tolist()}
    assert len(pairs & held) > 3
    root = state_of(sl, decks[0], acts5)
    w = weights_of("dcfr", 0, 3)
    tR, tS = X.table_of(keys0, R0), X.table_of(keys0, S0)
    values = h.cfr_iterate(3, w, 1, root)
    R_ref, S_ref, v_ref = ref_of(tree, tR, tS, w, 1)
    assert same_bits(values, v_ref)
    assert_tables(h, R_ref, S_ref, "round-5 descendant")
    keys1, n1, R1, S1 = h.tables_get()
    dk1, cnt1, dR1, dS1 = h.delta_get()
    old = np.array([tuple(k) in held for k in keys1.tolist()])
    assert np.array_equal(keys1[old], keys0) and np.array_equal(dk1[old], dk0)
    early = ((keys0[:, 0] >> np.uint64(59)) & np.uint64(7)) < 5
    assert early.any() and same_bits(R1[old][early], R0[early]) and same_bits(S1[old][early], S0[early])
    assert any(R_ref[k] != tR.get(k, [0.0] * 3) for k in pairs)
    assert np.array_equal(cnt1[old], cnt0) and same_bits(dR1[old], dR0) and same_bits(dS1[old], dS0)
    assert not cnt1[~old].any() and not dR1[~old].any() and not dS1[~old].any()
    c1 = h.counters()
    assert (c1["choice_visits"], c1["terminal_visits"], c1["dropped"]) == (c0["choice_visits"], c0["terminal_visits"], 0)
    assert c1["rows"] == len(held | pairs) and c1["iterations"] == c0["iterations"] + 6


# ---- 5. a store too small for the forest's pairs ---------------------------------------------------------------------------------------------------
def test_full_store_returns_enomem_and_changes_no_row(ctx, sl, oracle):
    h, tree, _ = solver_of(ctx, sl, oracle, 2, capacity_log2=4)
    pairs = level_pairs(tree)[:6]
    R0 = {k: [1.5, -2.0, 0.25 if W.key_actions(k) == 3 else 0.0] for k in pairs}
    plant(h, R0, R0)
    before, c0 = tables_of(h), h.counters()
    assert len(before[0]) == 6
    raises(sl, sl.SCOPA_ENOMEM, h.cfr_iterate, 2, weights_of("dcfr", 0, 2))
    c1 = h.counters()
    assert c1["dropped"] > c0["dropped"] and c1["rows"] <= 16 and c1["iterations"] == c0["iterations"]
    after = tables_of(h)
    for k in pairs:
        assert same_bits(after[0][k], before[0][k]) and same_bits(after[1][k], before[1][k])
    assert all(not any(after[0][k]) and not any(after[1][k]) for k in after[0] if k not in before[0])                   # the rows claimed are zero rows
    for which in (0, 1):
        assert same_bits(out4_of(h.exploitability(None, which)), X.solve(tree, after[0], after[1], which)["out4"])


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx, sl, oracle):
    h, tree, decks = solver_of(ctx, sl, oracle, 1, capacity_log2=10)
    _, acts, _ = shape(oracle, 1)
    L = sl.lib()
    good = np.ones((2, 3))
    state = lambda: (tuple(x.tobytes() for x in h.tables_get()), h.counters())
    start = state()

    def raw(handle, root, n_iters, w, alternating):
        vals = np.zeros((max(n_iters, 1), 2))
        return L.scopa_full_chance_cfr_iterate(handle, sl._ptr(root), n_iters, sl._ptr(w), alternating, sl._ptr(vals))

    round1 = state_of(sl, decks[0], acts[:6])                                       # R = 5
    other = oracle.full_deal_py_seed(7)
    other5 = state_of(sl, other, F.random_root(other, 5, np.random.RandomState(3))[1])
    assert raw(None, None, 2, good, 1) == sl.SCOPA_EINVAL
    assert raw(h._h, None, -1, None, 1) == sl.SCOPA_EINVAL
    assert raw(h._h, None, (1 << 20) + 1, None, 1) == sl.SCOPA_EINVAL
    assert raw(h._h, None, 2, good, 2) == sl.SCOPA_EINVAL and raw(h._h, None, 2, good, -1) == sl.SCOPA_EINVAL
    for bad in (np.nan, 1.5, -0.25, np.inf):
        w = good.copy()
        w[1, 2] = bad
        assert raw(h._h, None, 2, w, 1) == sl.SCOPA_EINVAL
        assert raw(h._h, round1, 2, w, 1) == sl.SCOPA_EINVAL   # the weights come before the limits
    assert raw(h._h, state_of(sl, decks[0], acts[:-1]), 2, good, 1) == sl.SCOPA_EINVAL          # mid-round
    assert raw(h._h, round1, 2, good, 1) == sl.SCOPA_ELIMIT
    other1 = state_of(sl, other, F.random_root(other, 1, np.random.RandomState(3))[1])
    assert raw(h._h, other1, 2, good, 1) == sl.SCOPA_ELIMIT                         # the limits come before the decks
    assert raw(h._h, other5, 2, good, 1) == sl.SCOPA_EINVAL                         # a root the handle's decks do not fit
    assert raw(h._h, round1, 0, None, 1) == sl.SCOPA_ELIMIT                         # n_iters = 0 is checked like any call ...
    assert raw(h._h, None, 0, None, 1) == sl.SCOPA_OK and state() == start          # ... and then does nothing: no row claimed
    assert h.cfr_iterate(0).shape == (0, 2) and state() == start
    with pytest.raises(ValueError):
        h.cfr_iterate(2, np.ones((3, 3)))
    many, acts3, _ = packet(oracle, 3, 90, 0)                                       # 90 x 36^3 > 1 << 22: one deck over the cap
    ctx.mccfr_seed(SEED)
    big = sl.FullChanceMCCFR(ctx, many, state_of(sl, many[0], acts3), 10)
    raises(sl, sl.SCOPA_ELIMIT, big.cfr_iterate, 1)
    assert big.counters() == dict(choice_visits=0, terminal_visits=0, rows=0, dropped=0, iterations=0)
    assert state() == start
    step_and_check(h, tree, 2, None, 1, "a valid call after the refusals")          # weights = None: all 1.0


# ---- 7. the iteration counter, and MCCFR after the exact iterations -----------------------------------------------------------------------------------
def test_counter_advances_and_mccfr_goes_on_from_it(ctx, sl, oracle):
    h, tree, decks = solver_of(ctx, sl, oracle, 2)
    _, _, st = shape(oracle, 2)
    h.cfr_iterate(3, weights_of("cfr+", 0, 3), 0)
    assert h.counters()["iterations"] == 6
    h.cfr_iterate(2, weights_of("cfr+", 3, 2), 1)
    counter = h.counters()["iterations"]
    assert counter == 10
    keys0, _, R, S = h.tables_get()
    rows = W.Rows()
    rows.plant(keys0, R, S)
    rows.touch_all(keys0)                                                           # apply adds 0.0 into every row the store holds: a -0.0 cell becomes 0.0
    h.cut(0)
    for deck in (2, 1):                                                             # the existing suite's standard for iterate: batch 1 at cut 0, one deck listed, on bits
        counter = W.iterate(st, decks, 1, SEED, rows, counter, listed=[deck])
        h.iterate(1, 1, lists=[[deck]])
        assert h.counters()["iterations"] == counter
        keys, _, R2, S2 = h.tables_get()
        assert np.array_equal(keys, rows.arrays("R")[0]) and same_bits(R2, rows.arrays("R")[1]) and same_bits(S2, rows.arrays("S")[1])
    assert counter == 14
    fresh = W.Rows()
    fresh.plant(keys0, R, S)
    fresh.touch_all(keys0)
    assert W.iterate(st, decks, 1, SEED, fresh, 0, listed=[2]) == 2
    assert not same_bits(fresh.arrays("R")[1], rows.arrays("R")[1])                 # from counter 0 the draws, and so the tables, are others


# ---- 8. the Python trainer ---------------------------------------------------------------------------------------------------------------------------
def test_trainer_solve_cfr(ctx, sl, oracle):
    from scopa_amd.algorithms import FullChanceMCCFRTrainer, schedule
    decks, acts, st = shape(oracle, 2)
    tree = tree_of(st, decks, 2)
    ctx.mccfr_seed(SEED)
    a, b, c = [FullChanceMCCFRTrainer(decks=decks, root_actions=acts, capacity_log2=14, batch=1, ctx=ctx) for _ in range(3)]
    last = a.solve_cfr(6, variant="dcfr", exploitability_freq=3)
    want = []
    for t in (3, 6):
        v = b.solver.cfr_iterate(3, schedule("dcfr", t - 3, 3), True)
        e = b.solver.exploitability()
        want.append((t, e["exploitability"], e["br0"], e["br1"], e["value"]))
    assert a.cfr_records == want and len(want) == 2 and same_bits(last, v[-1])
    a.solve_cfr(6, variant="dcfr")                                                  # t continues over calls
    assert a.cfr_records == []
    v12 = c.solver.cfr_iterate(12, schedule("dcfr", 0, 12), True)
    ta, tc = a.tables(), c.tables()
    assert np.array_equal(ta["keys"], tc["keys"]) and same_bits(ta["regret"], tc["regret"]) and same_bits(ta["strategy"], tc["strategy"])
    assert a.counters() == c.counters() and a.counters()["iterations"] == 24
    R_ref, S_ref, v_ref = ref_of(tree, {}, {}, schedule("dcfr", 0, 12), True)
    assert same_bits(v12, v_ref)
    assert_tables(c.solver, R_ref, S_ref, "trainer, 12 iterations")
    assert same_bits(a.solve_cfr(1, variant="cfr+", alternating=False, root_actions=acts), c.solver.cfr_iterate(1, schedule("cfr+", 12, 1), False)[-1])
    with pytest.raises(ValueError):
        a.solve_cfr(2, variant="nope")
    with pytest.raises(ValueError):
        a.solve_cfr(2, exploitability_freq=0)
    for t in (a, b, c):
        t.close()
