"""GPU checks of FullScopa over a set of decks (scopa_amd/csrc/scopa_full_chance.hip) against the restatement tests/full_chance_ref.py, which
tests/test_full_chance_ref.py holds to the oracle's infoset strings, to exact enumeration summed over decks, and to the guards that each comparison
here separates a wrong kernel from a right one.

The standard is tests/test_gpu_full_mccfr.py's: key-pair set, visit counts, counters and d_strategy exact; a d_regret row met once bit-identical; the
rest within the reorder budget (in_budget, K_REORDER of oracle/mccfr_edges.py)."""
import numpy as np
import pytest

import full_chance_ref as X
import full_mccfr_ref as F
import philox_words as W
from test_gpu_full_mccfr import in_budget, root_of, same_bits

pytestmark = pytest.mark.gpu

SEED = 0x5C09A
DECK_SEEDS = (42, 7)
N_DECKS = 4
_REF, _SETS = {}, {}


def deck_set(oracle, deck_seed, r0, n=N_DECKS, fix_seat=0):
    """(decks [n][40], actions to the root, oracle root state): the packet of `n` decks seat `fix_seat` cannot tell apart below test_gpu_full_mccfr's
    root of (deck_seed, r0)"""
    from scopa_amd.algorithms import packet_decks
    key = (deck_seed, r0, n, fix_seat)
    if key not in _SETS:
        deck, acts, st = root_of(oracle, deck_seed, r0)
        _SETS[key] = (packet_decks(deck, r0, n, 5, fix_seat=fix_seat), acts, st)
    return _SETS[key]


def solver_of(ctx, sl, oracle, deck_seed, r0, capacity_log2=14, seed=SEED, n=N_DECKS, fix_seat=0):
    decks, acts, st = deck_set(oracle, deck_seed, r0, n, fix_seat)
    ps = sl.FullState(deck=decks[0])
    for a in acts:
        ps.step(a)
    ctx.mccfr_seed(seed)
    return sl.FullChanceMCCFR(ctx, decks, ps.s, capacity_log2), st, decks


def ref_delta(oracle, deck_seed, r0, trav, iteration, b0, nb, seed, listed=None, n=N_DECKS, fix_seat=0, **kw):
    """the restatement's increments of one launch from zero tables, computed once: Rows (read only)"""
    key = (deck_seed, r0, trav, iteration, b0, nb, seed, listed, n, fix_seat, tuple(sorted(kw.items())))
    if key not in _REF:
        decks, _, st = deck_set(oracle, deck_seed, r0, n, fix_seat)
        rows = X.Rows()
        X.traverse(st, decks, trav, iteration, b0, nb, seed, rows, listed, **kw)
        _REF[key] = rows
    return _REF[key]


def assert_delta(h, rows, what, hidden=()):
    """the device's increments against the restatement's: pairs, counts, d_strategy exact; d_regret bit-identical on rows met once, else in the budget.
    hidden: pairs the store holds beside the launch's (fillers), each of which must show no visit and no increment"""
    keys, counts, dR, dS = h.delta_get()
    if len(hidden):
        hid = {tuple(k) for k in np.asarray(hidden, np.uint64).reshape(-1, 2).tolist()}
        is_hid = np.array([tuple(k) in hid for k in keys.tolist()], bool)
        assert is_hid.sum() == len(hid) and not counts[is_hid].any() and not dR[is_hid].any() and not dS[is_hid].any(), what
        keys, counts, dR, dS = keys[~is_hid], counts[~is_hid], dR[~is_hid], dS[~is_hid]
    k_ref, c_ref = rows.arrays("count")
    assert keys.shape == k_ref.shape and np.array_equal(keys, k_ref), f"{what}: key-pair sets differ ({keys.shape[0]} rows against {k_ref.shape[0]})"
    assert np.array_equal(counts, c_ref), what
    assert same_bits(dS, rows.arrays("dS")[1]), f"{what}: d_strategy differs"
    want, A = rows.arrays("dR")[1], rows.arrays("A")[1]
    once = c_ref == 1
    assert same_bits(dR[once], want[once]), f"{what}: a d_regret row met once differs"
    assert in_budget(dR, want, A, what), what
    return keys, counts


def assert_tables(h, rows, A, what):
    """the device's tables after an apply against the restatement's: pairs and strategy exact, regret within the budget of the launch applied (A: the
    |increment| sums of that launch by pair, taken before the restatement's apply); no increment left"""
    keys, _, R, S = h.tables_get()
    k_ref, R_ref = rows.arrays("R")
    assert keys.shape == k_ref.shape and np.array_equal(keys, k_ref), what
    assert same_bits(S, rows.arrays("S")[1]), f"{what}: strategy differs"
    A_rows = np.array([A.get(tuple(k), [0.0] * 3) for k in keys.tolist()]).reshape(-1, 3)
    assert in_budget(R, R_ref, A_rows, what), what
    _, counts, dR, dS = h.delta_get()
    assert not counts.any() and not dR.any() and not dS.any(), f"{what}: increments left after apply"


def rows_from_device(h, skip=()):
    """the device's tables planted in the restatement, every row touched (delta_get reports unmet rows with zero increments); skip: pairs left out"""
    keys, _, R, S = h.tables_get()
    keep = [i for i, k in enumerate(keys.tolist()) if tuple(k) not in skip]
    rows = X.Rows()
    rows.plant(keys[keep], R[keep], S[keep])
    for k in list(rows.R):
        rows.touch(k)
    return rows


def cuts_of(r0):
    return [-1] + list(range(0, min(3, 6 - r0) + 1))


# ---- 1. one launch ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [1, 5])
@pytest.mark.parametrize("trav", [0, 1])
@pytest.mark.parametrize("r0", [4, 3])
@pytest.mark.parametrize("deck_seed", DECK_SEEDS)
def test_one_launch_vs_restatement_by_every_cut(ctx, sl, oracle, deck_seed, r0, trav, nb):
    h, _, decks = solver_of(ctx, sl, oracle, deck_seed, r0)
    rows = ref_delta(oracle, deck_seed, r0, trav, 0, 0, nb, SEED)
    assert (rows.choice, rows.terminal) == (N_DECKS * nb * F.shape_counts(r0)[trav], N_DECKS * nb * F.shape_counts(r0)[2])
    with pytest.raises(sl.ScopaError):
        h.cut(min(3, 6 - r0) + 1)
    for n, cut in enumerate(cuts_of(r0)):
        h.reset()
        h.cut(cut)
        h.traverse(trav, 0, 0, nb)
        keys, counts = assert_delta(h, rows, f"deck {deck_seed}, round {r0}, traverser {trav}, nb {nb}, cut {cut}")
        c = h.counters()
        assert (c["choice_visits"], c["terminal_visits"]) == ((n + 1) * rows.choice, (n + 1) * rows.terminal)
        assert (c["rows"], c["dropped"], c["iterations"]) == (counts.size, 0, 0) and counts.sum() == rows.choice
        got = h.tables_get()
        assert not got[2].any() and not got[3].any()                      # traverse writes increments only
        assert [X.key_actions(k) for k in keys] == list(got[1])


# ---- 2. planted tables, batch 1 at cut 0 with one deck listed: two iterate calls bit for bit -----------------------------------------------------------------
def planted(oracle, deck_seed=42, r0=4):
    """pairs of the restatement's first traversals and edge rows for them, as test_gpu_full_mccfr.planted: the root (3 cards) with ONE positive regret,
    a 3-card row of the other player with negatives only, a 2-card row with two positives, and strategy rows with a zero sum, a one-hot and a mixed row"""
    decks, _, st = deck_set(oracle, deck_seed, r0)
    seen = X.Rows()
    for trav in range(2):
        X.traverse(st, decks, trav, 0, 0, 2, SEED, seen)
    keys = sorted(seen.count)
    k_root = X.wide_key(X.root_on(st, decks[0]), 0)
    k_neg = next(k for k in keys if (k[0] >> 62) & 1 == 1 and X.key_actions(k) == 3)
    k_two = next(k for k in keys if (k[0] >> 62) & 1 == 0 and X.key_actions(k) == 2)
    k_one = next(k for k in keys if (k[0] >> 62) & 1 == 1 and X.key_actions(k) == 2)
    K = np.array([k_root, k_neg, k_two, k_one], np.uint64)
    R = np.array([[0.0, 2.5, -1.0], [-1.0, -2.0, -0.5], [3.0, 1.0, 0.0], [0.0, 0.0, 0.0]])
    S = np.array([[0.25, 0.5, 2.0], [0.0, 0.0, 0.0], [0.0, 4.0, 0.0], [1.0, 3.0, 0.0]])
    return st, decks, K, np.array([3, 3, 2, 2], np.int32), R, S


def test_planted_tables_and_two_iterate_calls_bit_for_bit(ctx, sl, oracle):
    st, decks, K, n_act, R, S = planted(oracle)
    h, _, _ = solver_of(ctx, sl, oracle, 42, 4)
    bad_b = K.copy(); bad_b[0, 1] |= np.uint64(1 << 40)
    for bad in ((K, [3, 3, 2, 3], R, S), (K & np.uint64((1 << 63) - 1), n_act, R, S), (np.array([K[0]] * 4, np.uint64), [3] * 4, R, S), (bad_b, [4, 3, 2, 2], R, S),
                (bad_b, n_act, R, S)):
        with pytest.raises(sl.ScopaError) as e:
            h.tables_set(*bad)
        assert e.value.status == sl.SCOPA_EINVAL and h.counters()["rows"] == 0
    h.tables_set(K, n_act, R, S)
    order = np.lexsort((K[:, 1], K[:, 0]))
    got = h.tables_get()
    assert np.array_equal(got[0], K[order]) and np.array_equal(got[1], n_act[order]) and same_bits(got[2], R[order]) and same_bits(got[3], S[order])
    # one launch from the planted tables by EVERY cut: at cut > 0 the prefix lanes read sigma through the read-only probe, and the root's one
    # positive regret makes that sigma a point mass -- a probe that missed the row would draw other actions and the counts would differ
    assert F.sigma_of(R[0], 3) == [0.0, 1.0, 0.0]
    for trav in range(2):
        ref = X.Rows()
        ref.plant(K, R, S)
        for k in list(ref.R):
            ref.touch(k)
        X.traverse(st, decks, trav, 0, 0, 3, SEED, ref)
        for cut in cuts_of(4):
            h.tables_set(K, n_act, R, S)
            h.cut(cut)
            h.traverse(trav, 0, 0, 3)
            assert_delta(h, ref, f"planted tables, traverser {trav}, cut {cut}")
    h.tables_set(K, n_act, R, S)
    h.cut(0)
    rows = X.Rows()
    rows.plant(K, R, S)
    counter = 0
    for deck in (2, 1):                                                   # ONE lane makes every add of a launch in the restatement's own depth-first order
        counter = X.iterate(st, decks, 1, SEED, rows, counter, listed=[deck])
        h.iterate(1, 1, lists=[[deck]])
        assert h.counters()["iterations"] == counter
        keys, _, R2, S2 = h.tables_get()
        assert np.array_equal(keys, rows.arrays("R")[0]) and same_bits(R2, rows.arrays("R")[1]) and same_bits(S2, rows.arrays("S")[1])
        assert not h.delta_get()[1].any()
    assert counter == 4


# ---- 3. lists -----------------------------------------------------------------------------------------------------------------------------------------
def test_lists(ctx, sl, oracle):
    deck_seed, r0, trav, nb = 42, 3, 1, 3
    h, st, decks = solver_of(ctx, sl, oracle, deck_seed, r0)
    rows = ref_delta(oracle, deck_seed, r0, trav, 0, 0, nb, SEED, listed=(0, 2, 3))
    full = ref_delta(oracle, deck_seed, r0, trav, 0, 0, nb, SEED)
    assert set(rows.count) < set(full.count)                              # deck 1 has rows of its own: leaving it out shows in the key set
    for bad in ([0, 2, 2], [0, 4], [-1], [0, 1, 2, 3, 0]):
        with pytest.raises(sl.ScopaError) as e:
            h.traverse(trav, 0, 0, nb, bad)
        assert e.value.status == sl.SCOPA_EINVAL
    for bad in ([[0, 1], [2, 2]], [[0, 1], [0, 4]], [[0], [-1]]):
        with pytest.raises(sl.ScopaError) as e:
            h.iterate(nb, 2, lists=bad)
        assert e.value.status == sl.SCOPA_EINVAL
    c = h.counters()
    assert (c["rows"], c["choice_visits"], c["iterations"]) == (0, 0, 0)  # nothing changed
    got = []
    for listed in ([0, 2, 3], [3, 0, 2]):
        h.reset()
        h.traverse(trav, 0, 0, nb, listed)
        assert_delta(h, rows, f"list {listed}")                           # m < n: the rows of the unlisted deck are not there
        got.append(h.delta_get())
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1]) and same_bits(got[0][3], got[1][3])
    h.traverse(trav, 0, 0, nb, [])                                        # an empty list is a no-op
    assert h.counters()["choice_visits"] == 2 * rows.choice
    # iterate with a list per iteration = the traverse / apply sequence: counters and key set
    lists = [[1, 3], [0, 2], [2, 1]]
    h1, _, _ = solver_of(ctx, sl, oracle, deck_seed, r0)
    h2, _, _ = solver_of(ctx, sl, oracle, deck_seed, r0)
    h1.iterate(2, 3, lists=lists)
    for t, lst in enumerate(lists):
        for tr in range(2):
            h2.traverse(tr, 2 * t + tr, 0, 2, lst)
            h2.apply()
    assert h1.counters() == h2.counters() and h1.counters()["iterations"] == 6
    assert np.array_equal(h1.tables_get()[0], h2.tables_get()[0])
    assert h1.counters()["choice_visits"] == 3 * 2 * 2 * sum(F.shape_counts(r0)[:2])


# ---- 4. wide words ------------------------------------------------------------------------------------------------------------------------------------
WIDE = dict(deck_seed=42, r0=5, nb=16, n=300, listed=(297, 298, 299))


def test_wide_words_and_a_deck_index_above_255(ctx, sl, oracle):
    """b0 = 2^32 - nb, iteration bit 31, both seed words, deck indices 297..299 of a handle of 300 decks below a round-5 root"""
    w = WIDE
    seed, iteration, b0 = W.WIDE_SEED, W.ITER_B31, (1 << 32) - w["nb"]
    for trav in range(2):
        rows = ref_delta(oracle, w["deck_seed"], w["r0"], trav, iteration, b0, w["nb"], seed, listed=w["listed"], n=w["n"], fix_seat=None)
        h, _, _ = solver_of(ctx, sl, oracle, w["deck_seed"], w["r0"], seed=seed, n=w["n"], fix_seat=None)
        with pytest.raises(sl.ScopaError) as e:
            h.traverse(trav, iteration, b0 + 1, w["nb"], list(w["listed"]))   # b0 + nb overflows
        assert e.value.status == sl.SCOPA_EINVAL and h.counters()["rows"] == 0
        for cut in cuts_of(w["r0"]):
            h.reset()
            h.cut(cut)
            h.traverse(trav, iteration, b0, w["nb"], list(w["listed"]))
            assert_delta(h, rows, f"wide words, traverser {trav}, cut {cut}")
        h.close()


# ---- 5. the store -------------------------------------------------------------------------------------------------------------------------------------
def set_rows(h, keys):
    R, S = X.rows_for(keys)
    h.tables_set(keys, [X.key_actions(k) for k in keys], R, S)


def assert_own_rows(h, keys, what):
    got = h.tables_get()
    want = np.asarray(keys, np.uint64).reshape(-1, 2)
    want = want[np.lexsort((want[:, 1], want[:, 0]))]
    assert np.array_equal(got[0], want), what                              # every pair exactly once
    R, S = X.rows_for(got[0])
    assert same_bits(got[2], R) and same_bits(got[3], S) and list(got[1]) == [X.key_actions(k) for k in got[0]], what


def test_one_a_word_with_200_hands_in_one_call(ctx, sl, oracle):
    """200 pairs of ONE word A with distinct B set in one call: the import lanes meet word A of others on their probes and race on word B"""
    h, _, _ = solver_of(ctx, sl, oracle, 42, 4, capacity_log2=8)
    B = X.hands3(0, 200)
    keys = np.stack([np.full(200, X.FILLER_A, np.uint64), B], 1)
    for _ in range(3):
        set_rows(h, keys)
        assert_own_rows(h, keys, "200 hands of one A")
        assert (h.counters()["rows"], h.counters()["dropped"]) == (200, 0)


def test_tables_set_refusals_leave_the_store(ctx, sl, oracle):
    """every refusal of tables_set, on 3 planted rows in the smallest store (2^4 slots): a key pair twice, a key without the marker bit, an action count
    that is not the hand's, a hand word at or above 1 << 40, n_rows above the capacity, each array NULL with n_rows > 0.  Each is SCOPA_EINVAL with its
    own message, found by the host before any device work: after it the store answers counters() and holds what it held"""
    _, _, K, n_act, R, S = planted(oracle)
    K, n_act, R, S = K[:3], n_act[:3], R[:3], S[:3]
    h, _, _ = solver_of(ctx, sl, oracle, 42, 4, capacity_log2=4)
    h.tables_set(K, n_act, R, S)
    h.apply()
    before = (h.tables_get(), h.delta_get(), h.counters())
    assert (before[2]["rows"], before[2]["iterations"]) == (3, 1)

    def unchanged():
        now = h.tables_get() + h.delta_get()
        return all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(now, before[0] + before[1])) and h.counters() == before[2]

    seventeen = np.stack([np.full(17, X.FILLER_A, np.uint64), X.hands3(0, 17)], 1)
    R17, S17 = X.rows_for(seventeen)
    high = K.copy(); high[0, 1] |= np.uint64(1 << 40)
    who = "scopa_full_chance_tables_set: "
    bad_key = "a key without the marker bit, a hand word at or above 1 << 40, or an action count that is not the hand's (2 or 3)"
    no_marker = K.copy(); no_marker[:, 0] &= np.uint64((1 << 63) - 1)
    for bad, message in (((K[[0, 1, 0]], n_act[[0, 1, 0]], R, S), "a key pair twice"), ((no_marker, n_act, R, S), bad_key), ((K, [3, 3, 3], R, S), bad_key),
                         ((high, n_act, R, S), bad_key), ((high, [4, 3, 2], R, S), bad_key),
                         ((seventeen, [3] * 17, R17, S17), "n_rows outside [0, capacity] or a NULL array")):
        with pytest.raises(sl.ScopaError) as e:
            h.tables_set(*bad)
        assert e.value.status == sl.SCOPA_EINVAL and who + message in str(e.value), e.value
        assert unchanged(), message
    arrays = [K, n_act, R, S]
    for gone in range(4):
        args = [None if i == gone else sl._ptr(a) for i, a in enumerate(arrays)]
        assert sl.lib().scopa_full_chance_tables_set(h._h, 3, *args) == sl.SCOPA_EINVAL
        assert sl.lib().scopa_last_error(ctx._h).decode() == who + "n_rows outside [0, capacity] or a NULL array"
        assert unchanged(), gone
    h.tables_set(K, n_act, R, S)                                           # ... and the handle goes on
    assert h.counters()["rows"] == 3


def deep_chain(oracle, deck_seed=42, r0=4, trav=1, nb=2):
    """64 filler pairs of home g = (the root pair's home) - 1: set first, they fill g .. g + 63, and the root pair -- player 0's first node, the same on
    every deck of the fix_seat=0 packet -- is claimed by the launch behind them at g + 64, the LAST slot of its probe.  -> (capacity_log2, fillers, root
    pair, the launch's restatement): the smallest store of 2^16 .. 2^20 slots in which no other pair of the launch has its home in [g - 64, g + 129),
    so that nothing else lengthens or enters the chain"""
    decks, _, st = deck_set(oracle, deck_seed, r0)
    root_pair = X.wide_key(X.root_on(st, decks[0]), 0)
    rows = ref_delta(oracle, deck_seed, r0, trav, 0, 0, nb, SEED)
    others = np.array([k for k in rows.count if k != root_pair], np.uint64)
    for capacity_log2 in range(16, 21):
        mask = (1 << capacity_log2) - 1
        g = (int(X.home_of(root_pair[0], root_pair[1], capacity_log2)[0]) - 1) & mask
        d = (X.home_of(others[:, 0], others[:, 1], capacity_log2) - g + 64) & mask
        if not bool((d < 193).any()):
            return capacity_log2, X.fillers(g, 64, capacity_log2), root_pair, rows
    raise AssertionError("no store size isolates the chain")


def test_pair_behind_64_fillers_found_by_every_cut_and_by_the_match(ctx, sl, oracle):
    cap, fill, root_pair, rows = deep_chain(oracle)
    assert rows.count[root_pair] == N_DECKS * 2
    h, st, decks = solver_of(ctx, sl, oracle, 42, 4, capacity_log2=cap)
    for cut in cuts_of(4):
        set_rows(h, fill)
        h.cut(cut)
        h.traverse(1, 0, 0, 2)
        assert_delta(h, rows, f"behind 64 fillers, cut {cut}", hidden=fill)
        assert h.counters()["dropped"] == 0
    # the match: an iteration from the fillers alone claims the root pair behind them again (as a traverser node), gives it regrets and then a strategy
    # row that is not uniform; the match must walk the whole chain to play it
    set_rows(h, fill)
    h.cut(-1)
    h.iterate(2, 1)
    n_rows = h.counters()["rows"]
    keys, _, _, S = h.tables_get()
    table = {tuple(k): [float(x) for x in s] for k, s in zip(keys.tolist(), S)}
    assert len(set(table[root_pair])) > 1
    sums, r2 = h.match(256, 3, per_episode=True)
    want_sums, want_r2 = X.match(st, decks, table, 256, SEED, 3)
    assert np.array_equal(r2, want_r2) and np.array_equal(sums, want_sums) and h.counters()["rows"] == n_rows
    with_root, without = chain_match_without_root(oracle)
    assert not np.array_equal(with_root, without)
    # every cut from NON-ZERO tables with the root pair still at the last slot of its probe: each launch is restated from the device's own tables
    # (test_gpu_full_store.test_row_claimed_at_the_last_slot_of_its_probe does so for the one-deck store).  Sigma at the root is not uniform, so a
    # prefix lane (cut > 0, traverser 1: the root is the opponent's node) whose read-only probe missed the row would draw otherwise: `blind` is
    # the restatement of such a kernel and its counts differ
    hidden = {tuple(k) for k in fill.tolist()}
    it = h.counters()["iterations"]
    for cut in cuts_of(4):
        for trav in (1, 0):
            ref = rows_from_device(h, hidden)
            assert len(set(F.sigma_of(ref.R[root_pair], 3))) > 1, (cut, trav)
            if trav == 1:
                blind = ref.copy()
                blind.R[root_pair] = [0.0, 0.0, 0.0]
                X.traverse(st, decks, trav, it, 0, 16, SEED, blind)
            X.traverse(st, decks, trav, it, 0, 16, SEED, ref)
            if trav == 1:
                assert blind.arrays("count")[1].tolist() != ref.arrays("count")[1].tolist(), cut
            h.cut(cut)
            h.traverse(trav, it, 0, 16)
            assert_delta(h, ref, f"non-zero tables behind 64 fillers, cut {cut}, traverser {trav}", hidden=fill)
            h.apply()
            it += 1
    assert h.counters()["dropped"] == 0


def chain_match_without_root(oracle):
    """(the restatement's match of 256 episodes after one iteration at batch 2 from empty tables, the same with the root pair's row taken away): they
    differ, so a match that did not reach the end of the chain would show (checked on the CPU in test_full_chance_ref.py)"""
    decks, _, st = deck_set(oracle, 42, 4)
    rows = X.Rows()
    X.iterate(st, decks, 2, SEED, rows, 0)
    root_pair = X.wide_key(X.root_on(st, decks[0]), 0)
    with_root = X.match(st, decks, rows.S, 256, SEED, 3)[1]
    return with_root, X.match(st, decks, {k: v for k, v in rows.S.items() if k != root_pair}, 256, SEED, 3)[1]


def test_a_65th_pair_of_one_home_is_dropped_and_the_process_goes_on(ctx, sl, oracle):
    h, _, _ = solver_of(ctx, sl, oracle, 42, 4, capacity_log2=10)
    keys = X.fillers(700, 65, 10)
    set_rows(h, keys[:64])
    assert_own_rows(h, keys[:64], "64 pairs of one home")
    with pytest.raises(sl.ScopaError) as e:
        set_rows(h, keys)
    assert e.value.status == sl.SCOPA_ENOMEM
    c = h.counters()
    assert (c["rows"], c["dropped"]) == (64, 1)
    got = h.tables_get()
    assert len({tuple(k) for k in got[0].tolist()} & {tuple(k) for k in keys.tolist()}) == 64
    set_rows(h, keys[1:])                                                 # the next call works
    assert_own_rows(h, keys[1:], "after the drop")
    assert h.counters()["dropped"] == 1


def test_too_small_store_under_traversal(ctx, sl, oracle):
    r0, nb = 3, 4
    rows = ref_delta(oracle, 42, r0, 0, 0, 0, nb, SEED)
    want = dict(zip([tuple(k) for k in rows.arrays("count")[0].tolist()], rows.arrays("count")[1].tolist()))
    assert len(want) > (1 << 8)
    h, _, _ = solver_of(ctx, sl, oracle, 42, r0, capacity_log2=8)
    with pytest.raises(sl.ScopaError) as e:
        h.traverse(0, 0, 0, nb)
    assert e.value.status == sl.SCOPA_ENOMEM
    c = h.counters()                                                      # the process goes on
    assert c["dropped"] > 0 and c["rows"] <= (1 << 8) and c["choice_visits"] == rows.choice
    keys, counts, _, _ = h.delta_get()
    assert keys.shape[0] == c["rows"] == len({tuple(k) for k in keys.tolist()})
    for k, n in zip(keys.tolist(), counts.tolist()):
        assert n <= want[tuple(k)]                                        # (a pair the restatement never met is a KeyError)
    assert counts.sum() + c["dropped"] == rows.choice                     # every choice visit either updated its row or was dropped
    h.reset()
    try:
        h.traverse(1, 0, 0, 1, [0])                                       # up to 344 rows may not fit 256 slots either: the call returns either way
    except sl.ScopaError as e2:
        assert e2.status == sl.SCOPA_ENOMEM
    assert h.counters()["choice_visits"] == rows.choice + F.shape_counts(r0)[1]


# ---- 6. the match -------------------------------------------------------------------------------------------------------------------------------------
def held_out(oracle, deck_seed=42, r0=4, k=3):
    """k decks of the same packet that the handle does not hold"""
    from scopa_amd.algorithms import packet_decks
    decks, _, _ = deck_set(oracle, deck_seed, r0)
    more = packet_decks(decks[0], r0, N_DECKS + k + 4, 5, fix_seat=0)
    have = {d.tobytes() for d in decks}
    out = np.array([d for d in more if d.tobytes() not in have][:k], np.uint8)
    assert out.shape == (k, 40)
    return out


def test_match_vs_restatement_on_own_and_held_out_decks(ctx, sl, oracle):
    st, decks, K, n_act, R, S = planted(oracle)
    h, _, _ = solver_of(ctx, sl, oracle, 42, 4, seed=W.WIDE_SEED)
    h.tables_set(K, n_act, R, S)
    table = {tuple(k): [float(x) for x in s] for k, s in zip(K.tolist(), S)}
    other = held_out(oracle)
    stream = 5
    for which, ds in ((None, decks), (other, other)):
        for n in (1, 2, 63, 64, 65, 129, 4096):
            sums, r2 = h.match(n, stream, which, per_episode=True)
            want_sums, want_r2 = X.match(st, ds, table, n, W.WIDE_SEED, stream)
            assert np.array_equal(r2, want_r2) and np.array_equal(sums, want_sums), (n, which is None)
        assert np.array_equal(h.match(4096, stream, which), sums) and not np.array_equal(h.match(4096, stream + 1, which), sums)
        # n = 4096 over k decks: each deck gets 2048 / k (+1) episodes per seat; the exact value is the average over episodes' decks
        per_deck = [0.5 * (X.exact_match_value(st, d, table, 0) + X.exact_match_value(st, d, table, 1)) for d in ds]
        weight = np.bincount([X.deck_of_episode(i, 4096, len(ds)) for i in range(4096)], minlength=len(ds)) / 4096.0
        exact = float(np.dot(weight, per_deck))
        rewards = r2.astype(np.float64) / 2.0
        se = rewards.std(ddof=1) / np.sqrt(4096)
        print("match mean", rewards.mean(), "exact", exact, "se", se)
        assert abs(rewards.mean() - exact) <= 5.0 * se
    bad = other.copy()
    bad[1, [38, 2]] = bad[1, [2, 38]]                                     # a stock card swapped with one the root has seen
    with pytest.raises(sl.ScopaError) as e:
        h.match(64, stream, bad)
    assert e.value.status == sl.SCOPA_EINVAL
    with pytest.raises(sl.ScopaError) as e:
        h.match((1 << 36) + 1, stream)                                    # more episodes than one launch has lanes for
    assert e.value.status == sl.SCOPA_EINVAL
    assert h.counters()["rows"] == 4                                      # the match never inserts
    assert not h.match(0).any()


# ---- 7. the Python trainer ----------------------------------------------------------------------------------------------------------------------------
def test_trainer(ctx, sl, oracle, tmp_path):
    from scopa_amd.algorithms import FullChanceMCCFRTrainer
    decks, acts, st = deck_set(oracle, 42, 4)
    ctx.mccfr_seed(SEED)
    a = FullChanceMCCFRTrainer(decks=decks, root_actions=acts, capacity_log2=13, batch=8, ctx=ctx)
    b = FullChanceMCCFRTrainer(decks=decks[::-1].copy(), root_actions=acts, capacity_log2=14, batch=8, ctx=ctx)
    a.train(2)
    a.train(2, sample=2, seed=3)
    assert a.counters()["iterations"] == 8 and b.counters()["rows"] == 0
    assert a.counters()["choice_visits"] == (2 * 4 + 2 * 2) * 8 * 21 * 7
    t = a.tables()
    assert t["keys"].shape == (a.counters()["rows"], 2) and a.counters()["rows"] > 100
    path = str(tmp_path / "full_chance.npz")
    a.save(path)
    b.load(path)                                                          # (another deck order, so another root hand: the rows are by key)
    u = b.tables()
    assert np.array_equal(t["keys"], u["keys"]) and np.array_equal(t["n_act"], u["n_act"]) and same_bits(t["regret"], u["regret"]) and same_bits(t["strategy"], u["strategy"])
    # info_sets: the decoded strings are the states' own, along random play on two different decks of the set and on a held-out deck
    info, rng, found = b.info_sets, np.random.RandomState(3), 0
    assert len(info) == u["keys"].shape[0]
    for deck in (decks[1], decks[3], held_out(oracle)[0]):
        ps = sl.FullState(deck=deck)
        for x in acts:
            ps.step(x)
        for _ in range(40):
            s = sl.FullState(deck=deck)
            s.s[:] = ps.s
            while not s.is_terminal():
                p, legal = s.current_player(), s.legal()
                node = info.get((p, s.infoset_string(p)))
                probs = b.average_policy(s)
                assert list(probs) == legal and abs(sum(probs.values()) - 1.0) < 1e-12
                if len(legal) > 1 and node is not None:
                    found += 1
                    assert list(node.legal_actions) == sorted(legal)
                    total = node.strategy_sum.sum()
                    want = node.strategy_sum / total if total > 1e-12 else np.full(len(legal), 1.0 / len(legal))
                    assert [probs[c] for c in sorted(legal)] == list(want)
                s.step(legal[rng.randint(len(legal))])
    assert found > 100
    assert {X.key_to_string(k) for k in u["keys"].tolist()} == {k[1] for k in info}
    mean, se, scopas = b.evaluate_vs_random(2048)
    mean2, se2, _ = b.evaluate_vs_random(2048, decks=held_out(oracle))
    assert abs(mean) <= 21 and se > 0 and abs(mean2) <= 21 and se2 > 0 and scopas["data_collected"]
    tiny = FullChanceMCCFRTrainer(decks=decks, root_actions=acts[:18], capacity_log2=5, batch=4, ctx=ctx)
    with pytest.raises(RuntimeError, match="dropped"):
        tiny.train(1)
    for x in (tiny, a, b):
        x.close()


def test_one_deck_trainer_has_the_one_deck_solvers_strings(ctx, sl, oracle):
    """Round-5 root (36 histories), batch 512, 2 iterations on either trainer: each meets every infoset below the root (a history is missed with
    probability (35 / 36)^512 < 1e-6 per launch), so the string sets are equal although the draws differ"""
    from scopa_amd.algorithms import FullChanceMCCFRTrainer, FullMCCFRTrainer
    deck, acts, _ = root_of(oracle, 42, 4)
    ps = sl.FullState(deck=deck)
    for x in acts:
        ps.step(x)
    more = []
    rng = np.random.RandomState(1)
    for _ in range(6):
        legal = ps.legal()
        more.append(int(legal[rng.randint(len(legal))]))
        ps.step(more[-1])
    ctx.mccfr_seed(SEED)
    one = FullChanceMCCFRTrainer(decks=deck[None, :], root_actions=list(acts) + more, capacity_log2=10, batch=512, ctx=ctx)
    ref = FullMCCFRTrainer(deck=deck, root_actions=list(acts) + more, capacity_log2=10, batch=512, ctx=ctx)
    one.train(2)
    ref.train(2)
    assert one.counters()["choice_visits"] == ref.counters()["choice_visits"] == 2 * 512 * 21
    assert {k[1] for k in one.info_sets} == {k[1] for k in ref.info_sets} and len(one.info_sets) == one.counters()["rows"] > 10
    one.close()
    ref.close()
