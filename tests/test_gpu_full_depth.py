"""GPU checks of the FullScopa walk and match (scopa_amd/csrc/scopa_full_mccfr.hip) at the shape the solver is used at: from the deal's root, 36 plies
and up to 12 frames deep, on the project's edge regret rows, and the match at the edges of its episode count, against tests/full_mccfr_ref.py.

The comparison is tests/test_gpu_full_mccfr.py's (assert_delta, in_budget, same_bits): key set, visit counts, counters and d_strategy exact, d_regret
bit-identical on rows met once and within K_REORDER * eps * A_row + 2 eps |R_ref| (oracle/mccfr_edges.py) elsewhere.  Each traverser's reference from
the deal is one F.walk from zero tables (30 533 and 27 004 rows, 19 547 and 14 244 of them met more than once), computed once per process;
tests/test_full_mccfr_ref.py holds the inputs used here to the guards named below without a GPU.

Frames: cut 0 from the deal runs all 12 frames of the per-lane stack in one lane, cut 1 runs 10 below the cut, cut 2 runs 8, cut 3 (the default) 6;
the round-1 root runs 10 at cut 0.

A mutation of the kernel source and the test that fails under it (G: the CPU guard in tests/test_full_mccfr_ref.py showing that the restatement separates).
Each variant was built and run once against this module on an MI355X: the tests named failed; the `>=` variant passed all 31 tests of the module:
  kMaxFrames lowered to 11            test_deal_one_traversal_by_every_cut (cut 0: the 12th frame returns 0 with its sub-tree unwalked: terminal_visits
                                      falls below 46 656, d_regret moves) and test_deal_iterate_bit_for_bit
  q cut to 15 bits in fm_draw         test_deal_one_traversal_by_every_cut[0] (traverser 0 draws at ply 33 with all 12 digits in q; traverser 1 never
                                      draws past 11 digits, q < 23 328); G test_deal_q_word_separates
  s_vals[q] read at q % 36            test_deal_one_traversal_by_every_cut (cut 3 and the default, which is 3: 216 sub-trees with three rounds below each;
                                      cuts 1 and 2 have 6 and 36 and cannot show it): lane 0 takes another sub-tree's value where q >= 36, which moves
                                      the d_regret rows of the rounds above the cut
  mc_sigma's R[i] > 0.0 to >= 0.0     NONE CAN: the mutant computes the same numbers.  A cell at +0.0 gives pos = 0.0 either way; a cell at -0.0 gives
                                      pos = -0.0, and every use of it rounds back to what +0.0 gives (s == 0.0 holds for -0.0; -0.0 / s added to a sum or
                                      into a cell that starts at +0.0 leaves +0.0; acc + -0.0 > u is acc > u).  The neighbouring mutants that do change a
                                      number fail test_edge_rows_on_every_key: `> 0.0` to `!= 0.0` (allneg, onehot, big: negative cells enter the sum) and
                                      a flush of subnormals, `> 0.0` to `> 2.3e-308` (subnormal: uniform over every cell); G test_edge_rows_guard
  the match's 1e-12 to 1e-14          test_match_threshold (a row summing to 1e-13 would be played as a policy); G test_match_threshold_guard
  2 * i < n to 2 * i <= n             test_match_shapes[2], [64] (episode n / 2 changes seat; an odd n cannot show it); G test_match_inputs_separate
  stream_id << 8 cut to 16 bits       test_match_shapes (every n: stream id (1 << 24) - 1); G test_match_inputs_separate

Measured once on an MI355X, deck 42, from the deal (wall time of the call, the launch and its counter read-back; `timed` prints them again):
  cut 0, nb 1 (ONE lane walks the whole traversal)   0.52 s as traverser 0 (121 303 choice nodes), 0.44 s as traverser 1 (74 648)
  cut 1 / 2 / 3, nb 1                                0.126 / 0.023 / 0.007 s as traverser 0, 0.089 / 0.018 / 0.005 s as traverser 1
  iterate(1, 1) at cut 0                             0.94 s, so the bit-for-bit test stays at the deal (the issue's limit for moving it was 5 s)
  cut 0, nb 65, traverser 1                          0.60 s (65 lanes in two workgroups); 0.005 s by the default cut
Largest d_regret error over its budget in the deal-root launches: 6.6e-05 (traverser 1, the default cut); 0.0 at cut 0, where one lane adds in the
restatement's order."""
import ctypes as C
import time

import numpy as np
import pytest

import full_mccfr_ref as F
import mccfr_edges as E
import philox_words as W
from test_gpu_full_mccfr import SEED, assert_delta, assert_tables, in_budget, same_bits

pytestmark = pytest.mark.gpu

CAP = 18                                       # tests/test_full_mccfr_ref.py::test_deal_capacity_guard: no probe of these key sets looks at more than 13 slots
DEAL_VISITS, DEAL_TERMINALS = (121303, 74648), 46656
CUTS = (-1, 0, 1, 2, 3)
MATCH_NS, MATCH_STREAM = (1, 2, 63, 64, 65, 129), (1 << 24) - 1
EDGE_ROOTS = ((42, 4), (42, 3), (7, 3))        # (deck seed, round of the root)
_CACHE = {}


# ---- shared inputs, computed once (plain CPU code: tests/test_full_mccfr_ref.py imports them for its guards) --------------------------------------------
def deal_root(oracle, deck_seed=42):
    if ("deal", deck_seed) not in _CACHE:
        deck = oracle.full_deal_py_seed(deck_seed)
        _CACHE["deal", deck_seed] = (deck, F.root_of(deck))
    return _CACHE["deal", deck_seed]


def deal_ref(oracle, trav):
    """the restatement's increments of traversal 0 of `trav` at iteration 0 from the deal of deck 42, zero tables: Rows (read only)"""
    if ("walk", trav) not in _CACHE:
        rows = F.Rows()
        F.walk(deal_root(oracle)[1], trav, 0, 0, SEED, rows)
        _CACHE["walk", trav] = rows
    return _CACHE["walk", trav]


def deal_iterate_ref(oracle):
    """the restatement's tables after F.iterate(root, 1, SEED, rows, 0) from the deal of deck 42: its first half IS deal_ref(0), applied"""
    if "iterate" not in _CACHE:
        rows = deal_ref(oracle, 0).copy()
        rows.apply()
        F.traverse(deal_root(oracle)[1], 1, 1, 0, 1, SEED, rows)
        rows.apply()
        _CACHE["iterate"] = rows
    return _CACHE["iterate"]


def sub_root(oracle, deck_seed, r0):
    """(deck, actions, oracle state) of the root after r0 rounds of random play under RandomState(1000 * r0)"""
    if ("root", deck_seed, r0) not in _CACHE:
        deck = oracle.full_deal_py_seed(deck_seed)
        st, acts = F.random_root(deck, r0, np.random.RandomState(1000 * r0))
        _CACHE["root", deck_seed, r0] = (deck, acts, st)
    return _CACHE["root", deck_seed, r0]


def round_1_ref(oracle, trav, nb=5):
    """nb traversals with ids ending at 2^32 - 1 from the round-1 root of deck 42 (10 frames at cut 0), zero tables"""
    if ("r1", trav, nb) not in _CACHE:
        rows = F.Rows()
        F.traverse(sub_root(oracle, 42, 1)[2], trav, 0, (1 << 32) - nb, nb, SEED, rows)
        _CACHE["r1", trav, nb] = rows
    return _CACHE["r1", trav, nb]


def edge_ref(oracle, deck_seed, r0, name, trav):
    """((keys, n_act, R, S) planted, Rows after F.traverse(trav, 0, 0, 8) on them with every planted key touched, A of that launch); name None: zero tables"""
    key = ("edge", deck_seed, r0, name, trav)
    if key not in _CACHE:
        root = sub_root(oracle, deck_seed, r0)[2]
        if ("keys", deck_seed, r0) not in _CACHE:
            _CACHE["keys", deck_seed, r0] = F.subgame_keys(root)
        keys = _CACHE["keys", deck_seed, r0]
        planted = F.edge_rows(keys, name) if name else (keys, np.array([F.key_actions(k) for k in keys], np.int32), np.zeros((keys.size, 3)), np.zeros((keys.size, 3)))
        rows = F.Rows()
        rows.plant(planted[0], planted[2], planted[3])
        F.traverse(root, trav, 0, 0, 8, SEED, rows)
        met = len(rows.count)
        rows.touch_all(keys)
        _CACHE[key] = (planted, rows, met)
    return _CACHE[key]


def threshold_tables(oracle):
    """(root, [table, table]) on the round-4 root of deck 42: the root's strategy row at [1e-13, 0, 0] (below the threshold: uniform), then at
    [1e-11, 0, 3e-11] (above: a policy); a three-card row of the other player summing to 0.0 and a two-card row at [0, 1e-13] besides"""
    root = sub_root(oracle, 42, 4)[2]
    keys = F.subgame_keys(root).tolist()
    k_root = F.key_of(root, 0)
    k3 = next(k for k in keys if (k >> 62) & 1 == 1 and F.key_actions(k) == 3)
    k2 = next(k for k in keys if (k >> 62) & 1 == 1 and F.key_actions(k) == 2)
    rest = {k3: [0.0, 0.0, 0.0], k2: [0.0, 1e-13, 0.0]}
    return root, [{**rest, k_root: [1e-13, 0.0, 0.0]}, {**rest, k_root: [1e-11, 0.0, 3e-11]}]


def handle_of(ctx, sl, oracle, deck_seed, r0, capacity_log2=CAP, seed=SEED):
    ctx.mccfr_seed(seed)
    if r0 == 0:
        return sl.FullMCCFR(ctx, deal_root(oracle, deck_seed)[0], None, capacity_log2)
    deck, acts, _ = sub_root(oracle, deck_seed, r0)
    ps = sl.FullState(deck=deck)
    for a in acts:
        ps.step(a)
    return sl.FullMCCFR(ctx, deck, ps.s, capacity_log2)


def same_store(a, b):
    return all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- 1. the deal's root against the restatement ----------------------------------------------------------------------------------------------------------
TIMES = {}      # what of a timed launch -> seconds, printed by the tests that fill it (recorded in the module docstring)


def timed(what, fn, *args):
    t = time.perf_counter()
    fn(*args)
    TIMES[what] = time.perf_counter() - t
    print(f"{what}: {TIMES[what]:.3f} s on the device")


@pytest.mark.parametrize("trav", [0, 1])
def test_deal_one_traversal_by_every_cut(ctx, sl, oracle, trav):
    """nb = 1 from the deal by every cut against ONE reference: 12 frames in one lane (cut 0), 10 and 8 frames below a cut (cuts 1 and 2), the default (3)"""
    rows = deal_ref(oracle, trav)
    assert (rows.choice, rows.terminal) == (DEAL_VISITS[trav], DEAL_TERMINALS) and max(rows.count.values()) > 100
    h = handle_of(ctx, sl, oracle, 42, 0)
    for n, cut in enumerate(CUTS):
        h.reset()
        h.cut(cut)
        timed(f"deal, traverser {trav}, cut {cut}, nb 1", h.traverse, trav, 0, 0, 1)
        keys, _ = assert_delta(h, rows, f"deal, traverser {trav}, cut {cut}")
        c = h.counters()
        assert (c["choice_visits"], c["terminal_visits"], c["dropped"]) == ((n + 1) * DEAL_VISITS[trav], (n + 1) * DEAL_TERMINALS, 0), (cut, c)
        assert c["rows"] == keys.size == len(rows.count)


def test_deal_iterate_bit_for_bit(ctx, sl, oracle):
    """cut 0, batch 1: one lane makes every add of both halves in the restatement's order, and the second half's sigma is read from the 30 533 rows the
    first applied: keys, regret and strategy bit for bit"""
    rows = deal_iterate_ref(oracle)
    h = handle_of(ctx, sl, oracle, 42, 0)
    h.cut(0)
    timed("deal, iterate(1, 1), cut 0", h.iterate, 1, 1)
    keys, _, R, S = h.tables_get()
    k_ref, R_ref = rows.arrays("R")
    assert np.array_equal(keys, k_ref), f"key sets differ ({keys.size} rows against {k_ref.size})"
    assert same_bits(R, R_ref), "regret differs"
    assert same_bits(S, rows.arrays("S")[1]), "strategy differs"
    c = h.counters()
    assert (c["iterations"], c["choice_visits"], c["terminal_visits"], c["dropped"], c["rows"]) == (2, sum(DEAL_VISITS), 2 * DEAL_TERMINALS, 0, keys.size)
    _, counts, dR, dS = h.delta_get()
    assert not counts.any() and not dR.any() and not dS.any()


def test_deal_batch_65_cut_0_against_the_default_cut(ctx, sl):
    """A full wavefront plus a lone lane, ids up to 2^32 - 1, both key words, iteration bit 31, traverser 1: the two forms against each other with no
    restatement.  Exact between them: key set, counts, counters and d_strategy (every add into a cell of a launch is the same number).  Nothing is
    asserted between the two d_regret images: their budget needs the A of a restatement"""
    nb, got = 65, []
    deck = sl.full_deal_py_seed(42)
    ctx.mccfr_seed(W.WIDE_SEED)
    for cut in (0, -1):
        h = sl.FullMCCFR(ctx, deck, None, 22)
        h.cut(cut)
        timed(f"deal, traverser 1, cut {cut}, nb {nb}", h.traverse, 1, W.ITER_B31, (1 << 32) - nb, nb)
        keys, counts, _, dS = h.delta_get()
        c = h.counters()
        assert c["dropped"] == 0 and c["rows"] == keys.size == np.unique(keys).size
        assert counts.sum(dtype=np.uint64) == c["choice_visits"] == nb * DEAL_VISITS[1] and c["terminal_visits"] == nb * DEAL_TERMINALS
        got.append((keys, counts, dS, c))
        h.close()
    (k0, n0, s0, c0), (k1, n1, s1, c1) = got
    assert np.array_equal(k0, k1), f"key sets differ ({k0.size} rows against {k1.size})"
    assert np.array_equal(n0, n1) and same_bits(s0, s1) and c0 == c1
    assert n0.max() > nb                                                  # rows met more than once per traversal


@pytest.mark.parametrize("cut", [0, -1])
@pytest.mark.parametrize("trav", [0, 1])
def test_round_1_small_batch(ctx, sl, oracle, trav, cut):
    """5 lanes of a wavefront (cut 0: 10 frames) and 5 workgroups (the default cut, 2: 36 sub-trees with 3 rounds below), ids 2^32 - 5 .. 2^32 - 1"""
    nb = 5
    rows = round_1_ref(oracle, trav, nb)
    h = handle_of(ctx, sl, oracle, 42, 1)
    h.cut(cut)
    h.traverse(trav, 0, (1 << 32) - nb, nb)
    assert_delta(h, rows, f"round 1, traverser {trav}, cut {cut}, nb {nb}")
    c = h.counters()
    assert (c["choice_visits"], c["terminal_visits"], c["dropped"]) == (nb * F.shape_counts(1)[trav], nb * F.shape_counts(1)[2], 0) == (rows.choice, rows.terminal, 0)


# ---- 2. edge regret rows on every key of a sub-game ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", E.FINITE_TABLES)
@pytest.mark.parametrize("deck_seed,r0", EDGE_ROOTS)
def test_edge_rows_on_every_key(ctx, sl, oracle, deck_seed, r0, name):
    """every key of the sub-game holds a row of the edge table: the walk reads them through fm_row and fm_pick, by cut 0 and by the default cut"""
    h = handle_of(ctx, sl, oracle, deck_seed, r0, capacity_log2=14)
    for trav in range(2):
        planted, rows, _ = edge_ref(oracle, deck_seed, r0, name, trav)
        for cut in (0, -1):
            what = f"{name}, deck {deck_seed}, round {r0}, traverser {trav}, cut {cut}"
            h.cut(cut)
            h.tables_set(*planted)
            h.traverse(trav, 0, 0, 8)
            keys, counts = assert_delta(h, rows, what)
            assert keys.size == planted[0].size == h.counters()["rows"] and counts.sum() == 8 * F.shape_counts(r0)[trav]
            if name == "subnormal":
                # sigma of a kept 5e-324: uniform over the NON-ZERO cells (a flushed one: uniform over every cell, and other draws)
                _, _, _, dS = h.delta_get()
                opp = (((keys >> np.uint64(62)) & np.uint64(1)) != trav) & (counts > 0)
                live = planted[2][opp] > 0.0
                assert opp.sum() > 10 and (live.sum(1) < planted[1][opp]).any()
                sigma, want = np.where(live, 1.0 / live.sum(1)[:, None], 0.0), np.zeros(live.shape)
                for visit in range(int(counts[opp].max())):               # (the cell is a sum of `count` adds of sigma, not count * sigma)
                    want = np.where(visit < counts[opp, None], want + sigma, want)
                assert same_bits(dS[opp], want), what + ": sigma of subnormal regrets"
            done = rows.copy()
            A = dict(done.A)
            done.apply()
            h.apply()
            assert_tables(h, done, A, what + ", applied")
    assert h.counters()["dropped"] == 0


# ---- 3. the match at its edges ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def trained(ctx, sl, oracle):
    """a store trained at the deal, iterate(1, 1) at cut 0, and the agent's table read back from it (no dependence on the tests above)"""
    h = handle_of(ctx, sl, oracle, 42, 0)                                 # trained under SEED (the store deal_iterate_ref restates: the guards' table)
    if "trained" not in _CACHE:
        h.cut(0)
        h.iterate(1, 1)
        _CACHE["trained"] = h.tables_get()
    else:
        h.tables_set(*_CACHE["trained"])                                  # the same store for every case, trained once
    ctx.mccfr_seed(W.WIDE_SEED)                                           # ... and matched under both key words
    keys, _, _, S = h.tables_get()
    assert keys.size > 30533 and (S.sum(1) > 1e-12).sum() > 10000         # more rows than the first half alone leaves, and policies among them
    return h, deal_root(oracle)[1], {int(k): [float(x) for x in s] for k, s in zip(keys, S)}


@pytest.mark.parametrize("n", MATCH_NS)
def test_match_shapes(trained, n):
    """the root at the deal (36 plies, keys of every round), an odd n, n below, at and above a block of 64, the seat split inside the second block
    (n = 129: episode 65), the last stream id accepted: every episode's reward and all six sums"""
    h, root, table = trained
    before = (h.tables_get(), h.counters())
    sums, r2 = h.match(n, MATCH_STREAM, per_episode=True)
    want_sums, want_r2 = F.match(root, table, n, W.WIDE_SEED, MATCH_STREAM)
    assert r2.dtype == np.int8 and np.array_equal(r2, want_r2), f"episodes of n = {n}"
    assert np.array_equal(sums, want_sums) and np.array_equal(h.match(n, MATCH_STREAM), sums)
    assert same_store(h.tables_get(), before[0]) and h.counters() == before[1]               # the match never inserts


def test_match_threshold(ctx, sl, oracle):
    """the match's own copy of the average policy's rule: strategy rows summing to 0.0 and to 1e-13 are played uniformly, one summing to 4e-11 is not"""
    root, tables = threshold_tables(oracle)
    h = handle_of(ctx, sl, oracle, 42, 4, capacity_log2=10, seed=W.WIDE_SEED)
    for n, table in enumerate(tables):
        keys = np.array(sorted(table), np.uint64)
        S = np.array([table[int(k)] for k in keys])
        h.tables_set(keys, [F.key_actions(k) for k in keys], np.zeros_like(S), S)
        sums, r2 = h.match(129, MATCH_STREAM, per_episode=True)
        want_sums, want_r2 = F.match(root, table, 129, W.WIDE_SEED, MATCH_STREAM)
        assert np.array_equal(r2, want_r2) and np.array_equal(sums, want_sums), f"table {n}"


def test_match_refuses_a_stream_id_of_25_bits(trained, sl):
    h, _, _ = trained
    h.traverse(0, 2, 0, 1)                                                # increments left unapplied: they are part of what must stay
    before = (h.tables_get(), h.delta_get(), h.counters())
    for per_episode in (False, True):
        with pytest.raises(sl.ScopaError) as e:
            h.match(129, 1 << 24, per_episode=per_episode)
        assert e.value.status == sl.SCOPA_EINVAL
    assert same_store(h.tables_get(), before[0]) and same_store(h.delta_get(), before[1]) and h.counters() == before[2]
    assert h.match(2, MATCH_STREAM).any() or h.match(64, MATCH_STREAM).any()          # ... and the handle goes on


# ---- 4. the room contract of tables_get / delta_get --------------------------------------------------------------------------------------------------------
def test_rows_out_room(ctx, sl, oracle):
    """tables_get / delta_get with too little room: SCOPA_EINVAL, the needed count in *n_rows, nothing written; the count alone with every array NULL
    (tests/test_gpu_full_chance_depth.py::test_rows_out_room, on the one-deck handle: the round-4 root, one launch of 4 traversals, 2^10 slots)"""
    L, p = sl.lib(), sl._ptr
    h = handle_of(ctx, sl, oracle, 42, 4, capacity_log2=10)
    empty = C.c_int64(-7)
    for fn in (L.scopa_full_mccfr_tables_get, L.scopa_full_mccfr_delta_get):
        assert fn(h._h, C.byref(empty), None, None, None, None) == sl.SCOPA_OK and empty.value == 0
        empty.value = 0
        one = np.full(1, 0x5A5A5A5A5A5A5A5A, np.uint64)
        assert fn(h._h, C.byref(empty), p(one), None, None, None) == sl.SCOPA_OK and empty.value == 0 and (one == 0x5A5A5A5A5A5A5A5A).all()
        empty.value = -7
    h.traverse(0, 0, 0, 4)
    rows = h.counters()["rows"]
    assert rows > 8
    sent_u, sent_f = 0x5A5A5A5A5A5A5A5A, -12345.5
    for fn, third in ((L.scopa_full_mccfr_tables_get, True), (L.scopa_full_mccfr_delta_get, False)):
        n = C.c_int64(0)
        assert fn(h._h, C.byref(n), None, None, None, None) == sl.SCOPA_OK and n.value == rows          # the count alone
        keys, a, b = np.full(rows, sent_u, np.uint64), np.full((rows, 3), sent_f), np.full((rows, 3), sent_f)
        x = np.full(rows, 0x5A5A5A5A, np.int32 if third else np.uint32)
        args = (p(keys), p(x), p(a), p(b)) if third else (p(keys), p(a), p(b), p(x))
        n = C.c_int64(rows - 1)
        assert fn(h._h, C.byref(n), *args) == sl.SCOPA_EINVAL
        assert n.value == rows and (keys == sent_u).all() and (a == sent_f).all() and (b == sent_f).all() and (x == 0x5A5A5A5A).all()
        n = C.c_int64(rows)
        assert fn(h._h, C.byref(n), *args) == sl.SCOPA_OK and n.value == rows
        assert not (keys == sent_u).any() and not (a == sent_f).any() and not (b == sent_f).any() and not (x == 0x5A5A5A5A).any()
        assert len(set(keys.tolist())) == rows                             # (the handle goes with the test, as in this module's other tests)
