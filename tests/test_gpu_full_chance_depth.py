"""GPU checks of FullScopa over a set of decks (scopa_amd/csrc/scopa_full_chance.hip, scopa_full_wide.h) at the shapes the solver is used at: from the
deal's root on decks that share the first rounds, cut-0 launches of several workgroups, the project's edge regret rows on every pair of a sub-game, the
match at the edges of its episode count, stream id and deck count, and the host checks of create and of the row read-backs, against
tests/full_chance_ref.py.

The comparison is tests/test_gpu_full_chance.py's (assert_delta, assert_tables): pair set, visit counts, counters and d_strategy exact, d_regret
bit-identical on rows met once and within K_REORDER * eps * A_row + 2 eps |R_ref| (oracle/mccfr_edges.py) elsewhere.  No tolerance is added here.
DEAL3 is three decks that share the table and the deals of rounds 0 and 1; each traverser's reference from the deal is one X.walk per deck from zero
tables (72 884 and 55 274 rows; 46 and 14 pairs met on two decks, 5 and 2 on all three), computed once per process.  tests/test_full_chance_ref.py holds
the inputs used here to the guards named below without a GPU.

A mutation of the kernel source and the test that fails under it (G: the CPU guard in tests/test_full_chance_ref.py showing that the restatement
separates).  Each variant was built apart from the tree and run once against the one test named, on an MI355X; all six failed it:
  cut-0 lane id without the blockIdx term     test_cut_0_across_workgroups (every workgroup walks lanes 0 .. 63: 43 pairs against 91);
                                              G test_cut_0_lane_numbering_separates
  wide_key's table loop stopped at 8 slots    test_deal_one_traversal_by_every_cut, both traversers (tables of 9 and 10 cards: 72 886 pairs against
                                              72 884, 55 276 against 55 274); G test_deal3_is_what_the_gpu_test_needs
  the walk's tag without deck_index << 8      test_deal_iterate_bit_for_bit (deck index 1 draws as deck 0: 28 020 pairs against 27 717); the round-4 launches
                                              of tests/test_gpu_full_chance.py separate it too (G test_one_launch_inputs_separate_wrong_walks; not run)
  the match's 1e-12 to 1e-14                  test_match_threshold (the row summing to 1e-13 is played as a policy); G test_match_inputs_separate
  the match's stream_id << 8 cut to 16 bits   test_match_shapes, every n (stream id (1 << 24) - 1); G test_match_inputs_separate
  mc_sigma's R[i] > 0.0 to != 0.0             test_edge_rows_on_every_pair under allneg, onehot and big at all three roots (negative cells enter the sum);
                                              small_large and subnormal hold no negative cell and pass; G test_edge_rows_guard, which also shows
                                              that a flush of subnormals moves the subnormal table's image

Measured once on an MI355X, DEAL3 from the deal, nb = 1 (wall time of the call, the launch and its counter read-back; `timed` prints them again):
  cut 0 (three lanes of ONE wavefront, on tables that differ from round 2 on)   0.710 s as traverser 0 (363 909 choice nodes), 0.538 s as traverser 1
                                                                                (223 944); one lane on one deck takes 0.52 / 0.44 s
  cut 1 / 2 / 3                                                                 0.136 / 0.030 / 0.009 s as traverser 0, 0.106 / 0.021 / 0.006 s as traverser 1
  iterate(1, 1) on deck index 1 alone, cut 0                                    0.95 s
No launch is near 5 s, so the cut-0 cases keep all three decks.
Largest d_regret error over its budget in the DEAL3 launches: 1.6e-04 (traverser 1, cut 2); 0.0 at cut 0 in that run (the three lanes add
into the shared rows of rounds 0 and 1 from one wavefront)."""
import ctypes as C
import time

import numpy as np
import pytest

import full_chance_ref as X
import full_mccfr_ref as F
import mccfr_edges as E
import philox_words as W
from test_gpu_full_chance import SEED, assert_delta, assert_tables, deck_set, ref_delta, solver_of
from test_gpu_full_depth import same_store
from test_gpu_full_mccfr import same_bits

pytestmark = pytest.mark.gpu

CAP = 18                                       # tests/test_full_chance_ref.py::test_deal3_capacity_guard: the longest probe of the deal key sets
DEAL3_VISITS, DEAL3_TERMINALS = (363909, 223944), 139968                  # 3 x the one-deck figures: every deck's traversal has the same shape
DEAL3_ROWS, DEAL3_ONCE, DEAL3_MAX_COUNT = (72884, 55274), (22865, 21258), (151, 280)
DEAL3_ON_TWO, DEAL3_ON_THREE = (46, 14), (5, 2)                           # pairs met on exactly two decks, on all three
CUTS = (-1, 0, 1, 2, 3)
MATCH_NS, MATCH_STREAM = (1, 2, 63, 64, 65, 129), (1 << 24) - 1
EDGE_ROOTS = ((42, 4), (42, 3), (7, 3))        # (deck seed, round of the root) of test_gpu_full_chance.deck_set
LANES = dict(deck_seed=42, r0=5, nb=33, n=4)   # 132 lanes at cut 0: two workgroups and 4 lanes, deck boundaries at lanes 33, 66 and 99
_CACHE = {}


# ---- shared inputs, computed once (plain CPU code: tests/test_full_chance_ref.py imports them for its guards) ---------------------------------------------
def deal3(oracle):
    """(decks [3][40], the deal's root on deck 0): three decks with the first 16 cards in common"""
    if "deal3" not in _CACHE:
        from scopa_amd.algorithms import packet_decks
        decks = packet_decks(oracle.full_deal_py_seed(42), 2, 3, 5)
        _CACHE["deal3"] = (decks, F.root_of(decks[0]))
    return _CACHE["deal3"]


def held_out_deal(oracle, k):
    """k decks of DEAL3's packet that the handle does not hold"""
    from scopa_amd.algorithms import packet_decks
    more = packet_decks(oracle.full_deal_py_seed(42), 2, 12, 5)
    assert np.array_equal(more[:3], deal3(oracle)[0])
    return np.ascontiguousarray(more[3:3 + k])


def deal3_ref(oracle, trav):
    """(the restatement's increments of traversal 0 of `trav` at iteration 0 on every deck of DEAL3 from zero tables: Rows (read only),
    pair -> set of the decks that met it)"""
    if ("walk", trav) not in _CACHE:
        decks, root = deal3(oracle)
        rows, seen = X.Rows(), {}
        draw, q_max = oracle.philox_uniform, [0]

        def watched(seed, c0, *rest):                                      # the largest q of a draw's counter word, for the CPU guard
            q_max[0] = max(q_max[0], c0 & 0xFFFF)
            return draw(seed, c0, *rest)

        X.O.philox_uniform = watched
        try:
            X.traverse(root, decks, trav, 0, 0, 1, SEED, rows, seen=seen)
        finally:
            X.O.philox_uniform = draw
        _CACHE["walk", trav], _CACHE["q", trav] = (rows, seen), q_max[0]
    return _CACHE["walk", trav]


def deal3_trained_ref(oracle):
    """the restatement's tables after one iteration at batch 1 on all three decks (the store test_match_shapes trains on the device, up to the order
    of its adds): its first half IS deal3_ref(0), applied.  For the CPU guards"""
    if "trained_ref" not in _CACHE:
        decks, root = deal3(oracle)
        rows = deal3_ref(oracle, 0)[0].copy()
        rows.apply()
        X.traverse(root, decks, 1, 1, 0, 1, SEED, rows)
        rows.apply()
        _CACHE["trained_ref"] = rows
    return _CACHE["trained_ref"]


def deal3_iterate_ref(oracle):
    """the restatement's tables after one iteration at batch 1 on deck index 1 alone"""
    if "iterate" not in _CACHE:
        decks, root = deal3(oracle)
        rows = X.Rows()
        assert X.iterate(root, decks, 1, SEED, rows, 0, listed=[1]) == 2
        _CACHE["iterate"] = rows
    return _CACHE["iterate"]


def lanes_ref(oracle, trav, lanes, b0=0):
    """the restatement of a cut-0 launch on the LANES input that walks exactly the lanes listed (lane g: deck g / nb, traversal b0 + g % nb)"""
    w = LANES
    decks, _, st = deck_set(oracle, w["deck_seed"], w["r0"], w["n"], None)
    rows = X.Rows()
    for g in lanes:
        X.walk(X.root_on(st, decks[g // w["nb"]]), trav, (b0 + g % w["nb"]) & 0xFFFFFFFF, 0, SEED, rows, g // w["nb"])
    return rows


def edge_keys(oracle, deck_seed, r0):
    if ("keys", deck_seed, r0) not in _CACHE:
        decks, _, st = deck_set(oracle, deck_seed, r0)
        _CACHE["keys", deck_seed, r0] = X.subgame_keys(st, decks)
    return _CACHE["keys", deck_seed, r0]


def edge_ref(oracle, deck_seed, r0, name, trav, sigma_of=None):
    """((pairs, n_act, R, S) planted, Rows after X.traverse(trav, 0, 0, 4) on every deck with every planted pair touched, pairs met); name None: zero
    tables.  sigma_of: another rule in place of regret matching (a guard's wrong kernel), not cached"""
    key = ("edge", deck_seed, r0, name, trav)
    if key in _CACHE and sigma_of is None:
        return _CACHE[key]
    decks, _, st = deck_set(oracle, deck_seed, r0)
    keys = edge_keys(oracle, deck_seed, r0)
    planted = X.edge_rows(keys, name) if name else (keys, np.array([X.key_actions(k) for k in keys], np.int32), np.zeros((len(keys), 3)), np.zeros((len(keys), 3)))
    rows = X.Rows()
    rows.plant(planted[0], planted[2], planted[3])
    X.traverse(st, decks, trav, 0, 0, 4, SEED, rows, **({} if sigma_of is None else dict(sigma_of=sigma_of)))
    met = len(rows.count)
    rows.touch_all(keys)
    if sigma_of is None:
        _CACHE[key] = (planted, rows, met)
    return planted, rows, met


def threshold_tables(oracle):
    """(root, decks, [table, table]) on the round-4 set of deck 42: the root pair's strategy row at [1e-13, 0, 0] (below the threshold: uniform), then
    at [1e-11, 0, 3e-11] (above: a policy); a three-card row of the other player summing to 0.0 and a two-card row at [0, 1e-13] besides"""
    decks, _, st = deck_set(oracle, 42, 4)
    keys = [tuple(k) for k in edge_keys(oracle, 42, 4).tolist()]
    k_root = X.wide_key(X.root_on(st, decks[0]), 0)                        # (seat 0's hand is the same on every deck of the set)
    k3 = next(k for k in keys if (k[0] >> 62) & 1 == 1 and X.key_actions(k) == 3)
    k2 = next(k for k in keys if (k[0] >> 62) & 1 == 1 and X.key_actions(k) == 2)
    rest = {k3: [0.0, 0.0, 0.0], k2: [0.0, 1e-13, 0.0]}
    return st, decks, [{**rest, k_root: [1e-13, 0.0, 0.0]}, {**rest, k_root: [1e-11, 0.0, 3e-11]}]


def deal3_handle(ctx, sl, oracle, seed=SEED, capacity_log2=CAP):
    ctx.mccfr_seed(seed)
    return sl.FullChanceMCCFR(ctx, deal3(oracle)[0], None, capacity_log2)


TIMES = {}      # what of a timed launch -> seconds, printed by the tests that fill it (recorded in the module docstring)


def timed(what, fn, *args, **kw):
    t = time.perf_counter()
    fn(*args, **kw)
    TIMES[what] = time.perf_counter() - t
    print(f"{what}: {TIMES[what]:.3f} s on the device")


# ---- 1. the deal's root on three decks against the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trav", [0, 1])
def test_deal_one_traversal_by_every_cut(ctx, sl, oracle, trav):
    """nb = 1 on DEAL3 by every cut against ONE reference: at cut 0 the three decks are three lanes of one wavefront whose tables differ from round 2
    on (wide_key's table loop ends on the longest of them), at cut K three workgroups; the rows of rounds 0 and 1 are claimed and added to by all three"""
    rows, _ = deal3_ref(oracle, trav)
    assert (rows.choice, rows.terminal, len(rows.count)) == (DEAL3_VISITS[trav], DEAL3_TERMINALS, DEAL3_ROWS[trav])
    h = deal3_handle(ctx, sl, oracle)
    for n, cut in enumerate(CUTS):
        h.reset()
        h.cut(cut)
        timed(f"deal on 3 decks, traverser {trav}, cut {cut}, nb 1", h.traverse, trav, 0, 0, 1)
        keys, _ = assert_delta(h, rows, f"deal on 3 decks, traverser {trav}, cut {cut}")
        c = h.counters()
        assert (c["choice_visits"], c["terminal_visits"], c["dropped"]) == ((n + 1) * DEAL3_VISITS[trav], (n + 1) * DEAL3_TERMINALS, 0), (cut, c)
        assert c["rows"] == keys.shape[0] == len(rows.count)


def test_deal_iterate_bit_for_bit(ctx, sl, oracle):
    """cut 0, batch 1, deck index 1 alone: ONE lane makes every add of both halves in the restatement's order, and the second half's sigma is read from
    the rows the first applied: pairs, regret and strategy bit for bit.  Deck index 1, so that the tag's deck word and list[] are live"""
    rows = deal3_iterate_ref(oracle)
    h = deal3_handle(ctx, sl, oracle)
    h.cut(0)
    timed("deal, iterate(1, 1) on deck 1, cut 0", h.iterate, 1, 1, lists=[[1]])
    keys, _, R, S = h.tables_get()
    k_ref, R_ref = rows.arrays("R")
    assert keys.shape == k_ref.shape and np.array_equal(keys, k_ref), f"pair sets differ ({keys.shape[0]} rows against {k_ref.shape[0]})"
    assert same_bits(R, R_ref), "regret differs"
    assert same_bits(S, rows.arrays("S")[1]), "strategy differs"
    c = h.counters()
    one = (DEAL3_VISITS[0] + DEAL3_VISITS[1]) // 3
    assert (c["iterations"], c["choice_visits"], c["terminal_visits"], c["dropped"], c["rows"]) == (2, one, 2 * DEAL3_TERMINALS // 3, 0, keys.shape[0])
    _, counts, dR, dS = h.delta_get()
    assert not counts.any() and not dR.any() and not dS.any()


# ---- 2. a cut-0 launch of three workgroups -----------------------------------------------------------------------------------------------------------------
def test_cut_0_across_workgroups(ctx, sl, oracle):
    """nb = 33 on four decks below a round-5 root: 132 lanes, two full workgroups and 4 lanes of a third, a deck boundary inside a wavefront at lanes
    33, 66 and 99; then decks [3, 1] listed (66 lanes) with ids ending at 2^32 - 1.  Cut 0 against the restatement, then against cuts -1 and 1"""
    w = LANES
    nb = w["nb"]
    for listed, b0 in ((None, 0), ((3, 1), (1 << 32) - nb)):
        n_decks = w["n"] if listed is None else len(listed)
        for trav in range(2):
            rows = ref_delta(oracle, w["deck_seed"], w["r0"], trav, 0, b0, nb, SEED, listed=listed, n=w["n"], fix_seat=None)
            assert (rows.choice, rows.terminal) == (n_decks * nb * F.shape_counts(5)[trav], n_decks * nb * 6)
            h, _, _ = solver_of(ctx, sl, oracle, w["deck_seed"], w["r0"], n=w["n"], fix_seat=None)
            got = {}
            for n, cut in enumerate((0, -1, 1)):
                h.reset()
                h.cut(cut)
                h.traverse(trav, 0, b0, nb, None if listed is None else list(listed))
                assert_delta(h, rows, f"{n_decks * nb} lanes, traverser {trav}, cut {cut}")
                got[cut] = h.delta_get()
                c = h.counters()
                assert (c["choice_visits"], c["terminal_visits"], c["dropped"]) == ((n + 1) * rows.choice, (n + 1) * rows.terminal, 0)
            for cut in (-1, 1):
                assert np.array_equal(got[0][0], got[cut][0]) and np.array_equal(got[0][1], got[cut][1]) and same_bits(got[0][3], got[cut][3]), cut
            h.close()


# ---- 3. edge regret rows on every pair of a sub-game ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", E.FINITE_TABLES)
@pytest.mark.parametrize("deck_seed,r0", EDGE_ROOTS)
def test_edge_rows_on_every_pair(ctx, sl, oracle, deck_seed, r0, name):
    """every pair of the sub-game on the four decks holds a row of the edge table: the walk reads them through fw_claim / fw_find, fm_row and fm_pick at
    slots in ascending card id, by cut 0 and by the default cut"""
    h, _, _ = solver_of(ctx, sl, oracle, deck_seed, r0)
    for trav in range(2):
        planted, rows, _ = edge_ref(oracle, deck_seed, r0, name, trav)
        for cut in (0, -1):
            what = f"{name}, deck {deck_seed}, round {r0}, traverser {trav}, cut {cut}"
            h.cut(cut)
            h.tables_set(*planted)
            h.traverse(trav, 0, 0, 4)
            keys, counts = assert_delta(h, rows, what)
            assert keys.shape[0] == planted[0].shape[0] == h.counters()["rows"] and counts.sum() == 4 * 4 * F.shape_counts(r0)[trav]
            if name == "subnormal":
                # sigma of a kept 5e-324: uniform over the NON-ZERO cells (a flushed one: uniform over every cell, and other draws)
                _, _, _, dS = h.delta_get()
                opp = (((keys[:, 0] >> np.uint64(62)) & np.uint64(1)) != trav) & (counts > 0)
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


# ---- 4. the match at its edges -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def trained(ctx, sl, oracle):
    """a store trained at the deal on DEAL3, iterate(1, 1) at the default cut, and the agent's table read back from it (no dependence on the tests above)"""
    h = deal3_handle(ctx, sl, oracle)
    if "trained" not in _CACHE:
        h.iterate(1, 1)
        _CACHE["trained"] = h.tables_get()
    else:
        h.tables_set(*_CACHE["trained"])                                  # the same store for every case, trained once
    ctx.mccfr_seed(W.WIDE_SEED)                                           # ... and matched under both key words
    keys, _, _, S = h.tables_get()
    assert keys.shape[0] > DEAL3_ROWS[0] and (S.sum(1) > 1e-12).sum() > 10000   # more rows than the first half alone leaves, and policies among them
    decks, root = deal3(oracle)
    return h, root, decks, {tuple(k): [float(x) for x in s] for k, s in zip(keys.tolist(), S)}


@pytest.mark.parametrize("n", MATCH_NS)
def test_match_shapes(trained, oracle, n):
    """from the deal (36 plies, pairs of every round), an odd n, n below, at and above a block of 64, the seat split inside the second block, the last
    stream id accepted; on the handle's decks, on ONE held-out deck and on five (more decks than episodes at n = 1, 2 and 3): every episode's reward
    and all six sums"""
    h, root, decks, table = trained
    before = (h.tables_get(), h.counters())
    cases = [(None, decks, n), (held_out_deal(oracle, 1), None, n), (held_out_deal(oracle, 5), None, n)]
    if n == 2:
        cases.append((held_out_deal(oracle, 5), None, 3))
    for held, own, m in cases:
        ds = own if held is None else held
        sums, r2 = h.match(m, MATCH_STREAM, held, per_episode=True)
        want_sums, want_r2 = X.match(root, ds, table, m, W.WIDE_SEED, MATCH_STREAM)
        assert r2.dtype == np.int8 and np.array_equal(r2, want_r2), f"episodes of n = {m} on {len(ds)} decks"
        assert np.array_equal(sums, want_sums) and np.array_equal(h.match(m, MATCH_STREAM, held), sums)
    assert same_store(h.tables_get(), before[0]) and h.counters() == before[1]               # the match never inserts


def test_match_threshold(ctx, sl, oracle):
    """the match's own copy of the average policy's rule: strategy rows summing to 0.0 and to 1e-13 are played uniformly, one summing to 4e-11 is not"""
    st, decks, tables = threshold_tables(oracle)
    h, _, _ = solver_of(ctx, sl, oracle, 42, 4, capacity_log2=10, seed=W.WIDE_SEED)
    for n, table in enumerate(tables):
        keys = np.array(sorted(table), np.uint64)
        S = np.array([table[tuple(k)] for k in keys.tolist()])
        h.tables_set(keys, [X.key_actions(k) for k in keys], np.zeros_like(S), S)
        sums, r2 = h.match(129, MATCH_STREAM, per_episode=True)
        want_sums, want_r2 = X.match(st, decks, table, 129, W.WIDE_SEED, MATCH_STREAM)
        assert np.array_equal(r2, want_r2) and np.array_equal(sums, want_sums), f"table {n}"


def test_match_refuses_a_stream_id_of_25_bits(trained, oracle, sl):
    h, _, _, _ = trained
    h.traverse(0, 2, 0, 1)                                                # increments left unapplied: they are part of what must stay
    before = (h.tables_get(), h.delta_get(), h.counters())
    assert before[1][1].any()
    for held in (None, held_out_deal(oracle, 2)):
        for per_episode in (False, True):
            with pytest.raises(sl.ScopaError) as e:
                h.match(129, 1 << 24, held, per_episode=per_episode)
            assert e.value.status == sl.SCOPA_EINVAL
    assert same_store(h.tables_get(), before[0]) and same_store(h.delta_get(), before[1]) and h.counters() == before[2]
    assert h.match(2, MATCH_STREAM).any() or h.match(64, MATCH_STREAM).any()          # ... and the handle goes on


# ---- 5. host checks ------------------------------------------------------------------------------------------------------------------------------------------
def test_round_0_create_checks(ctx, sl, oracle):
    """at round 0 the root's table is the deck's first four cards IN ORDER; below a later root only the cards from position 4 + 6 round on are checked"""
    decks, _ = deal3(oracle)
    order = decks.copy()
    order[1, [0, 1]] = order[1, [1, 0]]                                   # the same four table cards, two of them swapped
    stock = decks.copy()
    stock[2, [2, 30]] = stock[2, [30, 2]]                                 # a table card swapped with a stock card
    for bad in (order, stock):
        with pytest.raises(sl.ScopaError) as e:
            sl.FullChanceMCCFR(ctx, bad, None, 10)
        assert e.value.status == sl.SCOPA_EINVAL
    ps, rng = sl.FullState(deck=decks[0]), np.random.RandomState(2)
    for _ in range(12):                                                   # two whole rounds, which all three decks deal alike
        legal = ps.legal()
        ps.step(int(legal[rng.randint(len(legal))]))
    later = sl.FullChanceMCCFR(ctx, order, ps.s, 10)                      # the first-four swap is accepted below a round-2 root
    assert int(later.root[0]["round"]) == 2
    with pytest.raises(sl.ScopaError) as e:
        sl.FullChanceMCCFR(ctx, stock, ps.s, 10)                          # (position 30 is past 4 + 6 * 2: still refused)
    assert e.value.status == sl.SCOPA_EINVAL
    later.close()
    h = sl.FullChanceMCCFR(ctx, decks, None, 10)
    for bad in (order, stock):
        with pytest.raises(sl.ScopaError) as e:
            h.match(64, 0, bad)
        assert e.value.status == sl.SCOPA_EINVAL
    assert h.match(64, 0, order[[0, 2]]).any()                            # the untouched decks of the same array are played
    h.close()


def test_rows_out_room(ctx, sl, oracle):
    """tables_get / delta_get with too little room: SCOPA_EINVAL, the needed count in *n_rows, nothing written; the count alone with every array NULL"""
    L, p = sl.lib(), sl._ptr
    w = LANES
    h, _, _ = solver_of(ctx, sl, oracle, w["deck_seed"], w["r0"], n=w["n"], fix_seat=None)
    empty = C.c_int64(-7)
    for fn in (L.scopa_full_chance_tables_get, L.scopa_full_chance_delta_get):
        assert fn(h._h, C.byref(empty), None, None, None, None) == sl.SCOPA_OK and empty.value == 0
        empty.value = 0
        one = np.full((1, 2), 0x5A5A5A5A5A5A5A5A, np.uint64)
        assert fn(h._h, C.byref(empty), p(one), None, None, None) == sl.SCOPA_OK and empty.value == 0 and (one == 0x5A5A5A5A5A5A5A5A).all()
        empty.value = -7
    h.traverse(0, 0, 0, 4)
    rows = h.counters()["rows"]
    assert rows > 8
    sent_u, sent_f = 0x5A5A5A5A5A5A5A5A, -12345.5
    for fn, third in ((L.scopa_full_chance_tables_get, True), (L.scopa_full_chance_delta_get, False)):
        n = C.c_int64(0)
        assert fn(h._h, C.byref(n), None, None, None, None) == sl.SCOPA_OK and n.value == rows          # the count alone
        keys, a, b = np.full((rows, 2), sent_u, np.uint64), np.full((rows, 3), sent_f), np.full((rows, 3), sent_f)
        x = np.full(rows, 0x5A5A5A5A, np.int32 if third else np.uint32)
        args = (p(keys), p(x), p(a), p(b)) if third else (p(keys), p(a), p(b), p(x))
        n = C.c_int64(rows - 1)
        assert fn(h._h, C.byref(n), *args) == sl.SCOPA_EINVAL
        assert n.value == rows and (keys == sent_u).all() and (a == sent_f).all() and (b == sent_f).all() and (x == 0x5A5A5A5A).all()
        n = C.c_int64(rows)
        assert fn(h._h, C.byref(n), *args) == sl.SCOPA_OK and n.value == rows
        assert not (keys == sent_u).any() and not (a == sent_f).any() and not (b == sent_f).any() and not (x == 0x5A5A5A5A).any()
        assert len({tuple(k) for k in keys.tolist()}) == rows
    h.close()
