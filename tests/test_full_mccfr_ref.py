"""CPU checks of the FullScopa sampling solver's yardstick, tests/full_mccfr_ref.py, and of the host-side entry points (no GPU).

The reference has no solver that runs on FullScopa, so the restatement is held to three things that do not come from the code under test: the
reference's own infoset strings (key), the visit counts that follow from the ply order (shape), and exact enumeration of the counterfactual regrets
(unbiasedness)."""
import ctypes as C

import numpy as np
import pytest

import full_mccfr_ref as F
import mccfr_edges as E
import philox_words as W
import test_gpu_full_depth as GD                   # (fixture builders are plain CPU code; only the modules' tests carry the gpu mark)
import test_gpu_full_store as GS
from test_gpu_full_mccfr import in_budget, ref_delta, root_of

OTHER_DECK_SEEDS = (7, 1234, 99991)
SEED = 0x5C09A


def _decision_states(sl, oracle, deck, actions_of):
    """(product state, oracle state, mover) at every decision node of one playout; actions_of(oracle state) picks the move"""
    a, b = sl.FullState(deck=deck), oracle.FullState(perm=deck)
    while not b.is_terminal():
        yield a, b, b.current_player()
        act = actions_of(b)
        if act not in b.legal():
            return             # 16 of the fixture's playouts fuzz the engine with cards the mover does not hold: a no-op ply, after which the mover no longer
                               # tells the hand sizes -- states no game reaches, and no infoset of the solver (the key's contract is over play)
        a.step(act); b.step(act)


def _check_bucket(sl, bucket, deck):
    """one (deck, player) bucket of (key, string): equality of keys <=> equality of strings, and the Python decode gives the string back"""
    by_key, by_string = {}, {}
    for key, string in bucket:
        assert key != 0 and key >> 63 == 1
        assert by_key.setdefault(key, string) == string, "one key, two strings"
        assert by_string.setdefault(string, key) == key, "one string, two keys"
    for key, string in by_key.items():
        assert sl.full_key_to_string(key, deck) == string == F.key_to_string(key, deck)
    return len(by_key)


def test_key_equality_is_string_equality(sl, oracle, golden):
    """Every decision state of the 48 reference playouts and of 2 010 random playouts on three other decks, bucketed by (deck, player to move)."""
    g = golden.json("full_scopa.json")
    playouts = []
    for c in g["playouts"]:
        it = iter(c["actions"])
        playouts.append((np.array(g["deals"][str(c["seed"])], np.uint8), lambda b, it=it: next(it)))
    rng = np.random.RandomState(5)
    for s in OTHER_DECK_SEEDS:
        deck = oracle.full_deal_py_seed(s)
        for _ in range(670):
            playouts.append((deck, lambda b: int(b.legal()[rng.randint(len(b.legal()))])))
    buckets, n_states = {}, 0
    for deck, pick in playouts:
        for a, b, p in _decision_states(sl, oracle, deck, pick):
            key = sl.full_infoset_key(a, deck, p)
            assert key == F.key_of(b, p)                                       # the restatement's packing is the library's
            assert a.infoset_string(p) == b.infoset_string(p)
            buckets.setdefault((deck.tobytes(), p), []).append((key, b.infoset_string(p)))
            n_states += 1
    assert 36 * (len(playouts) - 16) <= n_states <= 36 * len(playouts) and len(buckets) == 2 * len({d.tobytes() for d, _ in playouts})
    distinct = sum(_check_bucket(sl, bucket, np.frombuffer(d, np.uint8)) for (d, p), bucket in buckets.items())
    assert distinct > 20000 and distinct < n_states                           # keys recur within a bucket: the equivalence is exercised both ways


def test_key_argument_errors(sl):
    L, st = sl.lib(), sl.FullState(seed=42)
    key = C.c_uint64()
    ok = lambda s, d, p, k: L.scopa_full_infoset_key(s, d, p, k)
    sp, dp = sl._ptr(st.s), sl._ptr(st.deck)
    assert ok(sp, dp, 0, C.byref(key)) == sl.SCOPA_OK and key.value >> 63 == 1
    assert ok(None, dp, 0, C.byref(key)) == ok(sp, None, 0, C.byref(key)) == ok(sp, dp, 0, None) == sl.SCOPA_EINVAL
    assert ok(sp, dp, 2, C.byref(key)) == ok(sp, dp, -1, C.byref(key)) == sl.SCOPA_EINVAL
    bad = st.deck.copy(); bad[0] = bad[1]
    assert ok(sp, sl._ptr(bad), 0, C.byref(key)) == sl.SCOPA_EINVAL


def test_philox_uniform_is_u53_of_the_first_two_words(oracle):
    """the draw the restatement uses, against the Philox words and the u53 formula the other FullScopa tests spell out"""
    for seed, ctr in ((SEED, (35 << 16 | 46655, 0xFFFFFFFF, 0x80000000, 161)), (0x9E3779B97F4A7C15, (7, 1 << 31, 3, 176))):
        x = oracle.philox4x32_10(list(ctr), [seed & 0xFFFFFFFF, seed >> 32])
        assert oracle.philox_uniform(seed, *ctr) == ((int(x[0]) >> 5) * 67108864.0 + (int(x[1]) >> 6)) / 9007199254740992.0


@pytest.mark.parametrize("r0", [4, 3, 2])
def test_shape_counts(oracle, r0):
    """13 S / 8 S choice visits and 6^(6 - r0) terminals per traversal, S = (6^(6 - r0) - 1) / 5: the header's formula, here from the walk itself"""
    root, _ = F.random_root(oracle.full_deal_py_seed(42), r0, np.random.RandomState(r0))
    for trav in range(2):
        rows = F.Rows()
        F.walk(root, trav, 3, 1, SEED, rows)
        assert (rows.choice, rows.terminal) == (F.shape_counts(r0)[trav], F.shape_counts(r0)[2])
        assert sum(rows.count.values()) == rows.choice
    assert F.shape_counts(0) == (121303, 74648, 46656)


@pytest.mark.parametrize("trav", [0, 1])
def test_walk_is_unbiased_against_exact_enumeration(oracle, trav):
    """A round-4 root (1 296 histories), uniform frozen sigma: the mean d_regret row of 4 096 traversals at fixed seeds against the exactly enumerated
    counterfactual regret of every traverser infoset, every cell within 5 standard errors computed from the per-traversal increments themselves.
    Largest |mean - exact| / standard error at these seeds: 2.52 over 49 rows (traverser 0), 2.32 over 90 rows (traverser 1)."""
    root, _ = F.random_root(oracle.full_deal_py_seed(42), 4, np.random.RandomState(11))
    exact = F.exact_regret(root, trav)
    n = 4096
    keys = sorted(exact)
    col = {k: i for i, k in enumerate(keys)}
    inc = np.zeros((n, len(keys), 3))
    for t in range(n):
        rows = F.Rows()
        F.walk(root, trav, t, 0, SEED, rows, uniform=True)
        for k, d in rows.dR.items():
            if (k >> 62) & 1 == trav:
                inc[t, col[k]] = d                                             # (a key outside `exact` would be a KeyError: the key sets agree)
    mean, se = inc.mean(0), inc.std(0, ddof=1) / np.sqrt(n)
    want = np.array([exact[k] for k in keys])
    err = np.abs(mean - want)
    sure = se == 0.0                                                           # a cell every traversal gives the same increment
    assert (err[sure] <= 1e-12).all()
    ratio = err[~sure] / se[~sure]
    print("rows", len(keys), "largest |mean - exact| / se:", ratio.max())
    assert len(keys) >= 10 and (~sure).sum() >= 20
    assert (ratio <= 5.0).all()


def test_null_handle_is_refused_before_the_device(sl):
    """tables_set / tables_get and the rest: a NULL handle is SCOPA_EINVAL; create refuses a NULL context, deck or result"""
    L = sl.lib()
    n = C.c_int64(4)
    keys, act, tab = np.zeros(4, np.uint64), np.zeros(4, np.int32), np.zeros((4, 3))
    p = sl._ptr
    assert L.scopa_full_mccfr_tables_get(None, C.byref(n), p(keys), p(act), p(tab), p(tab)) == sl.SCOPA_EINVAL and n.value == 4
    assert L.scopa_full_mccfr_delta_get(None, C.byref(n), p(keys), p(tab), p(tab), p(act)) == sl.SCOPA_EINVAL
    assert L.scopa_full_mccfr_tables_set(None, 4, p(keys), p(act), p(tab), p(tab)) == sl.SCOPA_EINVAL
    for fn in (L.scopa_full_mccfr_destroy, L.scopa_full_mccfr_reset, L.scopa_full_mccfr_apply):
        assert fn(None) == sl.SCOPA_EINVAL
    assert L.scopa_full_mccfr_traverse(None, 0, 0xFFFFFFFF, 0xFFFFFFFF, 0) == sl.SCOPA_EINVAL
    assert L.scopa_full_mccfr_iterate(None, 0xFFFFFFFF, 1) == sl.SCOPA_EINVAL
    assert L.scopa_full_mccfr_cut(None, 0) == L.scopa_full_mccfr_root(None, None, None, None) == sl.SCOPA_EINVAL
    assert L.scopa_full_mccfr_counters(None, None, None, None, None, None) == sl.SCOPA_EINVAL
    assert L.scopa_full_mccfr_match(None, 1, 0, p(np.zeros(6, np.int64)), None) == sl.SCOPA_EINVAL
    h = C.c_void_p()
    assert L.scopa_full_mccfr_create(None, p(sl.full_deal_py_seed(42)), None, 10, C.byref(h)) == sl.SCOPA_EINVAL and not h.value


def test_planted_row_with_one_positive_regret_is_never_left(oracle):
    """the restatement's counts show what the GPU test relies on: under a regret row with one positive entry the opponent always plays that slot"""
    root, _ = F.random_root(oracle.full_deal_py_seed(42), 4, np.random.RandomState(11))
    key = F.key_of(root, 0)
    rows = F.Rows()
    rows.plant([key], [[0.0, 2.5, -1.0]], [[0.0, 0.0, 0.0]])
    F.traverse(root, 1, 0, 0, 32, SEED, rows)
    after = {F.key_of(F.child(root, c), 1) for c in F.hand(root, 0)}
    met = {k for k in rows.count if (k >> 62) & 1 == 1 and (k >> 59) & 7 == 4 and F.key_actions(k) == 3}
    assert rows.dS[key] == [0.0, 32.0, 0.0] and met == {F.key_of(F.child(root, F.hand(root, 0)[1]), 1)} and len(after) == 3


# ---- guards of the built stores of tests/test_gpu_full_store.py: the inputs do what that file claims, before a kernel is involved -----------------------
LAUNCHES_R3 = ((42, 0), (7, 1), (42, 1), (7, 0))                             # (deck seed, traverser) at round 3, nb 8


def _first_node_keys(rows, trav, r0):
    return [k for k in rows.count if (k >> 62) & 1 != trav and (k >> 59) & 7 == r0 and F.key_actions(k) == 3]


def test_home_slot_and_fillers():
    """splitmix64's finaliser on its published test vector (seed 0: the first output is the finaliser of the golden gamma), and fillers as specified"""
    assert int(F.fm_hash(np.uint64(0x9E3779B97F4A7C15))[0]) == (0xE220A8397B1DCDAF ^ (0xE220A8397B1DCDAF >> 32)) & 0xFFFFFFFF
    assert F.home_slot(np.uint64(1 << 63), 4) == int(F.home_slot(np.array([1 << 63], np.uint64), 4)[0]) < 16
    for home, n, c, tag in ((0, 10, 10, 2), (1021, 64, 10, 1), (3, 16, 4, 255), (123456, 64, 18, 7)):
        f = F.fillers(home, n, c, tag)
        assert f.dtype == np.uint64 and np.unique(f).size == n and (F.home_slot(f, c) == home).all()
        assert all(k >> 56 == 0xBF and k & 0xFFFF == 0 and (k >> 48) & 0xFF == tag and F.key_actions(k) == 3 for k in f.tolist())
        assert np.array_equal(f[:5], F.fillers(home, 5, c, tag))
    R, S = F.rows_for(F.fillers(5, 64, 10, 1))
    assert R.min() >= 1.0 and S.min() >= 2.125 and np.unique(R, axis=0).shape[0] == 64 and not (R == S).any()
    assert F.rows_for([(1 << 63) | (0b101 << 56) | (0x0302 << 16)])[0].tolist() == [[3.0, 4.25, 0.0]]


def test_store_model_and_what_is_sure_in_every_order():
    """the sequential probe length depends on the insertion order, the occupied set and reach do not: the GPU tests are guarded by reach"""
    (both, _), a = GS.overfull_stores()["touch"], 40
    first, second = F.Store(10).insert(both[:a]).insert(both[a:]), F.Store(10).insert(both[a:]).insert(both[:a])
    assert (first.longest_probe(), second.longest_probe()) == (60, 80) and set(first.slots) == set(second.slots) == set(range(GS.TOUCH_HOME, GS.TOUCH_HOME + 80))
    assert first.longest_reach() == second.longest_reach() == 80 > F.MAX_PROBE            # 40 + 40 touching: held whole only in some orders
    wrap, reachable = GS.overfull_stores()["wrap"]
    st = F.Store(10).insert(wrap)
    assert st.longest_probe() == 71 and wrap.size == 74 > reachable == len({(h + i) & 1023 for h in F.home_slot(wrap, 10).tolist() for i in range(64)})
    for name, (size, probe, reach) in dict(chain=(64, 64, 64), wrap64=(64, 64, 64), wrap=(64, 61, 64), touch=(64, 44, 64), ten=(10, 10, 10)).items():
        keys = GS.small_stores()[name]
        for order in (keys, keys[::-1]):
            st = F.Store(10).insert(order)
            assert (len(st.slots), st.longest_reach()) == (size, reach) and st.longest_probe() <= reach <= F.MAX_PROBE, name
        assert F.Store(10).insert(keys).longest_probe() == probe, name
    assert set(F.Store(10).insert(GS.small_stores()["wrap"]).slots) == set(range(1021, 1024)) | set(range(61))
    # a 65th key of the chain's home has nowhere to go, and the 10 keys set after it share no slot with the chain
    assert F.Store(10).insert(F.fillers(512, 65, 10, 5)).longest_probe() == 65 and set(F.home_slot(GS.small_stores()["ten"], 10).tolist()) == {100}


def test_mixed_load_guard():
    """640 keys in 1 024 slots under the fixed seed: the longest run of occupied slots, which bounds every probe in every order, is far below 64"""
    keys = GS.small_stores()["mixed"]
    st = F.Store(10).insert(keys)
    print("mixed load: longest probe of the model", st.longest_probe(), "longest reach", st.longest_reach())
    assert np.unique(keys).size == 640 and all(k >> 56 == 0xBF for k in keys.tolist())
    assert st.longest_probe() < 64 and st.longest_reach() < 64
    assert st.longest_reach() == 35                                           # recorded: numpy's RandomState streams do not change


def test_isolation_at_round_3(oracle):
    """2^18 slots: the key of the opponent's first node of the round is isolated in all four launches, and more than 100 traverser keys met more than
    once are; at 2^16 the first three launches have such a first-node key that is not: the GPU tests use 2^18"""
    for n, (deck_seed, trav) in enumerate(LAUNCHES_R3):
        rows = ref_delta(oracle, deck_seed, 3, trav, 0, 0, 8, SEED)
        met, first = list(rows.count), _first_node_keys(rows, trav, 3)
        assert 1 <= len(first) <= (1 if trav else 3) and all(F.isolated(k, met, 18) for k in first)
        assert trav == 0 or first == [F.key_of(root_of(oracle, deck_seed, 3)[2], 0)]
        assert sum(1 for k in met if (k >> 62) & 1 == trav and rows.count[k] > 1 and F.isolated(k, met, 18)) > 100
        assert n == 3 or not all(F.isolated(k, met, 16) for k in first)
        assert F.Store(18).insert(met).longest_reach() <= 4                  # the launch alone: no probe of any length


@pytest.mark.parametrize("deck_seed,trav", GS.BLOCKED_LAUNCHES)
def test_blocked_keys_guard(oracle, deck_seed, trav):
    fx = GS.blocked_launch(oracle, deck_seed, trav)
    met = list(fx.base.count)
    assert None not in fx.blocked and len(set(fx.blocked)) == 2 and all(F.isolated(k, met, 18) for k in fx.blocked)
    assert (fx.blocked[0] >> 62) & 1 == trav and fx.base.count[fx.blocked[0]] > 1 and fx.blocked[1] in _first_node_keys(fx.base, trav, 3)
    assert trav == 0 or fx.blocked[1] == F.key_of(fx.root, 0)                # the root itself: in the prefix of every cut > 0
    assert set(fx.rows.count) == set(met) - set(fx.blocked) and not np.isin(fx.fill, np.array(met, np.uint64)).any()
    assert fx.rows.dropped == sum(fx.base.count[k] for k in fx.blocked) and (fx.rows.choice, fx.rows.terminal) == (fx.base.choice, fx.base.terminal)
    assert fx.rows.count == {k: n for k, n in fx.base.count.items() if k not in fx.blocked}
    # the store of the test: the two chains fill h .. h + 63 exactly, a blocked key finds no room, every other key of the launch does
    st = F.Store(18).insert(fx.fill)
    for k in fx.blocked:
        h = F.home_slot(np.uint64(k), 18)
        assert st.reach(k) == 64 and all(((h + i) & (2 ** 18 - 1)) in st.slots for i in range(64))
    st.insert(sorted(fx.rows.count))
    assert max(st.reach(k) for k in fx.rows.count) <= 4 and st.longest_reach() == 64
    print("blocked", deck_seed, trav, [hex(k) for k in fx.blocked], "dropped per launch", fx.rows.dropped)


def test_planted_chains_guard(oracle):
    fx = GS.chained_planted(oracle)
    assert None not in list(fx.K), "no isolated candidate for a planted row"
    K = fx.K.tolist()
    assert K[0] == F.key_of(fx.root, 0) and [F.key_actions(k) for k in K] == list(fx.n_act) and [(k >> 62) & 1 for k in K] == [0, 1, 0, 1]
    launch = set(fx.zero) | set(K)
    for rows in fx.launch:
        launch |= set(rows.count)
    assert all(F.isolated(k, launch, 18) for k in K) and not np.isin(fx.fill, np.array(sorted(launch), np.uint64)).any()
    assert fx.fill.size == np.unique(fx.fill).size == 252
    st = F.Store(18).insert(np.concatenate([fx.K, fx.fill]))
    assert len(st.slots) == 256 and all(st.reach(k) == 64 for k in K)
    st.insert(sorted(launch - set(K)))
    assert st.longest_reach() == 64 and max(st.reach(k) for k in launch - set(K)) <= 4
    assert fx.launch[1].dS[K[0]] == [0.0, 24.0, 0.0]
    print("planted", [hex(k) for k in K])


def test_root_key_behind_63_fillers_guard(oracle):
    """the two stores built around the root key of (deck 42, round 4): at 2^18 slots it is claimed in the 64th slot of its probe and no key of the
    zero-table launches is near; at 2^6 slots its home is not slot 0, so a full chain wraps, and its planted strategy row changes the restated match"""
    fx = GS.chained_planted(oracle)
    k_root = F.key_of(fx.root, 0)
    st = F.Store(18).insert(F.fillers(F.home_slot(np.uint64(k_root), 18), 63, 18, 9)).insert([k_root])
    assert st.probe[k_root] == st.reach(k_root) == 64 and F.isolated(k_root, fx.zero, 18)
    assert 0 < F.home_slot(np.uint64(k_root), 6) < 64
    with_row, without = (F.match(fx.root, t, 129, W.WIDE_SEED, GS.MATCH_STREAM)[1] for t in ({k_root: [0.25, 0.5, 2.0]}, {}))
    assert not np.array_equal(with_row, without)


def test_match_streams_separate(oracle):
    """the restated match under stream (1 << 24) - 1 and under that id without its top byte: different episodes, so the GPU comparison would notice"""
    fx = GS.chained_planted(oracle)
    table = {int(k): [float(x) for x in s] for k, s in zip(fx.K, fx.S)}
    wide, narrow = (F.match(fx.root, table, 129, W.WIDE_SEED, s) for s in (GS.MATCH_STREAM, 0xFFFF))
    assert GS.MATCH_STREAM == (1 << 24) - 1 and not np.array_equal(wide[1], narrow[1]) and not np.array_equal(wide[0], narrow[0])


# ---- guards of tests/test_gpu_full_depth.py: its inputs can tell a wrong kernel from a right one, shown on the restatement alone -------------------------
def test_deal_capacity_guard(oracle):
    """the key sets of the deal-root launches at 2^18 slots: no probe looks at more than 64 slots in any arrival order (the 46 340 keys of the two first
    traversals alone reach 11 slots at 2^18, 24 at 2^17 and 101 at 2^16: measured once, not asserted)"""
    walks = [GD.deal_ref(oracle, trav) for trav in range(2)]
    assert [len(r.count) for r in walks] == [30533, 27004] and [sum(1 for n in r.count.values() if n > 1) for r in walks] == [19547, 14244]
    assert max(max(r.count.values()) for r in walks) == 134
    both = sorted(set(walks[0].count) | set(walks[1].count))
    assert len(both) == 46340
    trained = set(GD.deal_iterate_ref(oracle).R)                            # iterate(1, 1): the second half walks under the first half's regrets
    assert trained != set(both) and set(walks[0].count) < trained
    # one store of every key any of those launches meets: a probe in a store of fewer keys looks at no more slots than in this one
    reach = F.Store(GD.CAP).insert(sorted(trained | set(both))).longest_reach()
    print("deal-root key sets,", len(trained | set(both)), "keys at 2^%d slots: longest reach" % GD.CAP, reach)
    assert GD.CAP == 18 and reach <= 64
    for deck_seed, r0 in GD.EDGE_ROOTS:
        keys = GD.edge_ref(oracle, deck_seed, r0, None, 0)[0][0]
        assert F.Store(14).insert(keys).longest_reach() <= 64
        assert (deck_seed, r0) not in ((42, 4), (42, 3)) or keys.size == {4: 229, 3: 915}[r0]


def test_deal_q_word_separates(oracle, monkeypatch):
    """traverser 0 from the deal draws at ply 33 with q up to 6^6 - 1 = 46 655: with q cut to 15 bits in the draw's counter word the restatement's
    d_regret leaves the reorder budget (the counts do not move: the draw picks between two last cards), so the GPU comparison would notice"""
    ref = GD.deal_ref(oracle, 0)
    draw = oracle.philox_uniform
    monkeypatch.setattr(F.O, "philox_uniform", lambda seed, c0, *rest: draw(seed, (c0 & ~0xFFFF) | (c0 & 0x7FFF), *rest))
    cut = F.Rows()
    F.walk(GD.deal_root(oracle)[1], 0, 0, 0, SEED, cut)
    monkeypatch.undo()
    assert np.array_equal(cut.arrays("count")[0], ref.arrays("count")[0])
    assert not in_budget(cut.arrays("dR")[1], ref.arrays("dR")[1], ref.arrays("A")[1], "q cut to 15 bits against q whole")


@pytest.mark.parametrize("deck_seed,r0", GD.EDGE_ROOTS)
def test_edge_rows_guard(oracle, deck_seed, r0):
    """every finite edge table planted over every key of the sub-game: finite increments; every table but allneg moves the d_regret image or the key set
    away from the zero-table run's; allneg IS the zero-table run for traverser 0 (the uniform fallback); onehot meets far fewer rows; a subnormal
    table flushed to zero would be the zero table, which it separates from"""
    zero = [GD.edge_ref(oracle, deck_seed, r0, None, trav) for trav in range(2)]
    image = lambda rows: (rows.arrays("count"), rows.arrays("dR")[1].tobytes(), rows.arrays("dS")[1].tobytes())
    same = lambda a, b: np.array_equal(a[0][0], b[0][0]) and np.array_equal(a[0][1], b[0][1]) and a[1:] == b[1:]
    for name in E.FINITE_TABLES:
        runs = [GD.edge_ref(oracle, deck_seed, r0, name, trav) for trav in range(2)]
        for trav in range(2):
            planted, rows, met = runs[trav]
            assert all(np.isfinite(rows.arrays(w)[1]).all() for w in ("dR", "dS")) and len(rows.count) == planted[0].size, name
            assert rows.choice == 8 * F.shape_counts(r0)[trav]
        differs = [not same(image(runs[trav][1]), image(zero[trav][1])) for trav in range(2)]
        if name == "allneg":
            assert not differs[0]
        else:
            assert any(differs), name
        print(deck_seed, r0, name, "rows met", [r[2] for r in runs], "of", runs[0][0][0].size, "differs from zero tables", differs)
    hot, none = GD.edge_ref(oracle, deck_seed, r0, "onehot", 0)[2], zero[0][2]
    assert 2 * hot < none and ((deck_seed, r0) != (42, 3) or (hot, none) == (126, 790))
    sub = GD.edge_ref(oracle, deck_seed, r0, "subnormal", 0)[0][2]
    assert (sub == 5e-324).any() and ((sub == 0.0).sum(1) > 3 - GD.edge_ref(oracle, deck_seed, r0, "subnormal", 0)[0][1]).any()
    assert F.sigma_of([5e-324, 0.0, 5e-324], 3) == [0.5, 0.0, 0.5] and F.sigma_of([5e-324] * 3, 3) == [1.0 / 3] * 3


def test_match_inputs_separate(oracle):
    """the match of tests/test_gpu_full_depth.py on the restated trained store: the sums at n = 129 differ from an empty store's and from those of a
    stream id that lost its high byte or its two high bytes, and the episodes differ when the seat split moves by one (n = 64: what 2 i <= n does)"""
    root = GD.deal_root(oracle)[1]
    table = GD.deal_iterate_ref(oracle).S
    wide = F.match(root, table, 129, W.WIDE_SEED, GD.MATCH_STREAM)
    assert not np.array_equal(wide[0], F.match(root, {}, 129, W.WIDE_SEED, GD.MATCH_STREAM)[0])
    for narrow in ((1 << 16) - 1, (1 << 8) - 1):
        assert not np.array_equal(wide[0], F.match(root, table, 129, W.WIDE_SEED, narrow)[0]), narrow
    assert np.array_equal(wide[1], F.match(root, table, 129, W.WIDE_SEED, GD.MATCH_STREAM, split=65)[1])       # the rule: 2 i < 129 up to i = 64
    for split in (64, 66):
        assert not np.array_equal(wide[1], F.match(root, table, 129, W.WIDE_SEED, GD.MATCH_STREAM, split=split)[1]), split
    for n in (2, 64):                                                        # 2 i <= n: episode n / 2 in seat 0
        rule, moved = (F.match(root, table, n, W.WIDE_SEED, GD.MATCH_STREAM, split=s) for s in (None, n // 2 + 1))
        assert np.array_equal(rule[1], F.match(root, table, n, W.WIDE_SEED, GD.MATCH_STREAM, split=n // 2)[1])
        assert not np.array_equal(rule[1], moved[1]) or not np.array_equal(rule[0], moved[0]), n


def test_match_threshold_guard(oracle):
    """the planted rows of test_match_threshold: the 1e-13 row read as a policy (slot 0 always) gives other episodes than the rule (uniform), and the
    4e-11 row other episodes than uniform play"""
    root, (below, above) = GD.threshold_tables(oracle)
    k_root = F.key_of(root, 0)
    assert below[k_root] == [1e-13, 0.0, 0.0] and F.average_probs(below, k_root, 3) == [1.0 / 3] * 3 and F.average_probs(above, k_root, 3) == [0.25, 0.0, 0.75]
    assert sorted(F.average_probs(below, k, F.key_actions(k)) for k in below if k != k_root) == [[1.0 / 3] * 3, [0.5, 0.5]]
    run = lambda t: F.match(root, t, 129, W.WIDE_SEED, GD.MATCH_STREAM)[1]
    rule = run(below)
    assert np.array_equal(rule, run({})) and not np.array_equal(rule, run({**below, k_root: [1.0, 0.0, 0.0]}))
    assert not np.array_equal(run(above), rule)
    as_policy = {k: ([0.0, 1.0, 0.0] if v[1] else v) for k, v in below.items()}                 # the two-card row at [0, 1e-13]
    assert not np.array_equal(run(as_policy), rule)
