"""CPU checks of the FullScopa sampling solver's yardstick, tests/full_mccfr_ref.py, and of the host-side entry points (no GPU).

The reference has no solver that runs on FullScopa, so the restatement is held to three things that do not come from the code under test: the
reference's own infoset strings (key), the visit counts that follow from the ply order (shape), and exact enumeration of the counterfactual regrets
(unbiasedness)."""
import ctypes as C

import numpy as np
import pytest

import full_mccfr_ref as F

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
