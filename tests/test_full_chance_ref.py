"""CPU checks of the yardstick of FullScopa over a set of decks, tests/full_chance_ref.py, and of the host-side entry points (no GPU).

The restatement is held to what does not come from the code under test: the oracle's own infoset strings across decks (the key), exact enumeration
of the counterfactual regrets summed over decks (unbiasedness), and guards that the inputs of tests/test_gpu_full_chance.py separate a right kernel
from the wrong ones a two-word key and a deck in the draw make possible; the last section does the same for tests/test_gpu_full_chance_depth.py."""
import ctypes as C

import numpy as np
import pytest

import full_chance_ref as X
import full_mccfr_ref as F
import mccfr_edges as E
import philox_words as W
import test_gpu_full_chance as G                   # (fixture builders are plain CPU code; only the module's tests carry the gpu mark)
import test_gpu_full_chance_depth as GD
from scopa_amd.algorithms import packet_decks, sample_decks

SEED = 0x5C09A


# ---- 1. the key ---------------------------------------------------------------------------------------------------------------------------------------
def test_key_identity_across_decks(sl, oracle):
    """Random playouts on 8 decks -- two unrelated ones, the 4-deck packet seat 0 cannot tell apart at the start of round 4, and two decks that share
    the table alone -- in ONE bucket: pairs are equal exactly where the oracle's strings are equal, whatever the deck; the decode gives the string back; the library's host
    entry point equals the restatement.  Fails without scopa_full_infoset_key_wide."""
    deck42 = oracle.full_deal_py_seed(42)
    decks = [oracle.full_deal_py_seed(s) for s in (7, 1234)] + list(packet_decks(deck42, 4, 4, 5, fix_seat=0)) + list(packet_decks(deck42, 0, 2, 9))
    rng = np.random.RandomState(5)
    by_key, by_string, shared = {}, {}, {}
    for d, deck in enumerate(decks):
        for _ in range(150):
            a, b = sl.FullState(deck=deck), oracle.FullState(perm=deck)
            while not b.is_terminal():
                p = b.current_player()
                key, string = X.wide_key(b, p), b.infoset_string(p)
                assert key == sl.full_infoset_key_wide(a, p)
                assert key[0] >> 63 == 1 and (key[0] >> 56) & 7 == 0 and 0 < key[1] < 1 << 40 and X.key_actions(key) == len(b.legal())
                assert by_key.setdefault(key, string) == string, "one pair, two strings"
                assert by_string.setdefault(string, key) == key, "one string, two pairs"
                shared.setdefault(key, set()).add(d)
                legal = b.legal()
                act = int(legal[rng.randint(len(legal))])
                a.step(act); b.step(act)
    for key, string in by_key.items():
        assert sl.full_wide_key_to_string(*key) == string == X.key_to_string(key)
        f = sl.full_wide_key_fields(*key)
        assert f["hand"] == sorted(f["hand"]) and len(f["hand"]) == X.key_actions(key)
    n_shared = sum(len(v) > 1 for v in shared.values())
    print("pairs", len(by_key), "met on several decks", n_shared)
    assert len(by_key) > 5000 and n_shared > 10


def test_wide_key_refuses_what_the_one_word_key_refuses(sl):
    L = sl.lib()
    s = sl.FullState(seed=42)
    key2 = (C.c_uint64 * 2)()
    assert L.scopa_full_infoset_key_wide(sl._ptr(s.s), 0, C.byref(key2)) == 0 and key2[0] >> 63 == 1
    assert L.scopa_full_infoset_key_wide(None, 0, C.byref(key2)) == sl.SCOPA_EINVAL
    assert L.scopa_full_infoset_key_wide(sl._ptr(s.s), 0, None) == sl.SCOPA_EINVAL
    for player in (-1, 2):
        assert L.scopa_full_infoset_key_wide(sl._ptr(s.s), player, C.byref(key2)) == sl.SCOPA_EINVAL
    for field, value in (("round", 6), ("nt", 21)):
        bad = s.s.copy()
        bad[0][field] = value
        assert L.scopa_full_infoset_key_wide(sl._ptr(bad), 0, C.byref(key2)) == sl.SCOPA_EINVAL
    bad = s.s.copy()
    bad[0]["nh"][1] = 4
    assert L.scopa_full_infoset_key_wide(sl._ptr(bad), 0, C.byref(key2)) == sl.SCOPA_EINVAL


def test_null_handle_is_refused_before_the_device(sl):
    L = sl.lib()
    n = C.c_int64(4)
    keys, act, tab = np.zeros((4, 2), np.uint64), np.zeros(4, np.int32), np.zeros((4, 3))
    p = sl._ptr
    assert L.scopa_full_chance_tables_get(None, C.byref(n), p(keys), p(act), p(tab), p(tab)) == sl.SCOPA_EINVAL and n.value == 4
    assert L.scopa_full_chance_delta_get(None, C.byref(n), p(keys), p(tab), p(tab), p(act)) == sl.SCOPA_EINVAL
    assert L.scopa_full_chance_tables_set(None, 4, p(keys), p(act), p(tab), p(tab)) == sl.SCOPA_EINVAL
    for fn in (L.scopa_full_chance_destroy, L.scopa_full_chance_reset, L.scopa_full_chance_apply):
        assert fn(None) == sl.SCOPA_EINVAL
    assert L.scopa_full_chance_traverse(None, 0, 0xFFFFFFFF, 0xFFFFFFFF, 0, None, 0) == sl.SCOPA_EINVAL
    assert L.scopa_full_chance_iterate(None, 0xFFFFFFFF, 1, None, 0) == sl.SCOPA_EINVAL
    assert L.scopa_full_chance_match(None, 1, 0, None, 0, p(tab), None) == sl.SCOPA_EINVAL
    assert L.scopa_full_chance_cut(None, 0) == L.scopa_full_chance_root(None, None, None, None, None) == sl.SCOPA_EINVAL
    out = C.c_void_p()
    deck = sl.full_deal_py_seed(42)
    assert L.scopa_full_chance_create(None, p(deck), 1, None, 10, C.byref(out)) == sl.SCOPA_EINVAL and not out.value


# ---- 2. the deck sets of the GPU tests share rows ------------------------------------------------------------------------------------------------------
def _sharing(oracle, fix_seat):
    decks, _, st = G.deck_set(oracle, 42, 4, fix_seat=fix_seat)
    seen, rows = {}, X.Rows()
    for trav in range(2):
        X.traverse(st, decks, trav, 0, 0, 4, SEED, rows, seen=seen)
    by_a = {}
    for a, b in seen:
        by_a.setdefault(a, set()).add(b)
    return len(seen), sum(len(v) > 1 for v in seen.values()), sum(len(v) > 1 for v in by_a.values())


def test_the_deck_sets_of_the_gpu_tests_share_rows(oracle):
    """4 decks of packet_decks(deck 42, 4, 4, 5, fix_seat=0) below the round-4 root of the GPU tests, 4 traversals per traverser: some pair is met on
    several decks (rows really are shared: the atomics of one row come from different decks) and some word A occurs with several hands (the second
    word really decides).  At this root: 649 pairs, 20 of them on >= 2 decks, 97 words A with several hands.  With fix_seat=None the same shape shares NO
    pair between decks -- the root's own hands differ -- so the fixed seat matters."""
    n, on_several, a_several = _sharing(oracle, 0)
    print("pairs", n, "on >= 2 decks", on_several, "A words with several hands", a_several)
    assert on_several >= 1 and a_several >= 1
    assert _sharing(oracle, None)[1] == 0


# ---- 3. unbiased across decks --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trav", [0, 1])
def test_walk_is_unbiased_across_decks(oracle, trav):
    """The construction and the 5 of test_full_mccfr_ref.test_walk_is_unbiased_against_exact_enumeration on 4 decks: a round-4 root, uniform frozen
    sigma; sample t is the sum over the decks of traversal id t's d_regret rows, and its mean over 4 096 ids is held, cell by cell, to the enumerated
    counterfactual regret summed over decks by key."""
    root, _ = F.random_root(oracle.full_deal_py_seed(42), 4, np.random.RandomState(11))
    decks = packet_decks(oracle.full_deal_py_seed(42), 4, 4, 5, fix_seat=0)
    exact = X.exact_regret(root, decks, trav)
    n = 4096
    keys = sorted(exact)
    col = {k: i for i, k in enumerate(keys)}
    inc = np.zeros((n, len(keys), 3))
    starts = [X.root_on(root, d) for d in decks]
    for t in range(n):
        rows = X.Rows()
        for d, st in enumerate(starts):
            X.walk(st, trav, t, 0, SEED, rows, d, uniform=True)
        for k, dr in rows.dR.items():
            if (k[0] >> 62) & 1 == trav:
                inc[t, col[k]] = dr                                            # (a pair outside `exact` would be a KeyError: the key sets agree)
    mean, se = inc.mean(0), inc.std(0, ddof=1) / np.sqrt(n)
    want = np.array([exact[k] for k in keys])
    err = np.abs(mean - want)
    sure = se == 0.0
    assert (err[sure] <= 1e-12).all()
    ratio = err[~sure] / se[~sure]
    print("rows", len(keys), "largest |mean - exact| / se:", ratio.max())
    assert len(keys) >= 10 and (~sure).sum() >= 20
    assert (ratio <= 5.0).all()


# ---- 4. separation guards ------------------------------------------------------------------------------------------------------------------------------
def _counts(rows):
    k, c = rows.arrays("count")
    return k.tolist(), c.tolist()


@pytest.mark.parametrize("deck_seed", G.DECK_SEEDS)
@pytest.mark.parametrize("r0", [4, 3])
def test_one_launch_inputs_separate_wrong_walks(oracle, deck_seed, r0):
    """On the inputs of test_one_launch_vs_restatement_by_every_cut (nb = 5, either traverser): with the deck index dropped from the tag word, or with
    slots taken in hand order, the restatement's counts differ from the right ones, which the GPU test compares exactly"""
    for what, kw in (("deck index dropped from the tag", dict(tag_deck=False)), ("slots in hand order", dict(hand_order=True))):
        differs = 0
        for trav in range(2):
            right = G.ref_delta(oracle, deck_seed, r0, trav, 0, 0, 5, SEED)
            wrong = G.ref_delta(oracle, deck_seed, r0, trav, 0, 0, 5, SEED, **kw)
            differs += _counts(right) != _counts(wrong)
        assert differs, what


def test_wide_inputs_separate_narrowed_words(oracle):
    """the inputs of test_wide_words_and_a_deck_index_above_255: the counts change with the seed, the iteration or b0 narrowed (philox_words.narrowed),
    and with the deck index cut to its low 8 bits"""
    w = G.WIDE
    decks, _, st = G.deck_set(oracle, w["deck_seed"], w["r0"], w["n"], None)
    seed, iteration, b0 = W.WIDE_SEED, W.ITER_B31, (1 << 32) - w["nb"]
    for trav in range(2):
        want = _counts(G.ref_delta(oracle, w["deck_seed"], w["r0"], trav, iteration, b0, w["nb"], seed, listed=w["listed"], n=w["n"], fix_seat=None))
        assert len(want[0]) > 10
        variants = [(what, s2, it2, ids, lambda d: d) for what, s2, it2, ids in W.narrowed(seed, iteration, b0, w["nb"])]
        variants.append(("the deck index cut to 8 bits", seed, iteration, W.ids_of(b0, w["nb"]), lambda d: d & 0xFF))
        for what, s2, it2, ids, index in variants:
            rows = X.Rows()
            for d in w["listed"]:
                start = X.root_on(st, decks[d])
                for t in ids:
                    X.walk(start, trav, t, it2, s2, rows, index(d))
            assert _counts(rows) != want, (what, trav)


def test_store_inputs_separate_a_hash_or_compare_without_b(oracle):
    """B dropped from the hash: the 200 hands of one word A would share ONE home and 136 of them would be dropped at 64 probes; 64 fillers of one
    restated home would no longer fill the slots before the planted pair.  B dropped from the compare: the 200 pairs would come back as one row."""
    keys = np.stack([np.full(200, X.FILLER_A, np.uint64), X.hands3(0, 200)], 1)
    assert np.unique(X.home_of(keys[:, 0], keys[:, 1], 8)).size > 100
    assert np.unique(X.home_of(keys[:, 0], keys[:, 1], 8, with_b=False)).size == 1
    assert len({tuple(k) for k in keys.tolist()}) == 200 and len({int(k[0]) for k in keys}) == 1
    fill = X.fillers(700, 65, 10)
    assert (X.home_of(fill[:, 0], fill[:, 1], 10) == 700).all() and len({tuple(k) for k in fill.tolist()}) == 65
    assert np.unique(X.home_of(fill[:, 0], fill[:, 1], 10, with_b=False)).size > 1
    # the store modelled sequentially with and without B in the compare: without it a pair takes the first slot of its probe that holds its A for
    # its own, so fewer rows come back than pairs went in (the GPU tests ask for every pair exactly once with its own row)
    assert X.store_model(keys, 8) == 200 and X.store_model(keys, 8, compare_b=False) < 200
    assert X.store_model(fill[:64], 10) == 64 and X.store_model(fill[:64], 10, compare_b=False) < 64
    R, S = X.rows_for(keys)
    assert (R > 0).all() and (S > 0).all() and np.unique(R, axis=0).shape[0] > 100


def test_deep_chain_is_what_the_gpu_test_needs(oracle):
    """the 64 fillers sit on one home, the root pair's home is the next slot, it is met by every deck's traversals, and no other pair of the launch
    comes near the chain"""
    cap, fill, root_pair, rows = G.deep_chain(oracle)
    g = int(X.home_of(fill[0, 0], fill[0, 1], cap)[0])
    assert (X.home_of(fill[:, 0], fill[:, 1], cap) == g).all() and int(X.home_of(*root_pair, cap)[0]) == (g + 1) & ((1 << cap) - 1)
    assert len({tuple(k) for k in fill.tolist()}) == 64 and rows.count[root_pair] == G.N_DECKS * 2
    print("store of 2^%d slots" % cap)
    with_root, without = G.chain_match_without_root(oracle)
    assert not np.array_equal(with_root, without)                          # the match of the GPU test plays the row at the end of the chain
    assert not ({tuple(k) for k in fill.tolist()} & set(rows.count))


def test_non_zero_chain_launches_have_a_root_sigma_that_decides(oracle):
    """the launch sequence of the GPU chain test from non-zero tables, on the restatement alone: before every launch sigma at the root pair is not
    uniform, and where the root is the opponent's node a walk that read a zero row there (a read-only probe that missed it) gives other counts"""
    decks, _, st = G.deck_set(oracle, 42, 4)
    root_pair = X.wide_key(X.root_on(st, decks[0]), 0)
    rows = X.Rows()
    it = X.iterate(st, decks, 2, SEED, rows, 0)
    for cut in G.cuts_of(4):
        for trav in (1, 0):
            for k in list(rows.R):
                rows.touch(k)
            assert len(set(F.sigma_of(rows.R[root_pair], 3))) > 1, (cut, trav)
            if trav == 1:
                blind = rows.copy()
                blind.R[root_pair] = [0.0, 0.0, 0.0]
                X.traverse(st, decks, trav, it, 0, 16, SEED, blind)
            X.traverse(st, decks, trav, it, 0, 16, SEED, rows)
            if trav == 1:
                assert blind.arrays("count")[1].tolist() != rows.arrays("count")[1].tolist(), cut
            rows.apply()
            it += 1
    # the planted one-launch comparison: a missed root row (sigma a point mass on slot 1) changes the counts of traverser 1
    st, decks, K, n_act, R, S = G.planted(oracle)
    got = []
    for miss in (False, True):
        ref = X.Rows()
        ref.plant(K[1:] if miss else K, R[1:] if miss else R, S[1:] if miss else S)
        for k in [tuple(k) for k in K.tolist()]:
            ref.touch(k)
        X.traverse(st, decks, 1, 0, 0, 3, SEED, ref)
        got.append(ref.arrays("count")[1].tolist())
    assert got[0] != got[1]


def test_too_small_store_input_overflows(oracle):
    assert len(G.ref_delta(oracle, 42, 3, 0, 0, 0, 4, SEED).count) > (1 << 8)


def test_match_deck_rule():
    """both seats meet the same decks: episode i of seat 0 and episode i + ceil(n / 2) of seat 1 are played on the same deck"""
    for n in (1, 2, 63, 64, 65, 129, 4096):
        for k in (1, 3, 4):
            half = (n + 1) // 2
            first = [X.deck_of_episode(i, n, k) for i in range(half)]
            second = [X.deck_of_episode(i, n, k) for i in range(half, n)]
            assert first == [i % k for i in range(half)] and second == first[:len(second)]


# ---- 5. Python level -----------------------------------------------------------------------------------------------------------------------------------
def test_packet_decks_and_sample_decks(sl):
    deck = sl.full_deal_py_seed(42)
    for r, fix in ((0, None), (4, 0), (4, 1), (5, None), (2, 1)):
        first = 4 + 6 * r
        decks = packet_decks(deck, r, 12, 3, fix_seat=fix)
        assert decks.shape == (12, 40) and decks.dtype == np.uint8 and np.array_equal(decks[0], deck)
        assert len({d.tobytes() for d in decks}) == 12
        assert (decks[:, :first] == deck[:first]).all() and (np.sort(decks, 1) == np.arange(40)).all()
        if fix is not None:
            assert (decks[:, first + 3 * fix:first + 3 * fix + 3] == deck[first + 3 * fix:first + 3 * fix + 3]).all()
            other = first + 3 * (1 - fix)
            assert len({d[other:other + 3].tobytes() for d in decks}) > 1
        assert np.array_equal(decks, packet_decks(deck, r, 12, 3, fix_seat=fix)) and not np.array_equal(decks, packet_decks(deck, r, 12, 4, fix_seat=fix))
    assert packet_decks(deck, 5, 6, 0, fix_seat=1).shape == (6, 40)             # 3 free cards: 3! decks and no more
    for bad in (dict(rounds_played=5, n=7, fix_seat=1), dict(rounds_played=6, n=1), dict(rounds_played=0, n=0), dict(rounds_played=0, n=2, fix_seat=2)):
        with pytest.raises(ValueError):
            packet_decks(deck, seed=0, **bad)
    lists = sample_decks(8, 3, 5, seed=2)
    assert lists.shape == (5, 3) and lists.dtype == np.int32 and (np.diff(lists, axis=1) > 0).all() and lists.min() >= 0 and lists.max() < 8
    assert np.array_equal(sample_decks(8, 3, 2, seed=2, start=3), lists[3:]) and len({tuple(x) for x in lists.tolist()}) > 1
    with pytest.raises(ValueError):
        sample_decks(4, 5, 1)


# ---- guards of tests/test_gpu_full_chance_depth.py: its inputs can tell a wrong kernel from a right one, shown on the restatement alone ---------------------
def test_new_helpers_agree_with_the_walk(oracle):
    """subgame_keys holds every pair any walk below the root meets, edge_rows takes pairs in (A, B) order, touch_all adds unmet pairs at zero"""
    decks, _, st = G.deck_set(oracle, 42, 4)
    keys = GD.edge_keys(oracle, 42, 4)
    assert keys.dtype == np.uint64 and keys.shape[1] == 2 and [tuple(k) for k in keys.tolist()] == sorted({tuple(k) for k in keys.tolist()})
    met = set()
    for trav in range(2):
        met |= set(G.ref_delta(oracle, 42, 4, trav, 0, 0, 5, SEED).count)
    assert met < {tuple(k) for k in keys.tolist()}
    k2, n_act, R, S = X.edge_rows(keys[::-1], "onehot")
    assert np.array_equal(k2, keys) and list(n_act) == [X.key_actions(k) for k in keys] and not S.any()
    assert np.array_equal(R, E.edge_table("onehot", n_act)[:, :3])
    rows = X.Rows()
    rows.touch_all(keys[:3])
    assert sorted(rows.count) == [tuple(k) for k in keys[:3].tolist()] and not any(rows.count.values())
    fill = X.fillers(700, 64, 10)
    assert X.longest_reach(fill, 10) == 64 and X.longest_reach(fill[:5], 10) == 5


def test_deal3_is_what_the_gpu_test_needs(oracle):
    """the constants of the DEAL3 launches; rows really are shared by the decks (some pair is met on all three), the keys carry tables of 9 cards and
    more (wide_key's table loop past 8 slots), and traverser 0 draws with q at or above 2^15"""
    decks, root = GD.deal3(oracle)
    assert decks.shape == (3, 40) and (decks[:, :16] == decks[0, :16]).all() and len({d.tobytes() for d in decks}) == 3
    for trav in range(2):
        rows, seen = GD.deal3_ref(oracle, trav)
        assert (rows.choice, rows.terminal, len(rows.count)) == (GD.DEAL3_VISITS[trav], GD.DEAL3_TERMINALS, GD.DEAL3_ROWS[trav])
        assert set(seen) == set(rows.count)
        assert [sum(1 for v in seen.values() if len(v) == k) for k in (2, 3)] == [GD.DEAL3_ON_TWO[trav], GD.DEAL3_ON_THREE[trav]]
        assert sum(1 for n in rows.count.values() if n == 1) == GD.DEAL3_ONCE[trav] and max(rows.count.values()) == GD.DEAL3_MAX_COUNT[trav]
        assert max(bin((k[0] >> 16) & ((1 << 40) - 1)).count("1") for k in rows.count) >= 9
        assert any(k[0] & 0xFFFF for k in rows.count)                          # capture and scopa fields that are not zero
    assert GD._CACHE["q", 0] >= 1 << 15
    print("largest q of a draw:", GD._CACHE["q", 0], GD._CACHE["q", 1])


def test_deal3_capacity_guard(oracle):
    """the pair sets of the DEAL3 launches (either traverser, the one-deck iterate, the trained store) in ONE store of 2^CAP slots: no probe looks
    at more than 64 slots in any arrival order, and a probe in a store of fewer pairs looks at no more.  Longest probe: 29 slots at 2^18"""
    sets = [set(GD.deal3_ref(oracle, trav)[0].count) for trav in range(2)] + [set(GD.deal3_iterate_ref(oracle).R), set(GD.deal3_trained_ref(oracle).R)]
    union = sorted(set().union(*sets))
    reach = X.longest_reach(union, GD.CAP)
    print("DEAL3 pair sets,", [len(s) for s in sets], "pairs,", len(union), "in all at 2^%d slots: longest probe" % GD.CAP, reach)
    assert GD.CAP == 18 and reach <= 64                                       # 18: the smallest the choice was made from
    assert reach == 29                                                        # recorded


def test_cut_0_lane_numbering_separates(oracle):
    """the 132-lane input: a launch whose lane id lost its workgroup term walks lanes 0 .. 63 in every workgroup (and, with 132 for the bound, in all 64
    lanes of the third); one in which lane g >= 64 repeats lane g - 64 walks them twice and lanes 64 .. 67 once.  Either has other counts than the launch"""
    w = GD.LANES
    for trav in range(2):
        true = G.ref_delta(oracle, w["deck_seed"], w["r0"], trav, 0, 0, w["nb"], SEED, n=w["n"], fix_seat=None)
        assert _counts(GD.lanes_ref(oracle, trav, range(132))) == _counts(true)
        for lanes in ([g % 64 for g in range(192)], [g if g < 64 else g - 64 for g in range(132)]):
            assert _counts(GD.lanes_ref(oracle, trav, lanes)) != _counts(true), trav
        listed = G.ref_delta(oracle, w["deck_seed"], w["r0"], trav, 0, (1 << 32) - w["nb"], w["nb"], SEED, listed=(3, 1), n=w["n"], fix_seat=None)
        assert _counts(listed) != _counts(G.ref_delta(oracle, w["deck_seed"], w["r0"], trav, 0, (1 << 32) - w["nb"], w["nb"], SEED, listed=(1, 2), n=w["n"], fix_seat=None))


def _sigma_nonzero(R, n):
    """sigma_of with `!= 0.0` in place of `> 0.0`: negative cells enter the sum"""
    pos = [R[i] if R[i] != 0.0 else 0.0 for i in range(n)]
    s = pos[0]
    for i in range(1, n):
        s += pos[i]
    return [1.0 / n] * n if s == 0.0 else [x / s for x in pos]


def _sigma_flushed(R, n):
    """sigma_of with subnormals flushed to zero"""
    return F.sigma_of([x if abs(x) >= 2.2250738585072014e-308 else 0.0 for x in R], n)


@pytest.mark.parametrize("deck_seed,r0", GD.EDGE_ROOTS)
def test_edge_rows_guard(oracle, deck_seed, r0):
    """every finite edge table planted over every pair of the sub-game on the four decks: finite increments, every pair in the store; `!= 0.0` in
    sigma changes counts or d_strategy under allneg, onehot and big, a subnormal flush under subnormal; every table but allneg moves the image away
    from the zero-table run's; the pairs fit the store of the GPU test"""
    image = lambda rows: (_counts(rows), rows.arrays("dS")[1].tobytes())
    keys = GD.edge_keys(oracle, deck_seed, r0)
    assert X.longest_reach(keys, 14) <= 64 and ((deck_seed, r0) not in ((42, 4), (42, 3)) or keys.shape[0] == {4: 810, 3: 2937}[r0])
    for name in E.FINITE_TABLES:
        runs = [GD.edge_ref(oracle, deck_seed, r0, name, trav) for trav in range(2)]
        zero = [GD.edge_ref(oracle, deck_seed, r0, None, trav) for trav in range(2)]
        for trav in range(2):
            planted, rows, met = runs[trav]
            assert all(np.isfinite(rows.arrays(w)[1]).all() for w in ("dR", "dS")) and len(rows.count) == planted[0].shape[0] == keys.shape[0], name
            assert rows.choice == 4 * 4 * F.shape_counts(r0)[trav] and 0 < met <= keys.shape[0]
        differs = [image(runs[trav][1]) != image(zero[trav][1]) or runs[trav][1].arrays("dR")[1].tobytes() != zero[trav][1].arrays("dR")[1].tobytes() for trav in range(2)]
        assert any(differs) or name == "allneg", name
        wrong = {"allneg": _sigma_nonzero, "onehot": _sigma_nonzero, "big": _sigma_nonzero, "subnormal": _sigma_flushed}.get(name)
        if wrong:
            assert any(image(GD.edge_ref(oracle, deck_seed, r0, name, trav, sigma_of=wrong)[1]) != image(runs[trav][1]) for trav in range(2)), name
    sub = GD.edge_ref(oracle, deck_seed, r0, "subnormal", 0)[0]
    assert (sub[2] == 5e-324).any() and ((sub[2] == 0.0).sum(1) > 3 - sub[1]).any()


def test_match_inputs_separate(oracle):
    """the match of tests/test_gpu_full_chance_depth.py on the restated trained store: a stream word cut to 16 bits, the seat rule 2 i <= n, the deck
    i % k in place of j % k, and (on the planted rows of test_match_threshold) the threshold 1e-14 each change some episode"""
    decks, root = GD.deal3(oracle)
    table = GD.deal3_trained_ref(oracle).S
    five = GD.held_out_deal(oracle, 5)
    assert five.shape == (5, 40) and (five[:, :16] == decks[0, :16]).all() and not ({d.tobytes() for d in five} & {d.tobytes() for d in decks})
    run = lambda ds, n, **kw: X.match(root, ds, table, n, W.WIDE_SEED, GD.MATCH_STREAM, **kw)
    rule = {(name, n): run(ds, n) for name, ds in (("own", decks), ("one", five[:1]), ("five", five)) for n in GD.MATCH_NS + (3,)}
    assert not np.array_equal(rule["own", 129][0], X.match(root, decks, {}, 129, W.WIDE_SEED, GD.MATCH_STREAM)[0])   # the store is played
    assert GD.MATCH_STREAM == (1 << 24) - 1
    for name, ds in (("own", decks), ("one", five[:1]), ("five", five)):
        assert not np.array_equal(rule[name, 129][1], run(ds, 129, stream_bits=16)[1]), name
        assert any(not np.array_equal(rule[name, n][1], run(ds, n, split_le=True)[1]) for n in (2, 64)), name
    for n in (1, 63, 65, 129):                                               # an odd n cannot show the seat rule
        assert np.array_equal(rule["own", n][1], run(decks, n, split_le=True)[1])
    assert any(not np.array_equal(rule[name, n][1], run(ds, n, deck_by_episode=True)[1]) for name, ds, n in (("own", decks, 129), ("five", five, 129), ("five", five, 3)))
    assert np.array_equal(rule["one", 129][1], run(five[:1], 129, deck_by_episode=True)[1])            # one deck: no rule to tell
    # the threshold, on the planted rows
    st, ds, (below, above) = GD.threshold_tables(oracle)
    k_root = X.wide_key(X.root_on(st, ds[0]), 0)
    assert below[k_root] == [1e-13, 0.0, 0.0] and F.average_probs(below, k_root, 3) == [1.0 / 3] * 3 and F.average_probs(above, k_root, 3) == [0.25, 0.0, 0.75]
    assert sorted(F.average_probs(below, k, X.key_actions(k)) for k in below if k != k_root) == [[1.0 / 3] * 3, [0.5, 0.5]]
    play = lambda t, **kw: X.match(st, ds, t, 129, W.WIDE_SEED, GD.MATCH_STREAM, **kw)[1]
    assert np.array_equal(play(below), play({})) and not np.array_equal(play(below), play(below, threshold=1e-14))
    assert not np.array_equal(play(above), play(below)) and np.array_equal(play(above), play(above, threshold=1e-14))
