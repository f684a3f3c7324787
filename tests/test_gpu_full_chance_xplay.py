"""GPU checks of FullScopa over decks, store against store (scopa_amd/csrc/scopa_full_chance_xplay.hip: scopa_full_chance_cross_play,
scopa_full_chance_pair_match, and their Python surface) against the restatement tests/full_chance_xplay_ref.py, which
tests/test_full_chance_xplay_ref.py holds to depth-first recursions, to full_chance_exploit_ref.solve and to full_chance_ref.match, and whose guards
show that the comparisons below tell a kernel that takes prob_b at player 0's levels, or slots in hand order, from the right one.

Every sum of the device code has one order, the restatement's, so all [K][K][4] results are compared on bits, and the match on every sum and every
episode.  Shapes are test_gpu_full_chance_exploit's: R = 1 on 3 decks, R = 2 on 5 decks, R = 3 on 2 decks (K = 2 there, for the restatement's
sake).  Below deck 42's R = 2 root nobody sweeps the table, so the two scopa quantities are zero there; the same shape on deck 11's packet has leaves
with up to 2 and 3 scopas and is run too.  The stores: one trained by three `iterate` calls, one planted through tables_set on every pair of the
forest with a zero-total row, a one-hot row and a row summing to 1e-13 among them, one empty.

Every test here fails on a tree without the two entry points (the bindings do not resolve).  Measured once on an MI355X (`-s` prints the figures
again): the module takes 8 s, of which the device calls are milliseconds -- a cross_play call of the small shapes 0.2 - 0.4 ms, 15 handles x 863
decks at R = 2 (the passing side of the K x k x 36^R edge, 3.1 GB of scratch) 3 ms, 3 236 decks at K = 1 1 ms; the rest is the restatement: the
R = 3 forest 2.1 s, the 512-episode matches from the deal 1.9 s, the two R = 2 pair-match sweeps 0.7 s."""
import ctypes as C
import time

import numpy as np
import pytest

import full_chance_ref as W
import full_chance_xplay_ref as XP
import full_mccfr_ref as F
from test_full_chance_xplay_ref import hot_table, planted
from test_gpu_full_chance_exploit import SEED, level_pairs, packet, plant, same_arrays, same_bits, state_of, tables_of

pytestmark = pytest.mark.gpu

SHAPES = {1: (5, 3, None, 42), 2: (4, 5, 0, 42), 3: (3, 2, 0, 42), "scopas": (4, 5, 0, 11)}     # (round of the root, decks, fixed seat, deck seed)
_TREES = {}


def xp_tree(st, decks, R):
    key = (bytes(st.s), np.ascontiguousarray(decks, np.uint8).tobytes())
    if key not in _TREES:
        _TREES[key] = XP.tree_of(st, decks, R)
    return _TREES[key]


def stores_of(ctx, sl, oracle, shape, K=3):
    """(handles: trained, planted, empty; their tables as the restatement takes them; forest; decks; oracle root; root record)"""
    r0, n, fix_seat, deck_seed = SHAPES[shape]
    decks, acts, st = packet(oracle, r0, n, fix_seat, deck_seed)
    root = state_of(sl, decks[0], acts)
    tree = xp_tree(st, decks, 6 - r0)
    ctx.mccfr_seed(SEED)
    hs = [sl.FullChanceMCCFR(ctx, decks, root, 16), sl.FullChanceMCCFR(ctx, decks[::-1].copy(), root, 15), sl.FullChanceMCCFR(ctx, decks[:1], root, 8)][:K]
    hs[0].iterate(16, 3)
    plant(hs[1], *planted(tree))
    return hs, [tables_of(h) for h in hs], tree, decks, st, root


def close(hs):
    for h in hs:
        h.close()


def held_out(decks, r0, fix_seat, k):
    from scopa_amd.algorithms import packet_decks
    have = {d.tobytes() for d in decks}
    more = packet_decks(decks[0], r0, len(decks) + k + 4, 9, fix_seat=fix_seat)
    out = np.array([d for d in more if d.tobytes() not in have][:k], np.uint8)
    assert out.shape == (k, 40)
    return out


def raw_cross_play(sl, handles, K, root, decks, which, out, k=None):
    """the C entry point itself, for refusals: -> status, with `out` as the call left it; k: a deck count other than the array's"""
    hs = (C.c_void_p * max(len(handles), 1))(*[None if h is None else h._h for h in handles])
    root = None if root is None else np.ascontiguousarray(root, sl.FULL_STATE_DTYPE).reshape(1)
    held = None if decks is None else np.ascontiguousarray(decks, np.uint8).reshape(-1, 40)
    return sl.lib().scopa_full_chance_cross_play(hs, K, sl._ptr(root), sl._ptr(held), (0 if held is None else held.shape[0]) if k is None else k, which, sl._ptr(out))


# ---- 1. bits against the restatement --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [1, 2, 3, "scopas"])
def test_cross_play_vs_restatement(ctx, sl, oracle, shape):
    K = 2 if shape == 3 else 3
    hs, tables, tree, decks, st, root = stores_of(ctx, sl, oracle, shape, K)
    assert len(tables[0][1]) > 10 and len(tables[1][1]) == len(level_pairs(tree)) and (K == 2 or not tables[2][1])
    for which in ((0, 1) if shape != 3 else (0,)):
        t0 = time.time()
        got = sl.FullChanceMCCFR.cross_play(hs, None, which)
        t1 = time.time()
        want = XP.cross_play(tree, tables, which)
        print("shape", shape, "which", which, "device", round(t1 - t0, 4), "s, restatement", round(time.time() - t1, 2), "s\n", got[:, :, 0])
        assert got.shape == (K, K, 4) and same_bits(got, want), (got, want)
        assert same_bits(sl.FullChanceMCCFR.cross_play(hs, None, which), got)                     # two calls: identical bits
        assert len({x for x in got[:, :, 0].ravel()}) == K * K
    if shape == "scopas":
        assert (got[:, :, 2] > 0.0).sum() >= 6 and (got[:, :, 3] > 0.0).sum() >= 6 and (got[:, :, 2] != got[:, :, 3]).sum() >= 6   # scopas are made, by both
    close(hs)


def test_held_out_decks_a_deck_twice_and_a_descendant_root(ctx, sl, oracle):
    hs, tables, tree, decks, st, root = stores_of(ctx, sl, oracle, 2)
    r0, _, fix_seat, _ = SHAPES[2]
    other = held_out(decks, r0, fix_seat, 3)
    for which in (0, 1):
        got = sl.FullChanceMCCFR.cross_play(hs, None, which, other)
        assert same_bits(got, XP.cross_play(xp_tree(st, other, 2), tables, which))
        assert not same_bits(got, sl.FullChanceMCCFR.cross_play(hs, None, which))
    twice = np.ascontiguousarray(np.concatenate([decks[:2], decks[:1], other[:1]]))               # deck 0 counts twice
    got = sl.FullChanceMCCFR.cross_play(hs, root, 0, twice)
    assert same_bits(got, XP.cross_play(xp_tree(st, twice, 2), tables, 0))
    assert not same_bits(got, sl.FullChanceMCCFR.cross_play(hs, root, 0, np.ascontiguousarray(twice[[0, 1, 3]])))
    # a round boundary six plies below the root, on decks that share the sixth deal too: the stores' own roots and decks do not matter
    from scopa_amd.algorithms import packet_decks
    _, acts, _ = packet(oracle, *SHAPES[2])
    ps, more, rng = sl.FullState(deck=decks[0]), [], np.random.RandomState(2)
    for a in acts:
        ps.step(a)
    for _ in range(6):
        legal = ps.legal()
        more.append(int(legal[rng.randint(len(legal))]))
        ps.step(more[-1])
    below = packet_decks(decks[0], 5, 3, 4)
    st5 = F.root_of(decks[0], list(acts) + more)
    for which in (0, 1):
        got = sl.FullChanceMCCFR.cross_play(hs[::-1], ps.s, which, below)                          # hs[2], one deck and 256 slots, owns the scratch
        assert same_bits(got, XP.cross_play(xp_tree(st5, below, 1), tables[::-1], which))
    assert len(set(got[:, :, 0].ravel())) > 1
    close(hs)


# ---- 2. the handle list ---------------------------------------------------------------------------------------------------------------------------------
def test_a_handle_twice_and_one_handle(ctx, sl, oracle):
    hs, tables, tree, decks, st, root = stores_of(ctx, sl, oracle, 2)
    got = sl.FullChanceMCCFR.cross_play([hs[0], hs[1], hs[0]], None, 0)
    assert same_bits(got, XP.cross_play(tree, [tables[0], tables[1], tables[0]], 0))
    assert same_bits(got[0], got[2]) and same_bits(got[:, 0], got[:, 2]) and not same_bits(got[0], got[1])
    for j in range(3):
        one = sl.FullChanceMCCFR.cross_play([hs[j]], None, 1, decks)                               # (hs[1] and hs[2] hold other deck lists)
        assert one.shape == (1, 1, 4) and same_bits(one, XP.cross_play(tree, [tables[j]], 1))
    close(hs)


# ---- 3. the routes that exist: exploitability's value, a merged store, the pure response ----------------------------------------------------------------------
@pytest.mark.parametrize("shape", [1, 2])
def test_pins_to_exploitability(ctx, sl, oracle, shape):
    hs, tables, tree, decks, st, root = stores_of(ctx, sl, oracle, shape)
    r0, _, fix_seat, _ = SHAPES[shape]
    other = held_out(decks, r0, fix_seat, 2)
    player = lambda k: (k[0] >> 62) & 1
    third = sl.FullChanceMCCFR(ctx, decks, root, 16)
    for which in (0, 1):
        for ds in (None, other):
            got = sl.FullChanceMCCFR.cross_play(hs, None, which, ds)
            for a, h in enumerate(hs):
                assert same_bits(got[a, a, 0], h.exploitability(None, which, ds if ds is not None else decks)["value"]), (which, a)
            for a, b in ((0, 1), (1, 2)):
                R = {**{k: v for k, v in tables[a][0].items() if player(k) == 0}, **{k: v for k, v in tables[b][0].items() if player(k) == 1}}
                S = {**{k: v for k, v in tables[a][1].items() if player(k) == 0}, **{k: v for k, v in tables[b][1].items() if player(k) == 1}}
                plant(third, R, S)
                assert same_bits(got[a, b, 0], third.exploitability(None, which, ds if ds is not None else decks)["value"]), (which, a, b)
    for a in (0, 1):
        e = hs[a].exploitability(None, 0, decks)
        hot = [hot_table(hs[a].response_get(p)) for p in range(2)]
        p0, p1 = sl.FullChanceMCCFR(ctx, decks, root, 15), sl.FullChanceMCCFR(ctx, decks, root, 15)
        plant(p0, {}, hot[0])
        plant(p1, {}, hot[1])
        got = sl.FullChanceMCCFR.cross_play([hs[a], p0, p1], None, 0)
        assert got[1, 0, 0] == e["br0"] and got[0, 2, 0] == -e["br1"], (got[:, :, 0], e)          # (==, not bits: a signed zero may differ)
        assert e["br0"] != e["value"]
        close([p0, p1])
    close(hs + [third])


# ---- 4. nothing moved -------------------------------------------------------------------------------------------------------------------------------------
def test_cross_play_and_pair_match_leave_every_handle_as_it_was(ctx, sl, oracle):
    hs, tables, tree, decks, st, root = stores_of(ctx, sl, oracle, 2)
    hs[0].traverse(0, 7, 0, 4)                                                                     # increments and counts that no apply has folded in
    for h in hs:
        h.exploitability(None, 0)
    before = [(h.tables_get(), h.delta_get(), h.counters(), [h.response_get(p) for p in range(2)]) for h in hs]
    assert before[0][1][1].sum() > 0
    sl.FullChanceMCCFR.cross_play(hs, None, 0)
    sl.FullChanceMCCFR.cross_play(hs[::-1], None, 1, decks[:2])
    hs[0].pair_match(hs[1], 1000, 3)
    hs[1].pair_match(hs[0], 1000, 3, decks[:2])
    for h, (t, d, c, r) in zip(hs, before):
        assert same_arrays(h.tables_get(), t) and same_arrays(h.delta_get(), d) and h.counters() == c
        assert all(same_arrays(h.response_get(p), r[p]) for p in range(2))
    close(hs)


# ---- 5. limits and refusals, each with h_out untouched ------------------------------------------------------------------------------------------------------
def test_refusals_leave_h_out_untouched(ctx, sl, oracle):
    hs, tables, tree, decks, st, root = stores_of(ctx, sl, oracle, 2)
    out = np.full((17, 17, 4), 7.25)
    sentinel = out.copy()

    def refused(status, handles, K, root_=None, decks_=None, which=0, k=None):
        assert raw_cross_play(sl, handles, K, root_, decks_, which, out, k) == status and np.array_equal(out, sentinel)

    refused(sl.SCOPA_EINVAL, [hs[0]] * 17, 17)
    refused(sl.SCOPA_EINVAL, [hs[0]], 0)
    refused(sl.SCOPA_EINVAL, [hs[0], None, hs[1]], 3)
    refused(sl.SCOPA_EINVAL, hs, 3, which=2)
    refused(sl.SCOPA_EINVAL, hs, 3, decks_=decks, k=0)
    refused(sl.SCOPA_EINVAL, hs, 3, decks_=decks, k=-3)
    assert sl.lib().scopa_full_chance_cross_play(None, 1, None, None, 0, 0, sl._ptr(out)) == sl.SCOPA_EINVAL
    assert sl.lib().scopa_full_chance_cross_play((C.c_void_p * 1)(hs[0]._h), 1, None, None, 0, 0, None) == sl.SCOPA_EINVAL
    other_ctx = sl.Context(0)
    alien = sl.FullChanceMCCFR(other_ctx, decks, root, 8)
    refused(sl.SCOPA_EINVAL, [hs[0], alien], 2)
    alien.close()
    other_ctx.close()
    mid = root.copy()
    mid["step"] = 25                                                                               # not a round boundary
    refused(sl.SCOPA_EINVAL, hs, 3, root_=mid)
    deck = oracle.full_deal_py_seed(42)
    early = sl.FullState(deck=deck)
    for _ in range(6):
        early.step(early.legal()[0])
    refused(sl.SCOPA_ELIMIT, hs, 3, root_=early.s, decks_=deck[None, :])                           # R = 5
    bad = decks.copy()
    bad[1, [38, 2]] = bad[1, [2, 38]]                                                              # a stock card swapped with one the root has seen
    refused(sl.SCOPA_EINVAL, hs, 3, decks_=bad)
    with pytest.raises(sl.ScopaError) as e:
        sl.FullChanceMCCFR.cross_play(hs, None, 0, bad)
    assert e.value.status == sl.SCOPA_EINVAL and "deck" in str(e.value)
    assert same_bits(sl.FullChanceMCCFR.cross_play(hs, None, 0), XP.cross_play(tree, tables, 0))   # the handles still answer
    close(hs)


def test_the_edge_of_the_store_leaf_limit(ctx, sl, oracle):
    """K x k x 36^R <= 1 << 24 at R = 2: 15 x 863 x 1296 = 16 776 720 passes, 16 x 863 x 1296 = 17 895 168 is refused; k x 36^R <= 1 << 22 holds
    3 236 decks and refuses 3 237.  The passing side is one store listed 15 times, so every entry must be the one value exploitability reports."""
    from scopa_amd.algorithms import packet_decks
    r0, _, fix_seat, _ = SHAPES[2]
    decks, acts, st = packet(oracle, r0, 5, fix_seat)
    root = state_of(sl, decks[0], acts)
    many = packet_decks(decks[0], r0, 3237, 6)
    assert 15 * 863 * 1296 <= 1 << 24 < 16 * 863 * 1296 and 3236 * 1296 <= 1 << 22 < 3237 * 1296
    ctx.mccfr_seed(SEED)
    h = sl.FullChanceMCCFR(ctx, decks, root, 16)
    h.iterate(16, 3)
    out = np.full((16, 16, 4), 7.25)
    assert raw_cross_play(sl, [h] * 16, 16, None, many[:863], 0, out) == sl.SCOPA_ELIMIT and np.all(out == 7.25)
    assert raw_cross_play(sl, [h], 1, None, many, 0, out) == sl.SCOPA_ELIMIT and np.all(out == 7.25)
    t0 = time.time()
    got = sl.FullChanceMCCFR.cross_play([h] * 15, None, 0, many[:863])
    print("15 handles x 863 decks at R = 2:", round(time.time() - t0, 3), "s")
    value = h.exploitability(None, 0, many[:863])["value"]
    assert got.shape == (15, 15, 4) and same_bits(got[:, :, 0], np.full((15, 15), value)) and all(same_bits(got[a, b], got[0, 0]) for a in range(15) for b in range(15))
    t0 = time.time()
    one = sl.FullChanceMCCFR.cross_play([h], None, 0, many[:3236])
    print("1 handle x 3236 decks at R = 2:", round(time.time() - t0, 3), "s")
    assert same_bits(one[0, 0, 0], h.exploitability(None, 0, many[:3236])["value"])
    h.close()


# ---- 6. the pair match ------------------------------------------------------------------------------------------------------------------------------------
def test_pair_match_vs_restatement(ctx, sl, oracle):
    hs, tables, tree, decks, st, root = stores_of(ctx, sl, oracle, 2)
    r0, _, fix_seat, _ = SHAPES[2]
    other = held_out(decks, r0, fix_seat, 3)
    S = [t[1] for t in tables]
    stream = 5
    own = [decks, decks[::-1], decks[:1]]                                                          # what each handle was created on: h_a's are the default
    for which in (None, other):
        for a, b, n in ((0, 1, 2000), (1, 0, 2000), (0, 0, 2000), (0, 1, 1999), (1, 2, 65), (0, 1, 1)):
            sums, r2 = hs[a].pair_match(hs[b], n, stream, which, per_episode=True)
            want, want_r2 = XP.pair_match(st, own[a] if which is None else other, S[a], S[b], n, SEED, stream)
            assert np.array_equal(r2, want_r2) and np.array_equal(sums, want), (a, b, n, which is None)
            assert np.array_equal(hs[a].pair_match(hs[b], n, stream, which), sums)
        # an opponent without rows, or with rows of no pair met, is uniform play: `match` exactly
        filler = sl.FullChanceMCCFR(ctx, decks, root, 8)
        keys = W.fillers(3, 40, 8)
        R_, S_ = W.rows_for(keys)
        filler.tables_set(keys, np.full(40, 3, np.int32), R_, S_)
        for empty in (hs[2], filler):
            for n in (2000, 1999):
                sums, r2 = hs[0].pair_match(empty, n, stream, which, per_episode=True)
                m_sums, m_r2 = hs[0].match(n, stream, which, per_episode=True)
                assert np.array_equal(sums, m_sums) and np.array_equal(r2, m_r2)
        filler.close()
    sums = hs[0].pair_match(hs[1], 2000, stream)
    assert not np.array_equal(sums, hs[0].match(2000, stream)) and not np.array_equal(sums, hs[0].pair_match(hs[1], 2000, stream + 1))
    assert not hs[0].pair_match(hs[1], 0).any()
    bad = other.copy()
    bad[1, [38, 2]] = bad[1, [2, 38]]
    for call in (lambda: hs[0].pair_match(hs[1], 64, stream, bad), lambda: hs[0].pair_match(hs[1], (1 << 36) + 1, stream),
                 lambda: hs[0].pair_match(hs[1], 64, 1 << 24), lambda: hs[0].pair_match(hs[1], -1)):
        with pytest.raises(sl.ScopaError) as e:
            call()
        assert e.value.status == sl.SCOPA_EINVAL
    sums6 = np.zeros(6, np.int64)
    assert sl.lib().scopa_full_chance_pair_match(hs[0]._h, None, 64, 0, None, 0, sl._ptr(sums6), None) == sl.SCOPA_EINVAL
    other_ctx = sl.Context(0)
    alien = sl.FullChanceMCCFR(other_ctx, decks, root, 8)
    with pytest.raises(sl.ScopaError) as e:
        hs[0].pair_match(alien, 64)
    assert e.value.status == sl.SCOPA_EINVAL
    alien.close()
    other_ctx.close()
    assert hs[1].counters()["rows"] == len(tables[1][1]) and hs[2].counters()["rows"] == 0         # the match never inserts
    close(hs)


def test_pair_match_from_the_deal(ctx, sl, oracle):
    """the whole 36-ply game, where no exact measure exists: 512 episodes on three decks that share two rounds, and on held-out decks of the packet"""
    from test_gpu_full_chance_depth import CAP, deal3, held_out_deal
    decks, st = deal3(oracle)
    ctx.mccfr_seed(SEED)
    a, b = sl.FullChanceMCCFR(ctx, decks, None, CAP), sl.FullChanceMCCFR(ctx, decks, None, CAP)
    a.iterate(1, 1)
    b.iterate(1, 2)
    S = [tables_of(h)[1] for h in (a, b)]
    assert len(S[0]) > 50000 and len(S[1]) > len(S[0])
    for which, ds in ((None, decks), (held_out_deal(oracle, 2), held_out_deal(oracle, 2))):
        sums, r2 = a.pair_match(b, 512, 9, which, per_episode=True)
        want, want_r2 = XP.pair_match(st, ds, S[0], S[1], 512, SEED, 9)
        assert np.array_equal(r2, want_r2) and np.array_equal(sums, want)
    sums, r2 = a.pair_match(b, 511, 9, None, per_episode=True)
    m_sums, m_r2 = a.match(511, 9, None, per_episode=True)
    assert not np.array_equal(r2, m_r2)
    empty = sl.FullChanceMCCFR(ctx, decks, None, 8)
    sums, r2 = a.pair_match(empty, 511, 9, None, per_episode=True)
    assert np.array_equal(sums, m_sums) and np.array_equal(r2, m_r2)
    close([a, b, empty])


# ---- 7. the Python surface ----------------------------------------------------------------------------------------------------------------------------------
def test_evaluate_against_the_exact_target(ctx, sl, oracle):
    """n = 1 << 16 on 4 decks: n / 2 is a multiple of k, so each seating plays every deck 8 192 times and the exact target is the match's law.  The
    Philox stream is fixed, so the comparison is deterministic."""
    from scopa_amd.algorithms import FullChanceMCCFRTrainer, full_chance
    r0, _, fix_seat, _ = SHAPES["scopas"]
    decks, acts, st = packet(oracle, r0, 4, fix_seat, 11)
    ctx.mccfr_seed(SEED)
    a = FullChanceMCCFRTrainer(decks=decks, root_actions=acts, capacity_log2=14, batch=16, ctx=ctx)
    b = FullChanceMCCFRTrainer(decks=decks, root_actions=acts, capacity_log2=14, batch=16, ctx=ctx)
    a.train(20)
    b.train(2)
    n = 1 << 16
    out = full_chance.cross_play([a, b])
    assert same_bits(out, a.cross_play([b])) and same_bits(out[0, 0, 0], a.policy_value()) and same_bits(out[1, 1, 0], b.policy_value())
    assert same_bits(full_chance.cross_play([a, b], current=True)[1, 1, 0], b.policy_value(current=True))
    assert same_bits(full_chance.cross_play([b, a], root_actions=acts), out[::-1, ::-1])
    e = a.evaluate_vs(b, n)
    print(e)
    assert e["episodes"] == n and (n // 2) % len(decks) == 0 and [h["episodes"] for h in e["by_seat"]] == [n // 2, n // 2]
    assert e["exact_by_seat"] == (out[0, 1, 0], -out[1, 0, 0]) and e["exact_reward"] == (out[0, 1, 0] - out[1, 0, 0]) / 2.0
    for seat, cell in enumerate((out[0, 1], out[1, 0])):
        se = np.sqrt((cell[1] - cell[0] ** 2) / (n / 2))
        h = e["by_seat"][seat]
        assert se > 0.0 and h["exact_std_error"] == se
        assert abs(h["reward"] - h["exact_reward"]) <= 5.0 * se, (seat, h, se)
    assert abs(e["reward"] - e["exact_reward"]) <= 5.0 * e["exact_std_error"] and 0.0 < e["exact_std_error"] < e["by_seat"][0]["exact_std_error"]
    assert e["a_scopas"] > 0.0 and e["b_scopas"] > 0.0 and np.array_equal(e["sums"], a.solver.pair_match(b.solver, n))
    held = full_chance.evaluate(a, b, 4096, decks=held_out(decks, r0, fix_seat, 4), stream_id=3)
    assert held["exact_reward"] is not None and held["exact_reward"] != e["exact_reward"]
    a.close()
    b.close()
    # the deal's root: six rounds to go, no exact measure
    from test_gpu_full_chance_depth import CAP, deal3
    decks, _ = deal3(oracle)
    a = FullChanceMCCFRTrainer(decks=decks, capacity_log2=CAP, batch=1, ctx=ctx)
    b = FullChanceMCCFRTrainer(decks=decks, capacity_log2=8, batch=1, ctx=ctx)
    a.train(1)
    e = a.evaluate_vs(b, 600)
    assert e["exact_reward"] is None and e["exact_std_error"] is None and e["exact_by_seat"] is None
    assert all(h["exact_reward"] is None and h["exact_std_error"] is None and h["episodes"] == 300 for h in e["by_seat"])
    mean, se, scopas = a.evaluate_vs_random(600)                                                   # b is empty: uniform play
    assert e["reward"] == mean and abs(e["std_error"] - se) < 1e-12 and e["a_scopas"] == scopas["trained_avg"]
    with pytest.raises(sl.ScopaError) as err:
        a.cross_play([b])
    assert err.value.status == sl.SCOPA_ELIMIT
    a.close()
    b.close()
