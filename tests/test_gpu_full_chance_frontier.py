"""GPU checks of the frontier form of Deep CFR's traversal on FullScopa over decks (scopa_full_chance_sdcfr_traverse_frontier,
scopa_full_chance_sdcfr_policy_at; scopa_amd/csrc/scopa_full_chance_sdcfr.hip) against tests/full_chance_frontier_ref.py, which
tests/test_full_chance_frontier_ref.py holds to a depth-first recursion.

policy_at is held to the forest's table on bits and to the float64 forward pass within full_chance_sdcfr_ref's propagated tolerance; the traversal is
compared with the device's own policy_at as the restatement's policy, so no draw is ambiguous and features, regrets, ring positions, root values and
visits are compared exactly.  Shapes: R = 1 on 3 decks (one root per traversal, ragged 16-node tiles), R = 2 on 3 decks with a list, R = 3 on 2 decks,
R = 5 and the deal beyond the forest's cap, 90 decks at R = 3 (one over the cap), scratch budgets that put chunk seams inside a deck's batch."""
import numpy as np
import pytest
import torch

import full_chance_frontier_ref as FR
import full_chance_sdcfr_ref as S
import full_mccfr_ref as F
import test_gpu_full_chance_sdcfr as G

from test_gpu_full_chance_sdcfr import NETS, Ring, SEED, SENTINEL, dev_nets, forest_of, packet, raises, state_of

pytestmark = pytest.mark.gpu


def device_policy_fn(ctx, w):
    """the restatement's policy: scopa_full_chance_sdcfr_policy_at on the level's key pairs"""
    wp = [t.data_ptr() for t in w]

    def fn(keys2, player):
        return policy_at(ctx, wp, keys2, player)
    return fn


def policy_at(ctx, wp, keys2, player):
    keys2 = np.ascontiguousarray(keys2, np.uint64).reshape(-1, 2)
    n = len(keys2)
    k = torch.tensor(keys2.view(np.int64), device="cuda")
    pol = torch.full((n, 3), SENTINEL, dtype=torch.float32, device="cuda")
    thr = torch.zeros((n, 2), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.full_chance_sdcfr_policy_at(player, k.data_ptr(), n, wp, pol.data_ptr(), thr.data_ptr())
    ctx.synchronize()
    return pol.cpu().numpy(), thr.cpu().numpy().view(np.uint64)


def traverse(ctx, h, trav, batch, w, ring, write_base, iteration=3, b0=0, decks=None, root=None):
    m = h.n_decks if decks is None else len(decks)
    vals = torch.full((m * batch,), SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    h.sdcfr_traverse_frontier(trav, batch, [t.data_ptr() for t in w], ring.feat.data_ptr(), ring.regret.data_ptr(), ring.capacity, write_base, vals.data_ptr(),
                              iteration, b0, decks, root)
    ctx.synchronize()
    return vals.cpu().numpy()


def check_rows(root_st, all_decks, fn, R, trav, batch, listed, ring, write_base, vals, iteration, b0, what, only=None):
    """every row of every traversal of a call (only: of these slots) against the restatement; with all slots checked, the rest of the ring untouched"""
    feat, regret = ring.host()
    rows = S.rows_per_traversal(R)
    touched = np.zeros(ring.capacity, bool)
    for slot, deck in enumerate(listed):
        if only is not None and slot not in only:
            continue
        for i in range(batch):
            tid = (b0 + deck * batch + i) & 0xFFFFFFFF
            ref = FR.walk_frontier(root_st, all_decks[deck], trav, tid, iteration, SEED, fn)
            assert np.float32(vals[slot * batch + i]).tobytes() == np.float32(ref["value"]).tobytes(), (what, slot, i)
            assert ref["visits"] == S.visits_per_traversal(R, trav) and len(ref["rows"]) == rows
            pos = np.array([S.ring_row(write_base, rows, slot, batch, i, rank, ring.capacity) for rank in range(rows)])
            assert not touched[pos].any() and len(set(pos.tolist())) == rows
            touched[pos] = True
            want_reg = np.stack([ref["rows"][rank][1] for rank in range(rows)])
            want_feat = S.features(np.array([ref["rows"][rank][0] for rank in range(rows)], np.uint64))
            assert np.array_equal(regret[pos].view(np.uint32), want_reg.view(np.uint32)), (what, slot, i)
            assert np.array_equal(feat[pos].view(np.uint32), want_feat.view(np.uint32)), (what, slot, i)
    if only is None:
        assert touched.sum() == rows * len(listed) * batch
        assert (feat[~touched] == SENTINEL).all() and (regret[~touched] == SENTINEL).all(), what


def game(ctx, sl, oracle, r0, n, fix_seat, capacity_log2=10, **kw):
    decks, acts, st = packet(oracle, r0, n, fix_seat, **kw)
    ctx.mccfr_seed(SEED)
    return sl.FullChanceMCCFR(ctx, decks, state_of(sl, decks[0], acts), capacity_log2), decks, acts, st


# ---- 1. policy_at against the forest's table and float64 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["xavier", "negative", "exact"])
def test_policy_at_vs_the_forest(ctx, sl, oracle, kind):
    h, decks, acts, st = game(ctx, sl, oracle, 4, 3, 0)
    forest = forest_of(st, decks, 2)[0]
    nets = NETS[kind]()
    w = dev_nets(nets)
    wp = [t.data_ptr() for t in w]
    ring = Ring(S.rows_per_traversal(2) * 3)
    G.traverse(ctx, h, 0, 1, w, ring, 0)
    pol, thr, keys = h.sdcfr_policy_get()
    ref, tol = G.ref_policy(forest, nets, exact=kind == "exact")
    rng = np.random.RandomState(5)
    for player in (0, 1):
        nodes = forest.level_nodes(player)
        got_p, got_t = policy_at(ctx, wp, keys[nodes], player)
        assert np.array_equal(got_p.view(np.uint32), pol[nodes].view(np.uint32)) and np.array_equal(got_t, thr[nodes]), "every node of the player's levels"
        assert (np.abs(got_p.astype(np.float64) - ref[nodes]) <= tol[nodes]).all()
        if kind == "exact":
            assert np.array_equal(got_p, ref[nodes].astype(np.float32))
        if kind == "negative":
            assert not got_p.any() and (got_t[:, 0] == S.ZERO_SUM).all()
        for n in (1, 15, 17, 33):                                          # n % 16: a lone pair, ragged tiles either side of one and two tiles
            pick = nodes[rng.choice(len(nodes), n, replace=False)]
            p, t = policy_at(ctx, wp, keys[pick], player)
            assert np.array_equal(p.view(np.uint32), pol[pick].view(np.uint32)) and np.array_equal(t, thr[pick]), (player, n)
        perm = nodes[rng.permutation(len(nodes))]
        p, t = policy_at(ctx, wp, keys[perm], player)
        assert np.array_equal(p.view(np.uint32), pol[perm].view(np.uint32)) and np.array_equal(t, thr[perm]), "a permuted list"
        dup = nodes[rng.randint(0, 7, 40)]
        p, t = policy_at(ctx, wp, keys[dup], player)
        assert np.array_equal(p.view(np.uint32), pol[dup].view(np.uint32)) and np.array_equal(t, thr[dup]), "a list with duplicates"
    # n = 0 is a no-op; the refusals come before any launch
    L, vp, E = sl.lib(), sl.C.c_void_p, sl.SCOPA_EINVAL
    k = torch.tensor(keys[:16].view(np.int64), device="cuda")
    out_p = torch.full((16, 3), SENTINEL, dtype=torch.float32, device="cuda")
    out_t = torch.full((16, 2), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    args = lambda player=0, kp=k.data_ptr(), n=16, weights=wp, pp=out_p.data_ptr(), tp=out_t.data_ptr(), c=ctx._h: (
        c, player, vp(kp) if kp else None, n, *(vp(x) if x else None for x in weights), vp(pp) if pp else None, vp(tp) if tp else None)
    assert L.scopa_full_chance_sdcfr_policy_at(*args(n=0)) == sl.SCOPA_OK
    assert L.scopa_full_chance_sdcfr_policy_at(*args(n=0, kp=0, pp=0, tp=0)) == sl.SCOPA_OK
    assert L.scopa_full_chance_sdcfr_policy_at(*args(c=None)) == E
    assert L.scopa_full_chance_sdcfr_policy_at(*args(player=2)) == E and L.scopa_full_chance_sdcfr_policy_at(*args(player=-1)) == E
    assert L.scopa_full_chance_sdcfr_policy_at(*args(n=-1)) == E and L.scopa_full_chance_sdcfr_policy_at(*args(n=(1 << 28) + 1)) == E
    assert L.scopa_full_chance_sdcfr_policy_at(*args(kp=0)) == E and L.scopa_full_chance_sdcfr_policy_at(*args(pp=0)) == E
    assert L.scopa_full_chance_sdcfr_policy_at(*args(tp=0)) == E
    for i in range(6):
        assert L.scopa_full_chance_sdcfr_policy_at(*args(weights=wp[:i] + [0] + wp[i + 1:])) == E
    ctx.synchronize()
    assert (out_p.cpu().numpy() == SENTINEL).all() and (out_t.cpu().numpy() == -7).all()


# ---- 2. the traversal against the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r0,n,fix,batch,listed,kind", [(5, 3, None, 5, None, "mixed"), (4, 3, 0, 3, [2, 0], "mixed2"), (3, 2, 0, 2, None, "xavier")])
@pytest.mark.parametrize("trav", [0, 1])
def test_traversal_vs_restatement(ctx, sl, oracle, r0, n, fix, batch, listed, kind, trav):
    h, decks, acts, st = game(ctx, sl, oracle, r0, n, fix)
    R = 6 - r0
    w = dev_nets(NETS[kind]())
    m = n if listed is None else len(listed)
    rows = S.rows_per_traversal(R)
    ring = Ring(rows * m * batch + 7)
    write_base = ring.capacity - 3                                          # the call's rows wrap round the ring's end
    b0 = 1000 * trav
    vals = traverse(ctx, h, trav, batch, w, ring, write_base, iteration=3 + R, b0=b0, decks=listed)
    check_rows(st, decks, device_policy_fn(ctx, w), R, trav, batch, list(range(n)) if listed is None else listed, ring, write_base, vals, 3 + R, b0,
               (R, trav, batch, kind))
    assert h.sdcfr_visits() == m * batch * S.visits_per_traversal(R, trav)
    raises(sl, sl.SCOPA_ESTATE, h.sdcfr_policy_get)                          # no forest was built


# ---- 3. beyond the forest ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trav", [0, 1])
def test_five_rounds_vs_restatement(ctx, sl, oracle, trav):
    h, decks, acts, st = game(ctx, sl, oracle, 1, 2, 0)
    w = dev_nets(NETS["mixed"]())
    rows = S.rows_per_traversal(5)
    assert rows == 6220
    ring = Ring(rows * 2 + 5)
    vals = traverse(ctx, h, trav, 1, w, ring, ring.capacity - 2, iteration=8, b0=3)
    check_rows(st, decks, device_policy_fn(ctx, w), 5, trav, 1, [0, 1], ring, ring.capacity - 2, vals, 8, 3, ("R5", trav))
    assert h.sdcfr_visits() == 2 * (20215, 12440)[trav]
    raises(sl, sl.SCOPA_ELIMIT, G.traverse, ctx, h, trav, 1, w, ring, 0)     # the forest call still refuses R = 5


def test_the_deal_invariants(ctx, sl, oracle):
    deck = np.ascontiguousarray(oracle.full_deal_py_seed(42), np.uint8).reshape(1, 40)
    ctx.mccfr_seed(SEED)
    h = sl.FullChanceMCCFR(ctx, deck, state_of(sl, deck[0], []), 10)
    w = dev_nets(NETS["xavier"]())
    rows = S.rows_per_traversal(6)
    assert rows == 37324
    ring = Ring(rows + 9)
    vals = traverse(ctx, h, 1, 1, w, ring, 4)
    feat, regret = ring.host()
    assert (feat[:4] == SENTINEL).all() and (feat[4 + rows:] == SENTINEL).all() and (regret[:4] == SENTINEL).all() and (regret[4 + rows:] == SENTINEL).all()
    feat, regret = feat[4:4 + rows], regret[4:4 + rows]
    # a feature row is sdcfr_features of a pair: rebuild the pair from the row (hand, table, round, captured cards, scopas, player 1) and compare
    one = feat == 1.0
    bit = lambda cols, shift: (one[:, cols].astype(np.uint64) << (np.arange(cols.stop - cols.start, dtype=np.uint64) + np.uint64(shift))[None, :]).sum(1, dtype=np.uint64)
    rnd = one[:, 80:86].argmax(1).astype(np.uint64)
    A = (np.uint64(1) << np.uint64(63)) | (np.uint64(1) << np.uint64(62)) | (rnd << np.uint64(59)) | bit(slice(40, 80), 16) | \
        ((feat[:, 86] * 64).astype(np.uint64) << np.uint64(10)) | ((feat[:, 88] * 32).astype(np.uint64) << np.uint64(5)) | (feat[:, 87] * 32).astype(np.uint64)
    keys = np.stack([A, bit(slice(0, 40), 0)], 1)
    assert np.array_equal(sl.full_chance_sdcfr_features(keys).view(np.uint32), feat.view(np.uint32))
    # level-major ranks: traverser 1's levels 1 and 3 of round r hold 6^r and 3 * 6^r paths, with 3 and 2 cards
    held, at = feat[:, :40].sum(1), 0
    for r in range(6):
        for cards, width in ((3, 6 ** r), (2, 3 * 6 ** r)):
            assert (rnd[at:at + width] == r).all() and (held[at:at + width] == cards).all(), (r, cards)
            at += width
    assert at == rows
    not_held = np.where(feat[:, :40] == 0.0, regret, np.nan)
    assert (np.nanmax(not_held, 1) == np.nanmin(not_held, 1)).all() and np.abs(regret).max() <= 1.0 and np.isfinite(regret).all()
    assert np.isfinite(vals).all() and h.sdcfr_visits() == 74648


# ---- 4. independence of the chunking, the list and the deck count --------------------------------------------------------------------------------------
def test_chunk_seams_and_lists_change_no_bit(ctx, sl, oracle):
    h, decks, acts, st = game(ctx, sl, oracle, 4, 3, 0)
    batch, rows = 5, S.rows_per_traversal(2)
    w = dev_nets(NETS["mixed"]())
    per = rows * batch
    per_trav = 180 * 36 + 28 * rows                                         # bytes of one traversal at R = 2 (include/scopa.h)

    def run(listed=None, trav=1):
        m = 3 if listed is None else len(listed)
        ring = Ring(per * m)
        vals = traverse(ctx, h, trav, batch, w, ring, 0, decks=listed)
        f, r = ring.host()
        return f.reshape(m, per, 96), r.reshape(m, per, 40), vals.reshape(m, batch)

    same = lambda x, y: all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(x, y))
    try:
        h.debug_sdcfr_scratch(per_trav - 1)
        raises(sl, sl.SCOPA_EINVAL, run)                                      # a budget below one traversal
        h.debug_sdcfr_scratch(4 * per_trav + 100)                           # chunks of 4: seams inside deck 0's batch, between decks 1 and 2
        cut = [run(trav=t) for t in (0, 1)]
        h.debug_sdcfr_scratch(per_trav)                                     # a traversal a chunk
        ones = run()
    finally:
        h.debug_sdcfr_scratch(0)
    full = [run(trav=t) for t in (0, 1)]
    assert same(cut[0], full[0]) and same(cut[1], full[1]) and same(ones, full[1])
    assert same(run(), full[1]), "two runs"
    for listed in ([2, 0, 1], [1], [2, 0]):
        got = run(listed)
        for slot, deck in enumerate(listed):
            assert all(np.array_equal(a[slot].view(np.uint32), b[deck].view(np.uint32)) for a, b in zip(got, full[1])), (listed, slot)


def test_ninety_decks_at_three_rounds(ctx, sl, oracle):
    h, decks, acts, st = game(ctx, sl, oracle, 3, 90, 0)
    w = dev_nets(NETS["xavier"]())
    rows = S.rows_per_traversal(3)
    ring = Ring(rows * 90 + 1)
    raises(sl, sl.SCOPA_ELIMIT, G.traverse, ctx, h, 0, 1, w, ring, 0)        # 90 x 36^3 > 1 << 22
    vals = traverse(ctx, h, 0, 1, w, ring, 1, iteration=2, b0=11)
    check_rows(st, decks, device_policy_fn(ctx, w), 3, 0, 1, list(range(90)), ring, 1, vals, 2, 11, "deck 89", only={89})
    f, r = ring.host()
    assert (f[0] == SENTINEL).all() and (f[1:] != SENTINEL).any(1).all() and (r[1:] != SENTINEL).all()
    assert h.sdcfr_visits() == 90 * S.visits_per_traversal(3, 0)


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_memory_untouched(ctx, sl, oracle):
    h, decks, acts, st = game(ctx, sl, oracle, 5, 3, None)
    n, rows = 3, 4
    w = dev_nets(NETS["xavier"]())
    ring = Ring(rows * n * 2)
    vals = torch.full((n * 2,), SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    L, vp = sl.lib(), sl.C.c_void_p
    wp = [t.data_ptr() for t in w]

    def raw(handle=None, root=None, trav=0, batch=2, lst=None, m=None, weights=None, feat=None, regret=None, capacity=None, write_base=0, values=None, b0=0):
        handle = h._h if handle is None else handle
        lst = None if lst is None else np.ascontiguousarray(lst, np.int32)
        m = (0 if lst is None else lst.size) if m is None else m
        weights = wp if weights is None else weights
        return L.scopa_full_chance_sdcfr_traverse_frontier(handle, sl._ptr(root), trav, batch, m, sl._ptr(lst), *(vp(p) for p in weights),
                                                           vp(ring.feat.data_ptr() if feat is None else feat), vp(ring.regret.data_ptr() if regret is None else regret),
                                                           ring.capacity if capacity is None else capacity, write_base, vp(vals.data_ptr() if values is None else values), 3, b0)

    E = sl.SCOPA_EINVAL
    assert L.scopa_full_chance_sdcfr_traverse_frontier(None, None, 0, 2, 0, None, *(vp(p) for p in wp), vp(ring.feat.data_ptr()), vp(ring.regret.data_ptr()),
                                                       ring.capacity, 0, vp(vals.data_ptr()), 3, 0) == E
    assert raw(trav=2) == E and raw(trav=-1) == E
    assert raw(root=state_of(sl, decks[0], acts[:-1])) == E                  # mid-round
    assert raw(root=state_of(sl, decks[0], acts[:6])) == E                   # R = 5 is no limit here: the ring is too small for its 6 220 rows a traversal
    other = oracle.full_deal_py_seed(7)
    assert raw(root=state_of(sl, other, F.random_root(other, 5, np.random.RandomState(3))[1])) == E   # a root the handle's decks do not fit
    assert raw(lst=[0, 3]) == E and raw(lst=[1, 1]) == E and raw(lst=[-1]) == E and raw(lst=[0, 1, 2, 0]) == E and raw(m=2) == E and raw(lst=[0], m=0) == E
    assert raw(batch=0) == E and raw(batch=-1) == E and raw(batch=(1 << 24) + 1) == E
    for k in range(6):
        assert raw(weights=wp[:k] + [0] + wp[k + 1:]) == E
    assert raw(feat=0) == E and raw(regret=0) == E and raw(values=0) == E
    assert raw(feat=ring.feat.data_ptr() + 4) == E and raw(regret=ring.regret.data_ptr() + 8) == E
    assert raw(capacity=rows - 1, lst=[0], batch=1) == E                     # capacity < ROWS
    assert raw(capacity=rows * n * 2 - 1) == E                               # ROWS * m * batch > capacity
    assert raw(write_base=ring.capacity) == E and raw(write_base=-1) == E and raw(capacity=1 << 30) == E
    assert raw(b0=(1 << 32) - n * 2 + 1) == E                                # id overflow
    assert L.scopa_full_chance_debug_sdcfr_scratch(ctx._h, -1) == E and L.scopa_full_chance_debug_sdcfr_scratch(None, 0) == E
    ctx.synchronize()
    f, r = ring.host()
    assert (f == SENTINEL).all() and (r == SENTINEL).all() and (vals.cpu().numpy() == SENTINEL).all() and h.sdcfr_visits() == 0
    assert raw(b0=(1 << 32) - n * 2) == sl.SCOPA_OK                          # the last ids there are: a valid call after the refusals
    ctx.synchronize()
    f, r = ring.host()
    assert (f != SENTINEL).any(1).all() and (r != SENTINEL).all()
    check_rows(st, decks, device_policy_fn(ctx, w), 1, 0, 2, [0, 1, 2], ring, 0, vals.cpu().numpy(), 3, (1 << 32) - n * 2, "last ids")


# ---- 6. isolation ----------------------------------------------------------------------------------------------------------------------------------
def test_store_and_forest_form_are_left_alone(ctx, sl, oracle):
    h, decks, acts, st = game(ctx, sl, oracle, 4, 3, 0)
    w = dev_nets(NETS["mixed"]())
    rows = S.rows_per_traversal(2)
    h.iterate(2, 2)

    def forest_call():
        ring = Ring(rows * 3 * 2 + 3)
        vals = G.traverse(ctx, h, 1, 2, w, ring, 2)
        return [x.tobytes() for x in ring.host()] + [vals.tobytes()] + [x.tobytes() for x in h.sdcfr_policy_get()]

    before = forest_call()
    store = [x.tobytes() for x in h.tables_get()] + [h.counters()]
    visits = h.sdcfr_visits()
    ring = Ring(rows * 3 * 2)
    for trav in (0, 1):
        traverse(ctx, h, trav, 2, w, ring, 0)
    assert store == [x.tobytes() for x in h.tables_get()] + [h.counters()], "the frontier call touches neither the store nor the counters"
    assert h.sdcfr_visits() == visits + 3 * 2 * (S.visits_per_traversal(2, 0) + S.visits_per_traversal(2, 1))
    assert forest_call() == before, "the forest form's bits after frontier calls on the same handle"


# ---- 7. end to end ---------------------------------------------------------------------------------------------------------------------------------
def test_train_from_the_deal(sl, oracle):
    from scopa_amd.algorithms import packet_decks
    from scopa_amd.algorithms.deep_cfr import FullChanceDeepCFR
    deck = oracle.full_deal_py_seed(42)
    _, prefix = F.random_root(deck, 4, np.random.RandomState(442))
    decks = packet_decks(deck, 4, 4, 5, fix_seat=0)                          # four decks that share the deal's first four rounds
    with pytest.raises(ValueError):
        FullChanceDeepCFR(decks, root_actions=(), traversal="forest", batch=1, decks_per_iteration=1, seed=SEED)
    with pytest.raises(ValueError):
        FullChanceDeepCFR(decks, root_actions=(), traversal="levels", batch=1, decks_per_iteration=1, seed=SEED)
    d = FullChanceDeepCFR(decks, root_actions=(), traversal="frontier", batch=1, decks_per_iteration=1, seed=SEED)
    try:
        assert d.R == 6 and d.rows_per_traversal == 37324
        d.train(2, advantage_epochs=1)
        d._stream.synchronize()
        assert [a.buffer.total for a in d.advantage_nets] == [2 * 37324, 2 * 37324]
        assert d.solver.sdcfr_visits() == 2 * (121303 + 74648)
        e = d.exploitability(decks=decks[:2], root_actions=prefix)
        assert all(np.isfinite(e[k]) for k in ("exploitability", "br0", "br1", "value")) and e["exploitability"] >= 0
        with pytest.raises(ValueError, match="1 << 22"):
            d.exploitability()
        with pytest.raises(ValueError, match="1 << 22"):
            d.policy_store()
        mean, scopas = d.evaluate_vs_random(64, decks=decks[:2], root_actions=prefix)
        assert np.isfinite(mean) and len(scopas) == 2
    finally:
        d.close()
