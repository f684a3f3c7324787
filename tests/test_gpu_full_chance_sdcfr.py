"""GPU checks of Deep CFR on FullScopa over a set of decks (scopa_amd/csrc/scopa_full_chance_sdcfr.hip: scopa_full_chance_sdcfr_*) against the
restatement tests/full_chance_sdcfr_ref.py, which tests/test_full_chance_sdcfr_ref.py holds to a depth-first recursion over real states.

The policy table is held to the float64 forward pass within its propagated tolerance (bit for bit on exact-arithmetic nets); the walk is compared
GIVEN the device's own table and thresholds, so no draw is ambiguous and everything -- features, ring positions, sampled paths through the rows'
nodes, regrets, root values, visit counts -- is compared exactly.  Shapes, as the exact-CFR suite's: R = 1 on 3 decks (levels of 3, 9, 27, 54 nodes:
ragged tiles, a 3-lane root level), R = 2 on 5 decks, R = 3 on 2 decks; batches 1 and 5."""
import numpy as np
import pytest
import torch

import full_chance_exploit_ref as X
import full_chance_ref as W
import full_chance_sdcfr_ref as S
import full_mccfr_ref as F

pytestmark = pytest.mark.gpu

SEED = 0x5C09A
SHAPES = {1: (5, 3, None), 2: (4, 5, 0), 3: (3, 2, 0)}      # R -> (round of the root, decks, the seat whose root hand the packet fixes)
_SETS, _FORESTS = {}, {}
SENTINEL = -7.0


# ---- helpers (copies of tests/test_gpu_full_chance_cfr.py's, which stays as it is) ---------------------------------------------------------------
def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def packet(oracle, r0, n, fix_seat, deck_seed=42, shared_rounds=None):
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


def state_of(sl, deck, acts):
    ps = sl.FullState(deck=deck)
    for a in acts:
        ps.step(a)
    return ps.s


def raises(sl, status, fn, *args, **kw):
    with pytest.raises(sl.ScopaError) as e:
        fn(*args, **kw)
    assert e.value.status == status, e.value


# ---- helpers of this file --------------------------------------------------------------------------------------------------------------------------
def forest_of(st, decks, R):
    """the restatement's forest, expanded once per (root, decks)"""
    key = (bytes(st.s), np.ascontiguousarray(decks, np.uint8).tobytes())
    if key not in _FORESTS:
        tree = X.tree_of(st, decks, R)
        _FORESTS[key] = (S.Forest(tree, R), tree)
    return _FORESTS[key]


def solver_of(ctx, sl, oracle, R, capacity_log2=14):
    decks, acts, st = shape(oracle, R)
    ctx.mccfr_seed(SEED)
    return sl.FullChanceMCCFR(ctx, decks, state_of(sl, decks[0], acts), capacity_log2), forest_of(st, decks, R)[0], decks


NETS = {"xavier": lambda: [S.xavier_net(1), S.xavier_net(2)], "shifted": lambda: [S.xavier_net(3, head_bias=0.6), S.xavier_net(4, head_bias=-0.3)],
        "negative": lambda: [S.negative_net(5), S.negative_net(6)], "exact": lambda: [S.exact_net(7), S.exact_net(8)],
        "mixed": lambda: [S.xavier_net(9), S.negative_net(10)], "mixed2": lambda: [S.negative_net(11), S.xavier_net(12, head_bias=0.3)]}


def dev_nets(nets):
    """the two players' nets as the traversal call takes them: six device tensors [2][...]"""
    return [torch.tensor(np.stack([nets[0][k], nets[1][k]]), device="cuda") for k in range(6)]


class Ring:
    def __init__(self, capacity):
        self.capacity = capacity
        self.feat = torch.full((capacity, 96), SENTINEL, dtype=torch.float32, device="cuda")
        self.regret = torch.full((capacity, 40), SENTINEL, dtype=torch.float32, device="cuda")

    def host(self):
        return self.feat.cpu().numpy(), self.regret.cpu().numpy()


def traverse(ctx, h, trav, batch, w, ring, write_base, iteration=3, b0=0, decks=None, root=None):
    m = h.n_decks if decks is None else len(decks)
    vals = torch.full((m * batch,), SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    h.sdcfr_traverse(trav, batch, [t.data_ptr() for t in w], ring.feat.data_ptr(), ring.regret.data_ptr(), ring.capacity, write_base, vals.data_ptr(), iteration, b0,
                     decks, root)
    ctx.synchronize()
    return vals.cpu().numpy()


def ref_policy(forest, nets, exact=False):
    pol, tol = np.zeros((len(forest.keys), 3)), np.zeros((len(forest.keys), 3))
    for k in range(forest.L):
        s = slice(forest.off[k], forest.off[k + 1])
        pol[s], tol[s] = S.node_policy(nets[k & 1], forest.keys[s], forest.n_act[s], exact)
    return pol, tol


def check_rows(forest, pol, thr, trav, batch, decks_listed, ring, write_base, vals, iteration, b0, what):
    """every row of every traversal of a call against the restatement's walk over the device's own tables; the rest of the ring untouched"""
    feat, regret = ring.host()
    rows = S.rows_per_traversal(forest.R)
    touched = np.zeros(ring.capacity, bool)
    for slot, deck in enumerate(decks_listed):
        for i in range(batch):
            tid = (b0 + deck * batch + i) & 0xFFFFFFFF
            ref = S.walk(forest, pol, thr, trav, deck, tid, iteration, SEED)
            assert np.float32(vals[slot * batch + i]).tobytes() == np.float32(ref["value"]).tobytes(), (what, slot, i)
            assert ref["visits"] == S.visits_per_traversal(forest.R, trav)
            for rank, (idx, reg) in ref["rows"].items():
                pos = S.ring_row(write_base, rows, slot, batch, i, rank, ring.capacity)
                assert not touched[pos]
                touched[pos] = True
                assert regret[pos].tobytes() == reg.tobytes(), (what, slot, i, rank)
                assert np.array_equal(feat[pos], S.features_of(*forest.keys[idx])), (what, slot, i, rank)
    assert touched.sum() == rows * len(decks_listed) * batch
    assert (feat[~touched] == SENTINEL).all() and (regret[~touched] == SENTINEL).all(), what


# ---- 1. the policy table against float64 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,kind", [(1, "xavier"), (1, "shifted"), (1, "negative"), (1, "exact"), (2, "xavier"), (2, "shifted"), (2, "negative"), (2, "exact"),
                                    (3, "xavier"), (3, "exact")])
def test_policy_table_vs_float64(ctx, sl, oracle, R, kind):
    h, forest, decks = solver_of(ctx, sl, oracle, R)
    nets = NETS[kind]()
    rows = S.rows_per_traversal(R)
    ring = Ring(rows * len(decks))
    traverse(ctx, h, 0, 1, dev_nets(nets), ring, 0)
    pol, thr, keys = h.sdcfr_policy_get()
    assert np.array_equal(keys, forest.keys)
    ref, tol = ref_policy(forest, nets, exact=kind == "exact")
    err = np.abs(pol.astype(np.float64) - ref)
    ratio = float((err / np.where(tol > 0, tol, 1.0))[tol > 0].max()) if (tol > 0).any() else 0.0
    print(f"R={R} {kind}: policy table max |float32 - float64| / tolerance = {ratio:.4f}")
    if kind == "exact":
        assert np.array_equal(pol, ref.astype(np.float32)), "exact-arithmetic nets: the table is bit for bit"
    else:
        assert (err <= tol).all(), ratio
    if kind == "negative":
        assert not pol.any() and (thr[:, 0] == S.ZERO_SUM).all()            # the zero-sum branch at every node
    live = np.arange(3)[None, :] < forest.n_act[:, None]
    assert not pol[~live].any()
    assert np.array_equal(thr, S.thresholds_all(pol, forest.n_act)), "thresholds of the device's own float32 policy"
    assert h.sdcfr_visits() == len(decks) * S.visits_per_traversal(R, 0)


# ---- 2. the walk given the device's table ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,trav,batch,kind", [(1, 0, 1, "xavier"), (1, 1, 5, "mixed"), (1, 0, 5, "mixed2"), (2, 0, 5, "mixed"), (2, 1, 1, "shifted"), (2, 1, 5, "mixed2"),
                                               (2, 0, 1, "negative"), (3, 0, 1, "shifted"), (3, 1, 5, "mixed"), (3, 0, 5, "mixed2"), (3, 1, 1, "xavier")])
def test_walk_given_the_device_table(ctx, sl, oracle, R, trav, batch, kind):
    h, forest, decks = solver_of(ctx, sl, oracle, R)
    n, rows = len(decks), S.rows_per_traversal(R)
    ring = Ring(rows * n * batch + 7)
    write_base = ring.capacity - 3                                          # the call's rows wrap round the ring's end
    b0 = 1000 * trav
    vals = traverse(ctx, h, trav, batch, dev_nets(NETS[kind]()), ring, write_base, iteration=3 + R, b0=b0)
    pol, thr, _ = h.sdcfr_policy_get()
    check_rows(forest, pol, thr, trav, batch, list(range(n)), ring, write_base, vals, 3 + R, b0, (R, trav, batch, kind))
    assert h.sdcfr_visits() == n * batch * S.visits_per_traversal(R, trav)


# ---- 3. independence of the list, of m and of the run; root changes -----------------------------------------------------------------------------------
def test_lists_samples_and_reruns_are_bit_identical(ctx, sl, oracle):
    h, forest, decks = solver_of(ctx, sl, oracle, 2)
    n, batch, rows = len(decks), 5, S.rows_per_traversal(2)
    w = dev_nets(NETS["mixed"]())
    per = rows * batch

    def run(listed):
        m = n if listed is None else len(listed)
        ring = Ring(per * m)
        vals = traverse(ctx, h, 1, batch, w, ring, 0, decks=listed)
        f, r = ring.host()
        return f.reshape(m, per, 96), r.reshape(m, per, 40), vals.reshape(m, batch)

    full = run(None)
    again = run(None)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(full, again)), "two runs"
    for listed in ([4, 0, 2, 3, 1], [3, 1], [2]):
        got = run(listed)
        for slot, deck in enumerate(listed):
            for a, b in zip(got, full):
                assert np.array_equal(a[slot].view(np.uint32), b[deck].view(np.uint32)), (listed, slot)


def test_root_change_rebuilds_the_forest(ctx, sl, oracle):
    decks, acts, st = packet(oracle, 4, 3, None, shared_rounds=5)           # the decks share round 4's deal too: they fit a root one round on
    ctx.mccfr_seed(SEED)
    h = sl.FullChanceMCCFR(ctx, decks, state_of(sl, decks[0], acts), 12)
    forest2 = forest_of(st, decks, 2)[0]
    rng, st1, acts1 = np.random.RandomState(9), F.clone(W.root_on(st, decks[0])), list(acts)
    for _ in range(6):
        legal = st1.legal()
        acts1.append(int(legal[rng.randint(len(legal))]))
        st1.step(acts1[-1])
    forest1 = forest_of(st1, decks, 1)[0]
    w = dev_nets(NETS["xavier"]())

    def run(forest, root):
        ring = Ring(S.rows_per_traversal(forest.R) * 3 * 5 + 2)
        vals = traverse(ctx, h, 0, 5, w, ring, 1, root=root)
        pol, thr, keys = h.sdcfr_policy_get()
        assert np.array_equal(keys, forest.keys)
        check_rows(forest, pol, thr, 0, 5, [0, 1, 2], ring, 1, vals, 3, 0, forest.R)
        return ring.host(), vals

    first = run(forest2, None)
    run(forest1, state_of(sl, decks[0], acts1))
    back = run(forest2, None)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(first[0] + (first[1],), back[0] + (back[1],)))


# ---- 4. the average policy ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_snap", [1, 3, 40])
@pytest.mark.parametrize("held", [False, True])
def test_average_policy_vs_float64(ctx, sl, oracle, n_snap, held):
    r0, n, fix = SHAPES[2]
    all_decks, acts, st = packet(oracle, r0, 2 * n, fix)
    decks = all_decks[:n]
    ctx.mccfr_seed(SEED)
    h = sl.FullChanceMCCFR(ctx, decks, state_of(sl, decks[0], acts), 12)
    on = all_decks[n:] if held else decks
    forest = forest_of(st, on, 2)[0]
    max_size = n_snap + 2
    snaps = [S.xavier_net(100 + s, head_bias=0.1 - 0.02 * (s % 7)) for s in range(n_snap)]
    if n_snap > 1:
        snaps[1] = S.negative_net(77)                                       # a snapshot that adds nothing anywhere
    slots = [(3 * s + 1) % max_size for s in range(n_snap)] if n_snap < 40 else list(range(2, 42))
    assert len(set(slots)) == n_snap
    store = [np.zeros((max_size,) + sh, np.float32) for sh in S.SHAPES]
    for s, net in zip(slots, snaps):
        for k in range(6):
            store[k][s] = net[k]
    d_store = [torch.tensor(t, device="cuda") for t in store]
    weights = np.arange(2, 2 + n_snap, dtype=np.float64)
    coef = np.array([w / weights.sum() for w in weights], np.float32)
    d_coef = torch.tensor(coef, device="cuda")
    torch.cuda.synchronize()
    worst = 0.0
    for player in (0, 1):
        keys, pol = h.sdcfr_average_policy(player, slots, [t.data_ptr() for t in d_store], max_size, d_coef.data_ptr(), on if held else None)
        nodes = forest.level_nodes(player)
        assert np.array_equal(keys, forest.keys[nodes])
        ref, tol, amb = S.average_policy(snaps, coef, keys, forest.n_act[nodes])
        ok = ~amb
        err = np.abs(pol - ref)
        assert (err[ok] <= tol[ok]).all()
        worst = max(worst, float((err[ok] / np.where(tol[ok] > 0, tol[ok], 1.0)).max()))
        assert np.allclose(pol.sum(1), 1.0, atol=1e-12) and (pol >= 0).all()
        order = np.lexsort((keys[:, 1], keys[:, 0]))
        k_, p_ = keys[order], pol[order]
        same = (k_[1:] == k_[:-1]).all(1)
        assert same.any() or player == 1                                    # (the packet fixes seat 0's root hand: its root key is every deck's)
        assert np.array_equal(p_[1:][same].view(np.uint64), p_[:-1][same].view(np.uint64)), "equal keys carry equal bits"
    print(f"S={n_snap} held={held}: average policy max |device - float64| / tolerance = {worst:.4f}")


# ---- 5. the policy in a store -----------------------------------------------------------------------------------------------------------------------------
def deep_of(sl, oracle, R, **kw):
    from scopa_amd.algorithms import FullChanceMCCFRTrainer
    from scopa_amd.algorithms.deep_cfr import FullChanceDeepCFR
    decks, acts, st = shape(oracle, R)
    stream = torch.cuda.Stream(device=0)
    c = sl.Context(0, stream=stream.cuda_stream)
    t = FullChanceMCCFRTrainer(decks=decks, root_actions=acts, capacity_log2=12, batch=1, ctx=c)
    return FullChanceDeepCFR(t, seed=SEED, **kw), t, c, st, decks, stream


def test_policy_store_vs_exact_restatement(sl, oracle):
    from scopa_amd.algorithms.full_chance import cross_play
    d, t, c, st, decks, stream = deep_of(sl, oracle, 2, batch=1)
    try:
        tree = forest_of(st, decks, 2)[1]
        empty = t.exploitability()
        u = d.policy_store()
        assert same_bits([u.exploitability()[k] for k in ("exploitability", "br0", "br1", "value")],
                         [empty[k] for k in ("exploitability", "br0", "br1", "value")]), "no snapshots: the uniform policy, as an empty store plays"
        u.close()
        with torch.cuda.stream(stream):
            for player in (0, 1):
                for it, seed in enumerate((21, 22, 23)):
                    net = S.xavier_net(seed + 10 * player, head_bias=0.05 * it)
                    d.strategy_buffers[player].add_strategy(None, it + 1, params=[torch.tensor(a, device="cuda") for a in net])
        stream.synchronize()
        keys, n_act, pol = d.policy_rows()
        assert len(np.unique(keys, axis=0)) == len(keys) and (n_act == [bin(int(b)).count("1") for b in keys[:, 1]]).all()
        assert np.allclose(pol.sum(1), 1.0, atol=1e-12)
        s = d.policy_store()
        got = s.exploitability()
        ref = X.solve(tree, {}, X.table_of(keys, pol), 0)
        assert same_bits([got[k] for k in ("exploitability", "br0", "br1", "value")], ref["out4"])
        xp = cross_play([s, t])
        assert same_bits(xp[0][0][0], ref["out4"][3]) and same_bits(xp[1][1][0], empty["value"])
        assert same_bits(d.exploitability()["exploitability"], ref["out4"][0])
        pr = d.get_policy(_root_state(sl, decks[0], t.root_actions), 0)
        assert abs(sum(pr.values()) - 1.0) < 1e-6 and len(pr) == 3
        s.close()
    finally:
        t.close()
        c.close()


def _root_state(sl, deck, acts):
    ps = sl.FullState(deck=deck)
    for a in acts:
        ps.step(a)
    return ps


# ---- 6. the handle's other calls --------------------------------------------------------------------------------------------------------------------------
def test_other_handle_calls_keep_their_bits(ctx, sl, oracle):
    """cfr_iterate, exploitability and the store's words on bits; the sampled iterate -- whose float64 atomic adds have no fixed order when decks share
    a pair -- on its exact integers, its key set and to rounding"""
    def run(interleave):
        h, forest, decks = solver_of(ctx, sl, oracle, 1, capacity_log2=10)
        w = dev_nets(NETS["xavier"]())
        ring = Ring(4 * 3 * 5)
        out = []
        if interleave:
            traverse(ctx, h, 0, 5, w, ring, 0)
        out.append(h.cfr_iterate(3))
        if interleave:
            before = [x.tobytes() for x in h.tables_get()] + [h.counters()]
            traverse(ctx, h, 1, 5, w, ring, 0)
            assert before == [x.tobytes() for x in h.tables_get()] + [h.counters()], "the traversal touches neither the store nor the counters"
        e = h.exploitability()
        out.append(np.array([e[k] for k in ("exploitability", "br0", "br1", "value")]))
        out.extend(h.tables_get())
        if interleave:
            traverse(ctx, h, 0, 5, w, ring, 0)
        h.iterate(2, 2)
        sampled = h.tables_get()
        counters = h.counters()
        h.close()
        return out, sampled, counters

    a, sa, ca = run(False)
    b, sb, cb = run(True)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
    assert ca == cb and np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1])
    assert np.allclose(sa[2], sb[2], rtol=1e-12, atol=1e-12) and np.allclose(sa[3], sb[3], rtol=1e-12, atol=1e-12)


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_memory_untouched(ctx, sl, oracle):
    h, forest, decks = solver_of(ctx, sl, oracle, 1)
    _, acts, _ = shape(oracle, 1)
    n, rows = len(decks), 4
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
        return L.scopa_full_chance_sdcfr_traverse(handle, sl._ptr(root), trav, batch, m, sl._ptr(lst), *(vp(p) for p in weights),
                                                  vp(ring.feat.data_ptr() if feat is None else feat), vp(ring.regret.data_ptr() if regret is None else regret),
                                                  ring.capacity if capacity is None else capacity, write_base, vp(vals.data_ptr() if values is None else values), 3, b0)

    E, LIM = sl.SCOPA_EINVAL, sl.SCOPA_ELIMIT
    assert L.scopa_full_chance_sdcfr_traverse(None, None, 0, 2, 0, None, *(vp(p) for p in wp), vp(ring.feat.data_ptr()), vp(ring.regret.data_ptr()), ring.capacity, 0,
                                              vp(vals.data_ptr()), 3, 0) == E
    assert raw(trav=2) == E and raw(trav=-1) == E
    assert raw(root=state_of(sl, decks[0], acts[:-1])) == E                  # mid-round
    assert raw(root=state_of(sl, decks[0], acts[:6])) == LIM                 # R = 5
    assert raw(root=state_of(sl, decks[0], acts[:12])) == LIM                # R = 4 on 3 decks: 3 x 36^4 > 1 << 22
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
    assert L.scopa_full_chance_sdcfr_visits(h._h, None) == E
    raises(sl, sl.SCOPA_ESTATE, h.sdcfr_policy_get)
    ctx.synchronize()
    f, r = ring.host()
    assert (f == SENTINEL).all() and (r == SENTINEL).all() and (vals.cpu().numpy() == SENTINEL).all() and h.sdcfr_visits() == 0
    many, acts3, _ = packet(oracle, 3, 90, 0)                                # 90 x 36^3 > 1 << 22: one deck over the cap
    big = sl.FullChanceMCCFR(ctx, many, state_of(sl, many[0], acts3), 10)
    raises(sl, LIM, big.sdcfr_traverse, 0, 1, wp, ring.feat.data_ptr(), ring.regret.data_ptr(), ring.capacity, 0, vals.data_ptr(), 0)
    raises(sl, LIM, big.sdcfr_average_policy, 0, [], [0] * 6, 0, 0)
    raises(sl, E, h.sdcfr_average_policy, 2, [], [0] * 6, 0, 0)
    raises(sl, E, h.sdcfr_average_policy, 0, [5], wp, 4, vals.data_ptr())   # a slot outside [0, max_size)
    assert raw(b0=(1 << 32) - n * 2) == sl.SCOPA_OK                          # the last ids there are: a valid call after the refusals
    ctx.synchronize()
    pol, thr, _ = h.sdcfr_policy_get()
    f, r = ring.host()
    assert (f != SENTINEL).all() and (r != SENTINEL).all()
    v = vals.cpu().numpy()
    check_rows(forest, pol, thr, 0, 2, [0, 1, 2], ring, 0, v, 3, (1 << 32) - n * 2, "last ids")


# ---- 8. end to end ------------------------------------------------------------------------------------------------------------------------------------------
def test_train_end_to_end(sl, oracle):
    """from decks alone: the solver makes its own stream, context and trainer"""
    from scopa_amd.algorithms.deep_cfr import FullChanceDeepCFR
    decks, acts, _ = shape(oracle, 1)
    d = FullChanceDeepCFR(decks, root_actions=acts, batch=5, decks_per_iteration=2, seed=SEED)
    try:
        d.train(3, advantage_epochs=2, exploitability_freq=2)
        d._stream.synchronize()
        per = S.rows_per_traversal(1) * 2 * 5
        assert [a.buffer.total for a in d.advantage_nets] == [3 * per, 3 * per]
        assert d.training_history["buffer_sizes"] == [[per, 2 * per, 3 * per]] * 2
        assert [it for it, _ in d.training_history["exploitability"]] == [0, 2] and all(np.isfinite(e) and e >= 0 for _, e in d.training_history["exploitability"])
        for a in d.advantage_nets:
            assert all(torch.isfinite(p).all() for p in a.param_list())
            f = a.buffer.feat[:3 * per].cpu().numpy()
            assert ((f[:, :40].sum(1) == 2) | (f[:, :40].sum(1) == 3)).all()
        assert [len(b._slots) for b in d.strategy_buffers] == [2, 2]
        assert [len(x[1]) for x in d.deck_log] == [2, 2, 2] and d.solver.sdcfr_visits() == 3 * 2 * 5 * (13 + 8)
        assert d.trainer.counters()["rows"] == 0                             # the trainer's own store is left alone
        # the TRAINED nets: their table against float64, and a walk over it on bits
        forest = forest_of(shape(oracle, 1)[2], decks, 1)[0]
        with torch.cuda.stream(d._stream):
            w = [x.clone() for x in d._stacked_weights()]
        d._stream.synchronize()
        nets = [[p.detach().cpu().numpy() for p in a.param_list()] for a in d.advantage_nets]
        ring = Ring(S.rows_per_traversal(1) * 3 * 5 + 3)
        vals = traverse(d.trainer.ctx, d.solver, 1, 5, w, ring, ring.capacity - 2, iteration=9, b0=7)
        pol, thr, _ = d.solver.sdcfr_policy_get()
        ref, tol = ref_policy(forest, nets)
        assert (np.abs(pol.astype(np.float64) - ref) <= tol).all() and pol.any()
        check_rows(forest, pol, thr, 1, 5, [0, 1, 2], ring, ring.capacity - 2, vals, 9, 7, "trained nets")
        # a run cut into calls with resume=True snapshots as one long call does
        d.train(2, advantage_epochs=1, resume=True)
        assert [len(b._slots) for b in d.strategy_buffers] == [4, 4] and d.strategy_buffers[0].weights == [2, 3, 4, 5]
    finally:
        d.close()
