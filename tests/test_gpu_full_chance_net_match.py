"""GPU checks of the Deep CFR nets in sampled matches on FullScopa over decks (scopa_full_chance_sdcfr_average_at, scopa_full_chance_sdcfr_match;
scopa_amd/csrc/scopa_full_chance_sdcfr.hip; FullChanceDeepCFR.average_policy_at / .match) against the forest's average policy, the store's match and
tests/full_chance_net_match_ref.py, which tests/test_full_chance_net_match_ref.py holds to full_chance_ref.match and a depth-first replay.

average_at is held to scopa_full_chance_sdcfr_average_policy's rows on bits and to the float64 average within full_chance_sdcfr_ref's propagated
tolerance; the match is held on bits to match / pair_match on policy_store() where the sub-game fits the sweeps (R = 1 on 3 decks, R = 2 on 5), and
beyond them (R = 5 and the deal, 40 episodes on 3 decks) to the restatement: with exact-arithmetic nets the restatement computes the rows itself, with
Xavier nets the trace is replayed on host states and every traced slot is held to the pick on the device's own row with the episode's draw."""
import numpy as np
import pytest
import torch

import full_chance_net_match_ref as M
import full_chance_ref as W
import full_chance_sdcfr_ref as S
import full_mccfr_ref as F

from test_gpu_full_chance_sdcfr import SEED, SHAPES, forest_of, packet, raises, state_of

pytestmark = pytest.mark.gpu

WIDE_SEED = 0x9E3779B97F4A7C15
SENTINEL = -7.0


# ---- helpers -----------------------------------------------------------------------------------------------------------------------------------------
class Snaps:
    """one player's snapshots on the device as the library takes them: six tensors [max_size][...], FIFO slots, float32 coefficients"""

    def __init__(self, nets, slots=None, max_size=None, weights=None):
        n = len(nets)
        self.nets = nets
        self.max_size = (n + 2) if max_size is None else max_size
        self.slots = [(3 * s + 1) % self.max_size for s in range(n)] if slots is None else list(slots)
        assert len(set(self.slots)) == n == len(self.slots)
        store = [np.zeros((self.max_size,) + sh, np.float32) for sh in S.SHAPES]
        for s, net in zip(self.slots, nets):
            for k in range(6):
                store[k][s] = net[k]
        self.store = [torch.tensor(t, device="cuda") for t in store]
        w = np.arange(2, 2 + n, dtype=np.float64) if weights is None else np.asarray(weights, np.float64)
        self.coef = np.array([x / w.sum() for x in w], np.float32)
        self.d_coef = torch.tensor(self.coef, device="cuda") if n else None
        torch.cuda.synchronize()

    @property
    def ptrs(self):
        return [t.data_ptr() for t in self.store]

    @property
    def args(self):
        """(slots, pointers, max_size, coefficient pointer): FullChanceMCCFR.sdcfr_match's form of a set"""
        return (self.slots, self.ptrs, self.max_size, self.d_coef.data_ptr() if self.slots else 0)


def average_at(ctx, snaps, keys2, player):
    keys2 = np.ascontiguousarray(keys2, np.uint64).reshape(-1, 2)
    n = len(keys2)
    k = torch.tensor(keys2.view(np.int64), device="cuda")
    out = torch.full((n, 3), SENTINEL, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ctx.full_chance_sdcfr_average_at(player, k.data_ptr(), n, *snaps.args, out.data_ptr())
    ctx.synchronize()
    return out.cpu().numpy()


def same(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def handle(ctx, sl, oracle, r0, n, fix, seed=SEED, capacity_log2=10):
    decks, acts, st = packet(oracle, r0, n, fix)
    ctx.mccfr_seed(seed)
    return sl.FullChanceMCCFR(ctx, decks, state_of(sl, decks[0], acts), capacity_log2), decks, acts, st


def device_rows_fn(ctx, sets):
    return lambda keys2, player: average_at(ctx, sets[player], keys2, player)


XAVIER3 = lambda base: [S.xavier_net(base + s, head_bias=0.1 - 0.04 * s) for s in range(3)]


# ---- 1. average_at against the forest's rows and float64 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1, 3, 40, "negative"])
def test_average_at_vs_the_forest_rows(ctx, sl, oracle, kind):
    r0, n, fix = SHAPES[2]
    h, decks, acts, st = handle(ctx, sl, oracle, r0, n, fix, capacity_log2=12)
    forest = forest_of(st, decks, 2)[0]
    if kind == "negative":
        nets = [S.negative_net(70), S.negative_net(71)]                    # every advantage negative under every snapshot: the uniform branch
    else:
        nets = [S.xavier_net(100 + s, head_bias=0.1 - 0.02 * (s % 7)) for s in range(kind)]
        if kind > 1:
            nets[1] = S.negative_net(77)                                    # a snapshot that adds nothing anywhere
    slots = list(range(41, 1, -1)) if kind == 40 else None                  # FIFO slots out of order, as a wrapped buffer has them
    snaps = Snaps(nets, slots=slots, max_size=44 if kind == 40 else None)
    assert kind in (0, 1) or snaps.slots != sorted(snaps.slots)
    rng = np.random.RandomState(5)
    worst = 0.0
    for player in (0, 1):
        keys, pol = h.sdcfr_average_policy(player, snaps.slots, snaps.ptrs, snaps.max_size, snaps.d_coef.data_ptr() if nets else 0)
        nodes = forest.level_nodes(player)
        assert np.array_equal(keys, forest.keys[nodes])
        got = average_at(ctx, snaps, keys, player)
        assert same(got, pol), "every node of the player's levels"
        held = M.held(keys)
        assert np.allclose(got.sum(1), 1.0, atol=1e-12) and (got >= 0).all() and not got[held == 2, 2].any()
        if kind in (0, "negative"):
            assert same(got, (np.arange(3)[None, :] < held[:, None]) / held[:, None].astype(np.float64))
        else:
            ref, tol, amb = S.average_policy(nets, snaps.coef, keys, forest.n_act[nodes])
            err = np.abs(got - ref)
            assert (err[~amb] <= tol[~amb]).all()
            worst = max(worst, float((err[~amb] / np.where(tol[~amb] > 0, tol[~amb], 1.0)).max()))
        for m in (1, 15, 17, 33):                                          # a lone pair, ragged tiles either side of one and two tiles
            pick = rng.choice(len(keys), m, replace=False)
            assert same(average_at(ctx, snaps, keys[pick], player), pol[pick]), (player, m)
        perm = rng.permutation(len(keys))
        assert same(average_at(ctx, snaps, keys[perm], player), pol[perm]), "a permuted list"
        dup = rng.randint(0, 7, 40)
        assert same(average_at(ctx, snaps, keys[dup], player), pol[dup]), "a list with duplicates"
        if kind == 3:
            # the work split: on 256 compute units a list of up to 4 096 pairs is a tile a workgroup.  20 003 pairs are 1 251 tiles: three a workgroup,
            # a ragged last tile, workgroups left without a share; 300 007 pairs are 18 751 tiles: 33 a workgroup, two batches of accumulators
            for m in (20003, 300007):
                idx = np.arange(m) % len(keys)
                assert same(average_at(ctx, snaps, keys[idx], player), pol[idx]), (player, m)
            # ... and forced at a short list (1 000 pairs, 63 tiles): one workgroup (two batches), 7 of nine tiles, 40 of which 8 have none, one a tile
            idx = rng.randint(0, len(keys), 1000)
            try:
                for grid in (1, 7, 40, 100):
                    ctx.full_chance_debug_sdcfr_average_grid(grid)
                    assert same(average_at(ctx, snaps, keys[idx], player), pol[idx]), (player, "grid", grid)
            finally:
                ctx.full_chance_debug_sdcfr_average_grid(0)
    print(f"kind={kind}: average_at max |device - float64| / tolerance = {worst:.4f}")


def test_average_at_refusals(ctx, sl, oracle):
    h, decks, acts, st = handle(ctx, sl, oracle, 5, 3, None)
    snaps = Snaps(XAVIER3(30))
    keys = W.subgame_keys(st, decks)
    keys = keys[((keys[:, 0] >> np.uint64(62)) & np.uint64(1)) == 0][:16]
    k = torch.tensor(np.ascontiguousarray(keys).view(np.int64), device="cuda")
    out = torch.full((16, 3), SENTINEL, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    L, vp, E = sl.lib(), sl.C.c_void_p, sl.SCOPA_EINVAL
    slots = np.array(snaps.slots, np.int32)

    def raw(c=ctx._h, player=0, kp=k.data_ptr(), n=16, n_snap=3, weights=snaps.ptrs, sl_=slots, max_size=snaps.max_size, coef=snaps.d_coef.data_ptr(), pp=out.data_ptr()):
        return L.scopa_full_chance_sdcfr_average_at(c, player, vp(kp) if kp else None, n, n_snap, *(vp(x) if x else None for x in weights), sl._ptr(sl_), max_size,
                                                    vp(coef) if coef else None, vp(pp) if pp else None)

    assert raw(n=0) == sl.SCOPA_OK and raw(n=0, kp=0, pp=0) == sl.SCOPA_OK
    assert raw(c=None) == E and raw(player=2) == E and raw(player=-1) == E and raw(n=-1) == E and raw(n=(1 << 28) + 1) == E
    assert raw(kp=0) == E and raw(pp=0) == E and raw(kp=k.data_ptr() + 8) == E and raw(pp=out.data_ptr() + 4) == E
    assert raw(n_snap=-1) == E and raw(n_snap=snaps.max_size + 1) == E and raw(sl_=None) == E and raw(coef=0) == E
    assert raw(sl_=np.array([1, 4, snaps.max_size], np.int32)) == E and raw(sl_=np.array([1, -1, 2], np.int32)) == E
    for i in range(6):
        assert raw(weights=snaps.ptrs[:i] + [0] + snaps.ptrs[i + 1:]) == E   # NULL weights with n_snap > 0
    ctx.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()
    assert raw(n_snap=0, weights=[0] * 6, sl_=None, coef=0, max_size=0) == sl.SCOPA_OK   # no snapshots: no tensors needed
    ctx.synchronize()
    assert np.allclose(out.cpu().numpy().sum(1), 1.0)


# ---- 2. the match against policy_store(...), on bits ---------------------------------------------------------------------------------------------------
def deep_on(sl, decks, acts, n_snap=3, capacity_log2=14):
    from scopa_amd.algorithms import FullChanceMCCFRTrainer
    from scopa_amd.algorithms.deep_cfr import FullChanceDeepCFR
    stream = torch.cuda.Stream(device=0)
    c = sl.Context(0, stream=stream.cuda_stream)
    t = FullChanceMCCFRTrainer(decks=decks, root_actions=acts, capacity_log2=capacity_log2, batch=2, ctx=c)
    d = FullChanceDeepCFR(t, seed=SEED)
    with torch.cuda.stream(stream):
        for player in (0, 1):
            for it in range(n_snap):
                net = S.xavier_net(21 + it + 10 * player, head_bias=0.05 * it)
                d.strategy_buffers[player].add_strategy(None, it + 1, params=[torch.tensor(a, device="cuda") for a in net])
    stream.synchronize()
    return d, t, c


@pytest.mark.parametrize("R,n_snap", [(1, 3), (2, 3), (2, 0)])
def test_match_equals_the_store_match_on_bits(sl, oracle, R, n_snap):
    r0, n_decks, fix = SHAPES[R]
    all_decks, acts, st = packet(oracle, r0, 2 * n_decks, fix)
    decks, held = all_decks[:n_decks], all_decks[n_decks:]
    d, t, c = deep_on(sl, decks, acts, n_snap)
    from scopa_amd.algorithms import FullChanceMCCFRTrainer
    empty = FullChanceMCCFRTrainer(decks=decks, root_actions=acts, capacity_log2=4, batch=1, ctx=c)
    stores = [empty]
    try:
        t.train(3)                                                          # the opponent store: a few MCCFR iterations on the training decks
        twice = np.stack([decks[0], decks[1], decks[0]])                    # a deck listed twice
        for on in (None, twice, held):
            s = d.policy_store(decks=on)
            stores.append(s)
            for n in (1, 2, 33, 70):                                        # odd halves and tile seams
                got, r2 = d.match(n, decks=on, stream_id=3 + n, per_episode=True)
                want, want_r2 = s.solver.match(n, 3 + n, on, per_episode=True)
                assert np.array_equal(got["sums"], want) and np.array_equal(r2, want_r2), (R, n, "uniform opponent")
                if n_snap == 0:                                             # no snapshots: the match on an empty store
                    want, want_r2 = empty.solver.match(n, 3 + n, on, per_episode=True)
                    assert np.array_equal(got["sums"], want) and np.array_equal(r2, want_r2), (R, n, "empty store")
                got, r2 = d.match(n, opponent=t, decks=on, stream_id=n, per_episode=True)
                want, want_r2 = s.solver.pair_match(t.solver, n, n, on, per_episode=True)
                assert np.array_equal(got["sums"], want) and np.array_equal(r2, want_r2), (R, n, "store opponent")
            assert got["exact_reward"] is not None and np.isfinite(got["exact_reward"]) and got["exact_std_error"] > 0   # inside the sweeps: the exact fields
        assert d.match(0)["episodes"] == 0
        # average_policy_at carries policy_rows' bits
        keys, n_act, pol = d.policy_rows()
        for player in (0, 1):
            mine = ((keys[:, 0] >> np.uint64(62)) & np.uint64(1)) == player
            assert same(d.average_policy_at(keys[mine], player), pol[mine])
        with pytest.raises(ValueError):
            d.match(4, opponent="random")
    finally:
        for s in stores:
            s.close()
        d.close()
        t.close()
        c.close()


def test_match_from_a_later_root_and_against_nets(sl, oracle):
    """root_actions moves the match's root: the episodes of policy_store(root_actions=...)'s match; a second FullChanceDeepCFR as the opponent plays
    pair_match against ITS policy_store"""
    r0, n_decks, fix = SHAPES[2]
    decks, acts, st = packet(oracle, r0, n_decks, fix)
    d, t, c = deep_on(sl, decks, acts[:18], 3, capacity_log2=18)                              # the solver stands at round 3; the match is asked at round 4
    from scopa_amd.algorithms.deep_cfr import FullChanceDeepCFR
    other = FullChanceDeepCFR(t, seed=SEED + 1)
    stores = []
    try:
        assert d.R == 3
        with torch.cuda.stream(d._stream):
            for player in (0, 1):
                other.strategy_buffers[player].add_strategy(None, 1, params=[torch.tensor(a, device="cuda") for a in S.xavier_net(60 + player)])
        d._stream.synchronize()
        t.train(2)                                                          # rows for the store opponent, from the round-3 root
        s = d.policy_store(decks=decks, root_actions=acts)
        o = other.policy_store(decks=decks, root_actions=acts)
        stores += [s, o]
        for n in (2, 33):
            got, r2 = d.match(n, decks=decks, root_actions=acts, stream_id=9, per_episode=True)
            want, want_r2 = s.solver.match(n, 9, per_episode=True)
            assert np.array_equal(got["sums"], want) and np.array_equal(r2, want_r2)
            got, r2 = d.match(n, opponent=other, decks=decks, root_actions=acts, stream_id=9, per_episode=True)
            want, want_r2 = s.solver.pair_match(o.solver, n, 9, per_episode=True)
            assert np.array_equal(got["sums"], want) and np.array_equal(r2, want_r2)
            assert got["exact_reward"] is not None
            # a store opponent that stands at another root (round 3): its rows are by pair, the match and the exact fields are taken at round 4
            got, r2 = d.match(n, opponent=t, decks=decks, root_actions=acts, stream_id=9, per_episode=True)
            want, want_r2 = s.solver.pair_match(t.solver, n, 9, per_episode=True)
            assert np.array_equal(got["sums"], want) and np.array_equal(r2, want_r2)
            assert got["exact_reward"] is not None and np.isfinite(got["exact_reward"])
        # from the solver's own root, 3 rounds on 5 decks: inside the sweeps too
        got = d.match(16, stream_id=1)
        assert got["exact_reward"] is not None and got["episodes"] == 16
    finally:
        for x in stores:
            x.close()
        other.close()
        d.close()
        t.close()
        c.close()


# ---- 3. beyond the sweeps: R = 5 and the deal ----------------------------------------------------------------------------------------------------------
def beyond(ctx, sl, oracle, r0, seed=SEED):
    if r0 == 0:
        from scopa_amd.algorithms import packet_decks
        deck = np.ascontiguousarray(oracle.full_deal_py_seed(42), np.uint8)
        decks = packet_decks(deck, 0, 3, 5)
        ctx.mccfr_seed(seed)
        return sl.FullChanceMCCFR(ctx, decks, state_of(sl, decks[0], []), 10), decks, F.root_of(decks[0])
    h, decks, acts, st = handle(ctx, sl, oracle, r0, 3, 0, seed=seed)
    return h, decks, st


@pytest.mark.parametrize("r0", [1, 0])
def test_exact_nets_vs_the_restatement(ctx, sl, oracle, r0):
    h, decks, st = beyond(ctx, sl, oracle, r0)
    sets = [Snaps([S.exact_net(7)], weights=[1.0]), Snaps([S.exact_net(8)], weights=[1.0])]
    assert sets[0].coef.tolist() == [1.0]
    host = M.host_rows_fn([(s.nets, s.coef) for s in sets], exact=True)
    sums, r2, trace = h.sdcfr_match(40, [s.args for s in sets], None, 4, per_episode=True, trace=True)
    want = M.match_levels(st, decks, 40, SEED, host, None, stream_id=4)
    assert np.array_equal(sums, want[0]) and np.array_equal(r2, want[1]) and np.array_equal(trace, want[2])
    raises(sl, sl.SCOPA_ELIMIT, h.sdcfr_average_policy, 0, [], [0] * 6, 0, 0)   # the forest route still refuses this root


@pytest.mark.parametrize("r0", [1, 0])
def test_xavier_nets_replayed_on_host_states(ctx, sl, oracle, r0):
    h, decks, st = beyond(ctx, sl, oracle, r0)
    sets = [Snaps(XAVIER3(40)), Snaps(XAVIER3(50))]
    n = 40
    sums, r2, trace = h.sdcfr_match(n, [s.args for s in sets], None, 6, per_episode=True, trace=True)
    got = M.replay(st, decks, n, trace)                                     # every traced slot is legal; the rewards and scopas are the states'
    assert np.array_equal(got[0], sums) and np.array_equal(got[1], r2)
    # every traced slot against the pick on average_at's row at that pair with that draw (uniform play at the opponent's nodes)
    rows = {}
    for player in (0, 1):
        pairs = sorted({key for i, met in enumerate(got[2]) for lv, p, key, step in met if p == player and p == (0 if 2 * i < n else 1)})
        rows.update(zip(pairs, average_at(ctx, sets[player], np.array(pairs, np.uint64), player)))
    checked = 0
    for i, met in enumerate(got[2]):
        seat = 0 if 2 * i < n else 1
        assert len(met) == 4 * (6 - r0)
        for lv, p, key, step in met:
            nl = int(M.held([key])[0])
            prob = M.probs_of(rows[key], nl) if p == seat else [1.0 / nl] * nl
            assert F.pick(prob, M.draw(SEED, i, 6, step)) == trace[i, lv], (i, lv)
            checked += 1
    assert checked == n * 4 * (6 - r0)


def test_nets_against_nets_swap_seats(ctx, sl, oracle):
    """One net set on both sides: the game of episode i does not depend on who is called the agent, so an episode that sits in seat 0 in one call and in
    seat 1 in another (same id, same deck: 40 and 12 episodes on 3 decks put ids 6..11 on deck i % 3 in either) carries the negated reward"""
    h, decks, st = beyond(ctx, sl, oracle, 1)
    sets = [Snaps(XAVIER3(40)), Snaps(XAVIER3(50))]
    args = [s.args for s in sets]
    a = h.sdcfr_match(40, args, args, 2, per_episode=True, trace=True)
    b = h.sdcfr_match(12, args, args, 2, per_episode=True, trace=True)
    assert np.array_equal(a[2][6:12], b[2][6:12]) and np.array_equal(a[1][6:12], -b[1][6:12]) and np.array_equal(a[2][:6], b[2][:6])
    assert a[1].any()
    want = M.match_levels(st, decks, 12, SEED, device_rows_fn(ctx, sets), ("nets", device_rows_fn(ctx, sets)), stream_id=2)
    assert np.array_equal(b[0], want[0]) and np.array_equal(b[1], want[1]) and np.array_equal(b[2], want[2])


# ---- 4. chunk seams, wide Philox words -----------------------------------------------------------------------------------------------------------------
def test_chunk_seams_change_no_bit(ctx, sl, oracle):
    r0, n_decks, fix = SHAPES[2]
    h, decks, acts, st = handle(ctx, sl, oracle, r0, n_decks, fix)
    sets = [Snaps(XAVIER3(40)), Snaps(XAVIER3(50))]
    args = [s.args for s in sets]
    run = lambda opp: h.sdcfr_match(70, args, opp, 5, per_episode=True, trace=True)
    full = [run(None), run(args)]
    try:
        h.debug_sdcfr_scratch(199)
        raises(sl, sl.SCOPA_EINVAL, run, None)                               # a budget below one episode's 200 bytes
        h.debug_sdcfr_scratch(200 * 24 + 7)                                  # chunks of 24, 24, 22: the seat seam (episode 35) inside the second
        cut = [run(None), run(args)]
        h.debug_sdcfr_scratch(200)                                           # an episode a chunk
        ones = run(None)
        h.debug_sdcfr_scratch(0)
        ctx.full_chance_debug_sdcfr_average_grid(2)                          # 35 episodes a seat are 3 tiles: two workgroups, of two tiles and of one
        split = [run(None), run(args)]
    finally:
        h.debug_sdcfr_scratch(0)
        ctx.full_chance_debug_sdcfr_average_grid(0)
    for x, y in zip(split, full):
        assert all(np.array_equal(p, q) for p, q in zip(x, y)), "the grid changes no bit"
    for x, y in zip(full + [full[0]], cut + [ones]):
        assert all(np.array_equal(p, q) for p, q in zip(x, y))
    assert all(np.array_equal(p, q) for p, q in zip(run(None), full[0])), "two runs"


def test_wide_philox_words_reach_the_draw(ctx, sl, oracle):
    r0, n_decks, fix = SHAPES[2]
    h, decks, acts, st = handle(ctx, sl, oracle, r0, n_decks, fix, seed=WIDE_SEED)
    sets = [Snaps([S.exact_net(7)], weights=[1.0]), Snaps([S.exact_net(8)], weights=[1.0])]
    host = M.host_rows_fn([(s.nets, s.coef) for s in sets], exact=True)
    stream = (1 << 24) - 1
    try:
        got = h.sdcfr_match(40, [s.args for s in sets], None, stream, per_episode=True, trace=True)
    finally:
        ctx.mccfr_seed(SEED)
    want = M.match_levels(st, decks, 40, WIDE_SEED, host, None, stream_id=stream)
    assert all(np.array_equal(p, q) for p, q in zip(got, want))
    for cut in (dict(seed_bits=32), dict(stream_bits=16)):                  # (the guard: the expectation moves with either cut)
        assert not np.array_equal(M.match_levels(st, decks, 40, WIDE_SEED, host, None, stream_id=stream, **cut)[2], want[2])


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------------------
def test_match_refusals_leave_the_sums_untouched(ctx, sl, oracle):
    h, decks, acts, st = handle(ctx, sl, oracle, 5, 3, None)
    sets = [Snaps(XAVIER3(40)), Snaps(XAVIER3(50))]
    L, vp, E = sl.lib(), sl.C.c_void_p, sl.SCOPA_EINVAL
    sums = np.full(6, 77, np.int64)

    def sets_of(edit=None):
        arr = (sl.FullSdcfrSnapshots * 2)()
        for q, s in enumerate(sets):
            arr[q].n_snap, arr[q].max_size = len(s.slots), s.max_size
            for name, ptr in zip(("d_w1", "d_b1", "d_w2", "d_b2", "d_w3", "d_b3"), s.ptrs):
                setattr(arr[q], name, ptr)
            arr[q].h_slots, arr[q].d_coef = s._slots.ctypes.data, s.d_coef.data_ptr()
        if edit:
            edit(arr)
        return arr

    for s in sets:
        s._slots = np.array(s.slots, np.int32)

    def raw(handle=h._h, n=8, stream_id=0, held=None, k=0, agent=True, edit=None, store=None, nets=False, out=sums):
        a = sets_of(edit)
        b = sets_of()
        return L.scopa_full_chance_sdcfr_match(handle, n, stream_id, sl._ptr(held), k, sl.C.cast(a, vp) if agent else None, store,
                                               sl.C.cast(b, vp) if nets else None, sl._ptr(out), None, None)

    other_ctx = sl.Context(0)
    other = sl.FullChanceMCCFR(other_ctx, decks, state_of(sl, decks[0], acts), 6)
    same_ctx = sl.FullChanceMCCFR(ctx, decks, state_of(sl, decks[0], acts), 6)
    try:
        assert raw(handle=None) == E and raw(n=-1) == E and raw(n=(1 << 36) + 1) == E and raw(stream_id=1 << 24) == E and raw(out=None) == E
        assert raw(held=decks, k=0) == E and raw(held=decks, k=(1 << 20) + 1) == E
        foreign = np.ascontiguousarray(oracle.full_deal_py_seed(7), np.uint8).reshape(1, 40)
        assert raw(held=foreign, k=1) == E                                    # a held-out deck that does not fit the root
        assert raw(agent=False) == E
        assert raw(store=other._h) == E                                       # an opponent store on another context
        assert raw(store=same_ctx._h, nets=True) == E                         # both kinds of opponent
        for name in ("d_w1", "d_b1", "d_w2", "d_b2", "d_w3", "d_b3", "h_slots", "d_coef"):
            assert raw(edit=lambda arr, name=name: setattr(arr[1], name, None)) == E, name   # NULL weights with n_snap > 0
        assert raw(edit=lambda arr: setattr(arr[0], "n_snap", arr[0].max_size + 1)) == E and raw(edit=lambda arr: setattr(arr[0], "n_snap", -1)) == E
        assert raw(edit=lambda arr: setattr(arr[0], "max_size", 2)) == E      # a slot outside [0, max_size)
        assert (sums == 77).all()
        assert raw(store=same_ctx._h) == sl.SCOPA_OK and sums[2] + sums[3] >= 0 and not (sums == 77).all()
        sums[:] = 77
        assert raw(n=0) == sl.SCOPA_OK and not sums.any()
    finally:
        other.close()
        same_ctx.close()
        other_ctx.close()


# ---- 6. end to end: nets trained from the deal, measured from the deal ---------------------------------------------------------------------------------
def test_trained_from_the_deal_plays_from_the_deal(sl, oracle):
    from scopa_amd.algorithms import FullChanceMCCFRTrainer, packet_decks
    from scopa_amd.algorithms.deep_cfr import FullChanceDeepCFR
    deck = oracle.full_deal_py_seed(42)
    decks = packet_decks(deck, 0, 6, 5)
    d = FullChanceDeepCFR(decks[:4], root_actions=(), traversal="frontier", batch=1, decks_per_iteration=1, seed=SEED)
    t = None
    try:
        d.train(3, advantage_epochs=1)
        d._stream.synchronize()
        assert all(len(b._slots) == 2 for b in d.strategy_buffers)
        out, r2 = d.match(64, per_episode=True)
        assert out["episodes"] == 64 and out["exact_reward"] is None and out["exact_by_seat"] is None and np.isfinite(out["reward"]) and out["std_error"] > 0
        assert out["by_seat"][0]["episodes"] == 32 and int(out["sums"][0]) == int(r2[:32].sum()) and int(out["sums"][1]) == int(r2[32:].sum())
        held = d.match(64, decks=decks[4:], stream_id=1)
        assert held["exact_reward"] is None and np.isfinite(held["reward"])
        t = FullChanceMCCFRTrainer(decks=decks[:4], root_actions=(), capacity_log2=20, batch=1, ctx=d.trainer.ctx)
        t.train(1)
        vs = d.match(64, opponent=t)
        assert vs["exact_reward"] is None and np.isfinite(vs["reward"])
        with pytest.raises(ValueError, match="1 << 22"):
            d.policy_store()                                                # the existing methods still refuse the deal
    finally:
        if t is not None:
            t.close()
        d.close()
