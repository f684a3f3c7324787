"""Deep CFR over a set of deals on the GPU: scopa_chance_sdcfr_traverse (k_chance_sdcfr_policy, k_chance_sdcfr_walk), scopa_chance_sdcfr_average_policy
(k_chance_sdcfr_avg_terms / _reduce over the keys' representative nodes) and ChanceDeepCFR.

The reference of every kernel test is the single-deal entry point on a context that holds the deal under the same seed -- scopa_sdcfr_traverse_fused,
scopa_sdcfr_average_policy -- which the reference fixtures already pin; the contract is equality bit for bit (np.array_equal), so no tolerance enters.
The six-deal set and the held-out deal are those of tests/test_gpu_chance_mccfr.py, its counts asserted first."""
import ctypes as C

import numpy as np
import pytest

import philox_words as W

pytestmark = pytest.mark.gpu

SEED = W.CH_SEED
ITERATION, B0 = W.CH_ITERATION, 1000
NET_SEED = 20240611
SENTINEL = -7.5


def _perm(h0, h1):
    return h0 + h1 + [c for c in range(16) if c not in h0 + h1]


SIX = np.array([_perm([0, 5, 10, 15], h) for h in ([1, 2, 3, 4], [1, 2, 3, 6], [1, 2, 7, 6], [9, 8, 7, 6])] +
               [_perm([0, 5, 10, 14], h) for h in ([1, 2, 3, 4], [9, 8, 7, 6])], np.uint8)
HELD_OUT = np.array(_perm([0, 5, 10, 15], [1, 2, 3, 7]), np.uint8)
LISTS = {"all": [0, 1, 2, 3, 4, 5], "three": [3, 0, 5], "one": [4]}


def random_net_cpu(gen, scale=1.0):
    """one advantage net's six tensors on the host, drawn from `gen` (tests/test_sdcfr_policy_ref.py rebuilds the World's nets with it)"""
    import torch
    shapes = [(128, 34), (128,), (64, 128), (64,), (16, 64), (16,)]
    fan = [34, 34, 128, 128, 64, 64]
    net = [scale * torch.randn(s, generator=gen) / np.sqrt(f) for s, f in zip(shapes, fan)]
    net[5] = net[5] - 0.15
    return net


class World:
    """The six-deal chance game on a context of its own stream, one context per deal (and the held-out deal) under the same seed, and both players'
    packed nets: random but fixed weights, scaled so that advantages of both signs occur."""

    def __init__(self, sl):
        import torch
        self.sl, self.torch = sl, torch
        self.stream = torch.cuda.Stream(device=0)
        self.ctx = sl.Context(0, stream=self.stream.cuda_stream)
        self.ctx.mccfr_seed(SEED)
        self.multi = sl.MultiDeal(self.ctx, 6)
        self.multi.set_perms(SIX)
        self.multi.build()
        self.game = sl.ChanceGame(self.multi)
        self.deal_ctx = []
        for perm in list(SIX) + [HELD_OUT]:
            c = sl.Context(0)
            c.mccfr_seed(SEED)
            c.set_deal(np.ascontiguousarray(perm))
            self.deal_ctx.append(c)
        gen = torch.Generator().manual_seed(NET_SEED)
        self.nets = [self.random_net(gen) for _ in range(2)]
        x = (torch.rand((256, 34), generator=gen) < 0.3).float().cuda()
        for w1, b1, w2, b2, w3, b3 in self.nets:
            adv = torch.relu(torch.relu(x @ w1.t() + b1) @ w2.t() + b2) @ w3.t() + b3
            assert bool((adv > 0).any()) and bool((adv < 0).any())   # both signs
        self.image = torch.zeros((2, sl.lib().scopa_sdcfr_image_floats()), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        for p, net in enumerate(self.nets):
            self.ctx.sdcfr_pack_weights(p, *(t.data_ptr() for t in net), self.image.data_ptr())
        self.ctx.synchronize()

    def random_net(self, gen, scale=1.0):
        return [t.cuda().contiguous() for t in random_net_cpu(gen, scale)]

    def seed(self, seed):
        """the Philox key of the chance game's context and of every per-deal context"""
        for c in [self.ctx] + self.deal_ctx:
            c.mccfr_seed(seed)

    def rings(self, capacity):
        torch = self.torch
        f = torch.full((capacity, 34), SENTINEL, dtype=torch.float32, device="cuda:0")
        r = torch.full((capacity, 16), SENTINEL, dtype=torch.float32, device="cuda:0")
        k = torch.full((capacity, 16), SENTINEL, dtype=torch.float32, device="cuda:0")
        return f, r, k

    def chance_call(self, traverser, batch, deals, capacity, write_base, with_mask, b0=B0, iteration=ITERATION):
        """-> (feat, regret, mask or None, root values) as numpy after one scopa_chance_sdcfr_traverse into sentinel-filled rings"""
        torch = self.torch
        m = 6 if deals is None else len(deals)
        f, r, k = self.rings(capacity)
        v = torch.full((m * batch,), SENTINEL, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        self.game.sdcfr_traverse(traverser, batch, self.image.data_ptr(), f.data_ptr(), r.data_ptr(), k.data_ptr() if with_mask else 0, capacity, write_base,
                                 v.data_ptr(), iteration, b0, deals)
        self.ctx.synchronize()
        return f.cpu().numpy(), r.cpu().numpy(), k.cpu().numpy() if with_mask else None, v.cpu().numpy()

    def single_calls(self, traverser, batch, deals, capacity, write_base, with_mask, b0=B0, iteration=ITERATION):
        """the same rings from m scopa_sdcfr_traverse_fused calls on the per-deal contexts: deal d in slot s with b0 + d * batch and the slot's write_base"""
        torch = self.torch
        f, r, k = self.rings(capacity)
        v = torch.full((len(deals) * batch,), SENTINEL, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        for s, d in enumerate(deals):
            c = self.deal_ctx[d]
            c.sdcfr_traverse_fused(traverser, batch, self.image.data_ptr(), f.data_ptr(), r.data_ptr(), k.data_ptr() if with_mask else 0, capacity,
                                   (write_base + 41 * s * batch) % capacity, v.data_ptr() + 4 * s * batch, 0, iteration, b0 + d * batch)
            c.synchronize()
        return f.cpu().numpy(), r.cpu().numpy(), k.cpu().numpy() if with_mask else None, v.cpu().numpy()

    def close(self):
        for c in self.deal_ctx:
            c.close()
        self.ctx.close()


@pytest.fixture(scope="module")
def world(sl):
    try:
        w = World(sl)
    except sl.ScopaError as e:
        if e.status == sl.SCOPA_ENODEV:
            pytest.skip("no GPU on this box")
        raise
    assert (w.game.n, w.game.G, w.game.n_occurrences) == (6, 3522, 3860)
    yield w
    w.close()


def _same(got, exp):
    for a, b in zip(got, exp):
        if a is None or b is None:
            assert a is None and b is None
        elif not np.array_equal(a, b):
            return False
    return True


# ---- 1. rows equal the single-deal path ------------------------------------------------------------------------------------------------------
def _rows_equal_single_deal_calls(world, name, traverser, batch, **words):
    deals = LISTS[name]
    capacity, write_base = 41 * len(deals) * batch + 50, 17
    for with_mask in (False, True):
        got = world.chance_call(traverser, batch, None if name == "all" else deals, capacity, write_base, with_mask, **words)
        exp = world.single_calls(traverser, batch, deals, capacity, write_base, with_mask, **words)
        assert (exp[0][write_base:write_base + 41 * len(deals) * batch] != SENTINEL).all() and (exp[3] != SENTINEL).all()
        assert _same(got, exp)
        assert (got[0][:write_base] == SENTINEL).all() and (got[1][write_base + 41 * len(deals) * batch:] == SENTINEL).all()
    if name == "all":   # the explicit list of all deals is the NULL list
        assert _same(world.chance_call(traverser, batch, deals, capacity, write_base, True, **words), exp)


@pytest.mark.parametrize("batch", [5, 13])
@pytest.mark.parametrize("traverser", [0, 1])
@pytest.mark.parametrize("name", ["all", "three", "one"])
def test_rows_equal_single_deal_calls(world, name, traverser, batch):
    """neither batch is a multiple of the twelve wavefronts of a workgroup: ragged workgroups, and at 13 a deal spans more than one workgroup"""
    _rows_equal_single_deal_calls(world, name, traverser, batch)


@pytest.mark.parametrize("traverser", [0, 1])
def test_rows_equal_single_deal_calls_under_a_wide_seed(world, traverser):
    """the same with a high key word and a bit-31 iteration, every context under the same wide seed: the single-deal calls are held to the oracle at
    such words by tests/test_gpu_sdcfr.py, and tests/test_sdcfr_policy_ref.py asserts that these rows are not the ones a narrowed word gives"""
    seed, iteration, b0, deals = W.CH_WIDE
    assert deals == LISTS["three"]
    world.seed(seed)
    try:
        _rows_equal_single_deal_calls(world, "three", traverser, W.CH_BATCH, b0=b0, iteration=iteration)
    finally:
        world.seed(SEED)


def test_visits_are_counted_on_the_host(world):
    v0 = world.game.sdcfr_visits()
    world.chance_call(0, 5, [3, 0, 5], 41 * 15, 0, False)
    world.chance_call(1, 13, None, 41 * 6 * 13, 0, False)
    assert world.game.sdcfr_visits() - v0 == 105 * 3 * 5 + 82 * 6 * 13


# ---- 2. ring wrap inside a launch ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("traverser", [0, 1])
def test_ring_wrap_inside_a_launch(world, traverser):
    deals, batch = [3, 0, 5], 5
    rows = 41 * len(deals) * batch
    capacity = rows + 7
    write_base = capacity - (41 * batch + 100)          # the ring wraps 100 rows into slot 1: in the middle of traversal 2 of deal 0
    assert (capacity - write_base - 41 * batch) % 41 != 0
    got = world.chance_call(traverser, batch, deals, capacity, write_base, True)
    exp = world.single_calls(traverser, batch, deals, capacity, write_base, True)
    assert _same(got, exp)
    untouched = (got[1] == SENTINEL).all(1)
    assert untouched.sum() == 7 and untouched[(write_base + rows) % capacity:write_base].all()
    assert (got[0][untouched] == SENTINEL).all() and (got[2][untouched] == SENTINEL).all()


# ---- 3. list order and m change no draw ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("traverser", [0, 1])
def test_list_order_and_m_change_no_draw(world, traverser):
    batch, n = 13, 41 * 13
    out = {}
    for name, deals in LISTS.items():
        deals = [3] if name == "one" else deals
        s = deals.index(3)
        f, r, k, v = world.chance_call(traverser, batch, deals, 41 * len(deals) * batch, 0, True)
        out[name] = (f[s * n:(s + 1) * n], r[s * n:(s + 1) * n], k[s * n:(s + 1) * n], v[s * batch:(s + 1) * batch])
    assert _same(out["three"], out["all"]) and _same(out["three"], out["one"])
    other = world.chance_call(traverser, batch, [2], n, 0, True)
    assert not np.array_equal(other[1], out["one"][1])      # another deal does not give these rows


# ---- 4. average policy over keys -------------------------------------------------------------------------------------------------------------
def _store(world, max_size=5):
    torch = world.torch
    gen = torch.Generator().manual_seed(99)
    nets = [world.random_net(gen, scale=1.0 + 0.2 * s) for s in range(max_size)]
    return [torch.stack([n[i] for n in nets]).contiguous() for i in range(6)]


def _average_tables(world, store, slots, coef, players=(0, 1)):
    """-> ([G][4] from the chance call, [per deal [I][4]] from scopa_sdcfr_average_policy on each of the six contexts); rows not written stay NaN"""
    torch = world.torch
    n = len(slots)
    d_slots = torch.tensor(slots if n else [0], dtype=torch.int32, device="cuda:0")
    d_coef = torch.tensor(coef if n else [0.0], dtype=torch.float32, device="cuda:0")
    ptrs = [t.data_ptr() for t in store] if n else [0] * 6
    out_G = torch.full((world.game.G, 4), float("nan"), dtype=torch.float64, device="cuda:0")
    locals_ = [torch.full((c.n_infosets, 4), float("nan"), dtype=torch.float64, device="cuda:0") for c in world.deal_ctx[:6]]
    torch.cuda.synchronize()
    for p in players:
        world.game.sdcfr_average_policy(p, n, ptrs, store[0].shape[0], d_slots.data_ptr() if n else 0, d_coef.data_ptr() if n else 0, out_G.data_ptr())
        for c, o in zip(world.deal_ctx[:6], locals_):
            c.sdcfr_average_policy(p, n, ptrs, store[0].shape[0], d_slots.data_ptr() if n else 0, d_coef.data_ptr() if n else 0, o.data_ptr())
            c.synchronize()
    world.ctx.synchronize()
    return out_G.cpu().numpy(), [o.cpu().numpy() for o in locals_]


@pytest.mark.parametrize("case", ["three", "none", "slot_out_of_range"])
def test_average_policy_over_keys(world, case):
    keys, mp = world.game.index()
    nl = ((keys >> np.uint64(1)) & np.uint64(7)).astype(np.int64)
    player = (keys & np.uint64(1)).astype(np.int64)
    store = _store(world)
    slots, coef = {"three": ([4, 0, 2], [0.5, 0.3, 0.2]), "none": ([], []), "slot_out_of_range": ([4, 7, 2], [0.5, 0.3, 0.2])}[case]
    one, _ = _average_tables(world, store, slots, coef, players=(0,))
    assert np.isnan(one[player == 1]).all() and not np.isnan(one[player == 0]).any()       # the other player's rows are left alone
    G, per_deal = _average_tables(world, store, slots, coef)
    assert not np.isnan(G).any()
    for d in range(6):
        I = world.deal_ctx[d].n_infosets
        assert (mp[d, :I] >= 0).all() and (mp[d, I:] == -1).all()
        assert np.array_equal(G[mp[d, :I]], per_deal[d])
    legal = np.arange(4)[None, :] < nl[:, None]
    assert (G[~legal] == 0.0).all() and np.abs(G.sum(1) - 1.0).max() <= 1e-15
    uniform = np.where(legal, 1.0 / nl[:, None], 0.0)
    if case == "three":
        assert not np.array_equal(G, uniform)
        again, _ = _average_tables(world, store, slots, coef)
        assert np.array_equal(again, G)                                                     # no atomics: the same bits from run to run
    else:
        assert np.array_equal(G, uniform)
    if case == "none":
        assert np.array_equal(world.game.exploitability(G), world.game.exploitability(uniform))


# ---- 5. one deal = DeepCFR -------------------------------------------------------------------------------------------------------------------
def test_one_deal_is_deepcfr(sl):
    import torch
    from scopa_amd.envs import load_game
    from scopa_amd.algorithms.deep_cfr import ChanceDeepCFR, DeepCFR
    torch.manual_seed(7)
    ref = DeepCFR(load_game("mini_scopa"), num_players=2, device="cuda:0", batch=8, seed=SEED)
    ref.train(iterations=2, advantage_epochs=2)
    stream = torch.cuda.Stream(device=0)
    ctx = sl.Context(0, stream=stream.cuda_stream)
    multi = sl.MultiDeal(ctx, 1)
    multi.set_perms(sl.deal_py_seed(42).reshape(1, 16))
    multi.build()
    torch.manual_seed(7)
    d = ChanceDeepCFR(sl.ChanceGame(multi), batch=8, seed=SEED)
    d.train(iterations=2, advantage_epochs=2)
    torch.cuda.synchronize()
    for p in range(2):
        a, b = d.advantage_nets[p], ref.advantage_nets[p]
        assert a.buffer.total == b.buffer.total == 2 * 41 * 8 and a.buffer.write_base == b.buffer.write_base and a.buffer.capacity == b.buffer.capacity
        assert torch.equal(a.buffer.feat, b.buffer.feat) and torch.equal(a.buffer.regret, b.buffer.regret)
        for x, y in zip(a.net.parameters(), b.net.parameters()):
            assert torch.equal(x, y)
        assert d.strategy_buffers[p].weights == ref.strategy_buffers[p].weights == [2]
        assert d.training_history["losses"][p] == ref.training_history["losses"][p]
    ctx.close()
    ref._engine.close()


# ---- 6. end to end on six deals --------------------------------------------------------------------------------------------------------------
def test_end_to_end_on_six_deals(world):
    import torch
    from scopa_amd.algorithms.chance import sample_deals
    from scopa_amd.algorithms.deep_cfr import ChanceDeepCFR
    torch.manual_seed(11)
    d = ChanceDeepCFR(world.game, batch=8, deals_per_iteration=3, seed=SEED)
    d.train(iterations=3, advantage_epochs=2, exploitability_freq=1)
    h = d.training_history
    assert all(len(h[k][p]) == 3 for k in ("losses", "values", "buffer_sizes") for p in range(2))
    assert h["buffer_sizes"][0] == [41 * 3 * 8 * (i + 1) for i in range(3)]
    assert [i for i, _ in h["exploitability"]] == [0, 1, 2]
    print("exploitability across the six deals after 1, 2, 3 iterations:", [e for _, e in h["exploitability"]])
    assert all(np.isfinite(e) and e >= 0.0 for _, e in h["exploitability"])
    assert [i for i, _ in d.deal_log] == [0, 1, 2] and np.array_equal(np.stack([x for _, x in d.deal_log]), sample_deals(6, 3, 0, 3, SEED))
    assert d.strategy_buffers[0].weights == [2, 3]
    G = d.policy_table()
    _, mp = world.game.index()
    c = world.deal_ctx[2]
    assert np.array_equal(d.policy_table_for(c), G[mp[2, :c.n_infosets]])
    held = d.policy_table_for(world.deal_ctx[6])
    assert held.shape == (world.deal_ctx[6].n_infosets, 4) and np.abs(held.sum(1) - 1.0).max() <= 1e-12
    world.ctx.mccfr_seed(SEED)


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_ring_alone(world):
    sl, torch = world.sl, world.torch
    L, batch = sl.lib(), 5
    capacity = 41 * 6 * batch
    f, r, k = world.rings(capacity)
    v = torch.full((6 * batch,), SENTINEL, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()

    def call(deals, capacity=capacity, regret_ptr=r.data_ptr(), b0=0):
        d = None if deals is None else np.ascontiguousarray(deals, np.int32)
        L.scopa_last_error(world.ctx._h)
        rc = L.scopa_chance_sdcfr_traverse(world.game._h, 0, batch, 0 if d is None else d.size, None if d is None else d.ctypes.data_as(C.c_void_p),
                                           C.c_void_p(world.image.data_ptr()), C.c_void_p(f.data_ptr()), C.c_void_p(regret_ptr), C.c_void_p(k.data_ptr()),
                                           capacity, 0, C.c_void_p(v.data_ptr()), ITERATION, b0)
        return rc, L.scopa_last_error(world.ctx._h).decode()

    cases = {"a duplicate id": call([1, 4, 1]), "an id equal to n": call([0, 6]), "a ring too small": call(None, capacity=capacity - 1),
             "a misaligned d_mem_regret": call(None, regret_ptr=r.data_ptr() + 4), "b0 overflow": call(None, b0=2 ** 32 - 6 * batch + 1)}
    for what, (rc, msg) in cases.items():
        assert rc == sl.SCOPA_EINVAL and msg.startswith("scopa_chance_sdcfr_traverse:"), (what, rc, msg)
    assert len({msg for _, msg in cases.values()}) == 4       # (the two list errors share one message)
    world.ctx.synchronize()
    for t in (f, r, k, v):
        assert bool((t == SENTINEL).all())
    _, _, last_b0, all_deals = W.CH_LAST
    assert batch == W.CH_BATCH and last_b0 == 2 ** 32 - 6 * batch
    assert call(None, b0=last_b0)[0] == sl.SCOPA_OK                 # the last id is 2^32 - 1: accepted
    world.ctx.synchronize()
    assert bool((r != SENTINEL).all())
    # ... and drawn: deal d walks the ids b0 + d * batch + i up to 2^32 - 1, row for row the single-deal calls at b0 + d * batch
    exp = world.single_calls(0, batch, all_deals, capacity, 0, True, b0=last_b0)
    assert _same((f.cpu().numpy(), r.cpu().numpy(), k.cpu().numpy(), v.cpu().numpy()), exp)
