"""The hand-written optimiser step of FullScopa's 96-128-64-40 advantage net (scopa_amd/csrc/scopa_full_train.hip: scopa_full_sdcfr_train_steps,
FullChanceDeepCFR(train_backend="hip")) on the GPU against the float64 statement tests/full_train_ref.py.

Method, as tests/test_gpu_sdcfr_train_ref.py: teacher forcing per train() call.  Before each call the net's weights, the step's [2][23272] moment
buffer and its step count are read back; the reference runs the same call from that snapshot on the host's copy of the deque; loss, moments, weights
and step size are compared (bounds and the exclusion rule: oracle/sdcfr_train_ref.py; the cap of 8 exclusions is held as a condition on these
memories by tests/test_full_train_ref.py).  Three calls per net, epochs 1 and 3.

Solvers: FullChanceDeepCFR on 3 decks at R = 1 (4 rows a traversal) and at R = 2 (28 rows), 16 traversals a deck.  Memories: (K) kernel rows only;
(E) kernel rows and add_experience rows with 0/1 masks of their own and random values in feature columns 92..95, in a ring that has wrapped, weights
scaled by 3 (clip coefficient below 1); (F) E with fractional masks and all-zero rows; (Z) every mask zero after one call on 0/1-mask rows.
Batches: 16 (one tile), 48 (fewer tiles than partials), 16 x 257 (one workgroup takes two tiles), and 20 rows in memory (ragged: the PyTorch path)."""
import collections
import gc

import numpy as np
import pytest

import full_train_ref as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x5C09A
_WORST = collections.defaultdict(float)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if _WORST:
        w = _WORST
        print(f"\n[float64 reference] full hip step: loss {w['loss_rel']:.3g} rel, exp_avg {w['exp_avg']:.3g}, exp_avg_sq {w['exp_avg_sq']:.3g}, "
              f"weights {w['weight']:.3g} ({w['weight_kept']:.3g} without the {int(w['excluded'])} excluded), update size {w['scale']:.3g}")


class Snap:
    """A DeviceMemory's contents (device tensors) with the host's own copy of the deque in logical order."""

    def __init__(self, mem, host):
        self.cap, self.total = mem.capacity, mem.total
        self.feat, self.regret = mem.feat.clone(), mem.regret.clone()
        self.side = None if mem._explicit is None else (mem._side_mask.clone(), mem._explicit.clone())
        f, r, m = (np.stack(c) for c in zip(*host))
        assert len(f) == len(mem)
        self.host = (f, r, m)

    def load(self, mem):
        assert mem.capacity == self.cap
        mem.feat.copy_(self.feat)
        mem.regret.copy_(self.regret)
        mem.total = self.total
        mem._explicit = mem._side_mask = None
        if self.side is not None:
            mem._side_mask, mem._explicit = self.side[0].clone(), self.side[1].clone()


def _solver(sl, oracle, R, **kw):
    import torch
    import full_mccfr_ref as F
    from scopa_amd.algorithms import FullChanceMCCFRTrainer, packet_decks
    from scopa_amd.algorithms.deep_cfr import FullChanceDeepCFR
    r0 = 6 - R
    deck = oracle.full_deal_py_seed(42)
    _, acts = F.random_root(deck, r0, np.random.RandomState(100 * r0 + 42))
    decks = packet_decks(deck, r0, 3, 5, fix_seat=None if R == 1 else 0)
    stream = torch.cuda.Stream(device=0)
    c = sl.Context(0, stream=stream.cuda_stream)
    t = FullChanceMCCFRTrainer(decks=decks, root_actions=acts, capacity_log2=12, batch=1, ctx=c)
    d = FullChanceDeepCFR(t, batch=16, seed=SEED, train_backend="hip", **kw)
    d._keep = (t, c, stream, decks, acts)
    return d


def _traverse(d, host):
    """One traversal call (16 traversals in each deck) into player 0's memory; the rows it wrote go to the host deque with mask = features[:40]."""
    mem = d.advantage_nets[0].buffer
    base, n = mem.write_base, d.rows_per_traversal * d.n_decks * d.batch
    d._traverse_batch(0, d.batch)
    d._iteration += 1
    rows = (base + np.arange(n)) % mem.capacity
    f, r = mem.feat.cpu().numpy()[rows], mem.regret.cpu().numpy()[rows]
    assert not f[:, 92:].any()
    host.extend(zip(f, r, f[:, :40].copy()))


def _reset(mem):
    mem.feat.zero_()
    mem.regret.zero_()
    mem.total, mem._explicit, mem._side_mask = 0, None, None


@pytest.fixture(scope="module")
def world(sl, oracle):
    """Three solvers (R = 1; R = 2; R = 2 with a ring just above one iteration's rows) and the memory setups."""
    import torch
    from scopa_amd.algorithms.deep_cfr.full_chance_deep_cfr import FullAdvantageNetwork
    torch.manual_seed(21)
    r1, r2, r2e = _solver(sl, oracle, 1), _solver(sl, oracle, 2), _solver(sl, oracle, 2, memory_size=T.E_CAPACITY)
    assert r1.rows_per_traversal == 4 and r2.rows_per_traversal == 28 and all(type(a) is FullAdvantageNetwork for d in (r1, r2, r2e) for a in d.advantage_nets)
    init = {k: v.detach().clone() for k, v in r2.advantage_nets[0].net.state_dict().items()}
    snaps = {}
    with torch.cuda.stream(r1._stream):
        host = collections.deque(maxlen=r1.advantage_nets[0].buffer.capacity)
        _traverse(r1, host)
        assert len(host) == T.ROWS_R1
        snaps["K1"] = Snap(r1.advantage_nets[0].buffer, host)
    with torch.cuda.stream(r2._stream):
        mem = r2.advantage_nets[0].buffer
        host = collections.deque(maxlen=mem.capacity)
        for _ in range(T.K_CALLS):
            _traverse(r2, host)
        assert len(host) == T.K_CALLS * T.ROWS_R2 > max(T.BATCHES_K)
        snaps["K"] = Snap(mem, host)
        total, mem.total = mem.total, 20                                  # 20 rows in memory: the reference's min(n, 32) batch
        snaps["K20"] = Snap(mem, list(host)[:20])
        mem.total = total
    kf = snaps["K"].host[0]                                               # features of real key pairs, for the add_experience rows
    with torch.cuda.stream(r2e._stream):
        a = r2e.advantage_nets[0]
        for name, masks in (("E", T.binary_mask), ("F", T.fractional_mask)):
            rng = np.random.default_rng(T.SEEDS[name])
            _reset(a.buffer)
            r2e._iteration = 0
            host = collections.deque(maxlen=T.E_CAPACITY)

            def add(x, adv, m):
                a.add_experience(x, adv, m)
                host.append((x, T.normalise_advantages(adv), m))
            T.fill_experience_memory(rng, masks, kf, lambda: _traverse(r2e, host), add)
            assert a.buffer.total == 2 * T.ROWS_R2 + 400 > T.E_CAPACITY == len(a.buffer) and bool(a.buffer._explicit.any()) and not bool(a.buffer._explicit.all())
            snaps[name] = Snap(a.buffer, host)
        z = FullAdvantageNetwork(DEV, memory_size=T.Z_CAPACITY)
        rng = np.random.default_rng(T.SEEDS["Z"])
        for name, masks in (("Z0", T.binary_mask), ("Z", T.zero_mask)):
            host = collections.deque(maxlen=T.Z_CAPACITY)
            for _ in range(T.Z_CAPACITY):
                x, adv, m = T.experience_row(rng, masks, kf)
                z.add_experience(x, adv, m)
                host.append((x, T.normalise_advantages(adv), m))
            snaps[name] = Snap(z.buffer, host)
    for d in (r1, r2, r2e):
        d._stream.synchronize()
    yield {"r1": r1, "r2": r2, "r2e": r2e, "init": init, "snaps": snaps}
    for d in (r1, r2, r2e):
        d._keep[0].close()
        d._keep[1].close()


def _net(world, solver, snap, scale=1.0):
    import torch
    from scopa_amd.algorithms.deep_cfr.full_chance_deep_cfr import FullAdvantageNetwork
    a = FullAdvantageNetwork(DEV, memory_size=snap.cap)
    a._ctx, a._ctx_stream = solver.trainer.ctx, solver._stream
    a.net.load_state_dict({k: v * scale if v.dim() == 2 else v for k, v in world["init"].items()})
    snap.load(a.buffer)
    torch.cuda.current_stream().synchronize()
    return a


def _call(a, snap, batch, epochs, what):
    import torch
    ragged = T.index_batches(len(a.buffer), batch, 1)[1] % 16 != 0
    first = a._hip_step == 0 and not a._warned_torch_path
    info, dev, caught = T.checked_call(a, snap.host, batch, epochs, what, sync=lambda: torch.cuda.current_stream().synchronize())
    warned = [c for c in caught if issubclass(c.category, RuntimeWarning) and "separate" in str(c.message)]
    assert len(warned) == (1 if ragged and first else 0), what               # the ragged call takes the PyTorch path and says so, once
    for q in ("loss_rel", "exp_avg", "exp_avg_sq", "weight", "weight_kept", "scale"):
        _WORST[q] = max(_WORST[q], dev[q])
    _WORST["excluded"] += dev["excluded"]
    return info


def _run(world, solver, snap, batch, scale=1.0, pre=None):
    import torch
    infos = []
    with torch.cuda.stream(solver._stream):
        for epochs in (1, 3):
            a = _net(world, solver, pre or snap, scale)
            if pre is not None:
                infos += _call(a, pre, batch, epochs, f"pre-call epochs={epochs}")
                snap.load(a.buffer)
            for call in range(3):
                infos += _call(a, snap, batch, epochs, f"call {call} batch={batch} epochs={epochs}")
            whole = T.index_batches(len(a.buffer), batch, 1)[1] % 16 == 0
            assert a._hip_step == ((3 + (pre is not None)) * epochs if whole else 0)
            del a
            gc.collect()
    return [i[1] for i in infos]


@pytest.mark.parametrize("solver,setup,batch", [("r1", "K1", 16), ("r1", "K1", 48)] + [("r2", "K", b) for b in T.BATCHES_K] + [("r2", "K20", 128)])
def test_traversal_rows(world, solver, setup, batch):
    """(K): rows as the traversal kernel writes them, mask = features[:40] (no mask array is passed); 1, 3 and 257 tiles, and the reference's
    min(n, 32) batch on a 20-row memory (the PyTorch path, with its warning)."""
    norms = _run(world, world[solver], world["snaps"][setup], batch)
    assert all(np.isfinite(norms)) and min(norms) > 0


@pytest.mark.parametrize("batch", T.BATCHES_E)
@pytest.mark.parametrize("setup", ["E", "F", "Z"])
def test_add_experience_rows(world, setup, batch):
    """(E) 0/1 masks that are not the features, ||g|| > 1; (F) fractional masks and all-zero rows; (Z) every mask zero: no gradient, the coefficient
    clamps to 1 and the weights move by Adam's carried moments alone."""
    snaps = world["snaps"]
    if setup == "Z":
        norms = _run(world, world["r2e"], snaps["Z"], batch, pre=snaps["Z0"])
        assert all(n > 0 for n in norms[0:1] + norms[4:7]) and sum(n == 0.0 for n in norms) == 3 + 9
    else:
        norms = _run(world, world["r2e"], snaps[setup], batch, scale=3.0 if setup == "E" else 1.0)
        if setup == "E":
            assert min(norms) > 1.0                                          # the clip coefficient is below 1


def _bits(a):
    import torch
    torch.cuda.synchronize()
    return [p.detach().cpu().numpy().copy() for p in a.net.parameters()] + [a._hip[0].cpu().numpy().copy()]


@pytest.mark.parametrize("batch", [48, 16 * (T.P_CAP + 1)])
def test_same_snapshot_twice_gives_the_same_bits(world, batch):
    import torch
    outs = []
    for rep in range(2):
        with torch.cuda.stream(world["r2"]._stream):
            a = _net(world, world["r2"], world["snaps"]["K"], scale=3.0)
            losses = [a.train(batch_size=batch, epochs=3) for _ in range(2)]
        outs.append((np.array(losses, np.float64), _bits(a)))
    assert np.array_equal(outs[0][0].view(np.uint64), outs[1][0].view(np.uint64))
    for x, y in zip(outs[0][1], outs[1][1]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def test_called_from_another_stream(world):
    """net.train() from torch's default stream while the solver owns another: the launches go to the solver's stream, ordered behind the caller's queue
    and in front of its later reads -- the same bits as the call made on the solver's stream."""
    import torch
    outs = []
    for inside in (True, False):
        a = _net(world, world["r2"], world["snaps"]["K"])
        torch.cuda.synchronize()
        if inside:
            with torch.cuda.stream(world["r2"]._stream):
                loss = [a.train(batch_size=128, epochs=3) for _ in range(2)]
        else:
            assert torch.cuda.current_stream().cuda_stream != world["r2"]._stream.cuda_stream
            loss = [a.train(batch_size=128, epochs=3) for _ in range(2)]
            w_now = [p.detach().clone() for p in a.net.parameters()]        # read on the caller's stream, without a wait of the host's
            torch.cuda.current_stream().synchronize()
            assert all(torch.equal(x, p.detach()) for x, p in zip(w_now, a.net.parameters()))
        outs.append((loss, _bits(a)))
    assert outs[0][0] == outs[1][0]
    for x, y in zip(outs[0][1], outs[1][1]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


# ---- the C entry itself: bounds and refusals -------------------------------------------------------------------------------------------------------------
class Carved:
    """Tensors carved out of one float32 allocation whose every other word is NaN (a fixed payload), each piece on a 16-byte boundary plus `skew` words."""
    PAD = 64

    def __init__(self, shapes, skew=()):
        import torch
        self.off, pos = {}, self.PAD
        for name, shape in shapes.items():
            pos = (pos + 3) // 4 * 4 + (1 if name in skew else 0)
            self.off[name] = (pos, shape)
            pos += int(np.prod(shape)) + self.PAD
        self.buf = torch.full((pos,), float("nan"), dtype=torch.float32, device=DEV)
        self.guard = torch.ones(pos, dtype=torch.bool, device=DEV)
        for p, shape in self.off.values():
            self.guard[p:p + int(np.prod(shape))] = False
        self.nan_bits = self.buf.view(torch.int32)[0].item()

    def __getitem__(self, name):
        p, shape = self.off[name]
        return self.buf[p:p + int(np.prod(shape))].view(shape)

    def untouched(self):
        import torch
        return bool((self.buf.view(torch.int32)[self.guard] == self.nan_bits).all())


def _carved_problem(cap, seed, skew=()):
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    shapes = {"w1": (128, 96), "b1": (128,), "w2": (64, 128), "b2": (64,), "w3": (40, 64), "b3": (40,), "state": (2 * T.N_PARAMS,), "loss": (1,),
              "feat": (cap, 96), "regret": (cap, 40), "mask": (cap, 40)}
    c = Carved(shapes, skew)
    for name, (_, shape) in c.off.items():
        c[name].copy_(torch.randn(shape, generator=g) * (0.1 if name[0] in "wb" else 1.0))
    c["state"].zero_()
    c["loss"].zero_()
    c["mask"].copy_((torch.rand((cap, 40), generator=g) > 0.5).float())
    c["feat"][:, :40] = (torch.rand((cap, 40), generator=g) > 0.8).float().to(DEV)
    return c


def _step(ctx, c, rows, cap, use_mask=True, n_steps=None, first_step=1, lr=5e-4, n_rows=None, w2_shift=0, null=None):
    ptr = {k: c[k].data_ptr() for k in c.off}
    ptr["w2"] += w2_shift
    if null:
        ptr[null] = 0
    ctx.full_sdcfr_train_steps(rows.data_ptr() if null != "rows" else 0, rows.shape[1] if n_rows is None else n_rows, rows.shape[0] if n_steps is None else n_steps,
                               ptr["feat"], ptr["regret"], ptr["mask"] if use_mask else 0, cap, tuple(ptr[k] for k in ("w1", "b1", "w2", "b2", "w3", "b3")),
                               ptr["state"], first_step, lr, ptr["loss"])
    ctx.synchronize()


def _results(c):
    import torch
    return torch.cat([c[k].reshape(-1) for k in ("w1", "b1", "w2", "b2", "w3", "b3", "state", "loss")]).cpu().numpy()


@pytest.mark.parametrize("use_mask", [True, False])
def test_nothing_outside_the_tensors_is_read_or_written(sl, use_mask):
    """The six parameter tensors (W3 [40][64] and b3 [40] end at output 39), the moment buffer, the loss and the ring carved out of an allocation
    whose other words are NaN: after steps on index batches that name row capacity - 1, and on batches with the indices -1 and capacity (clamped to
    rows 0 and capacity - 1, never dereferenced), the surroundings hold their bits and no result is NaN -- an over-read of W3's rows 40..47 would be."""
    import torch
    cap = 70
    ctx = sl.Context(0)
    try:
        rng = np.random.default_rng(3)
        idx = rng.integers(0, cap, (2, 48))
        idx[:, 0], idx[:, 1], idx[1, 47] = cap - 1, 0, cap - 1
        wild = idx.copy()
        wild[:, 0], wild[:, 1], wild[1, 47] = cap, -1, cap + 5
        outs = []
        skew = ("b1", "b3", "state", "feat", "regret", "mask")               # (only W1, W2 and W3 need 16-byte alignment)
        for rows_h in (idx, wild):
            c = _carved_problem(cap, 11, skew)
            rc = torch.full((idx.size + 2 * Carved.PAD,), -(1 << 40), dtype=torch.int64, device=DEV)   # (a guard value that is no row either)
            rows = rc[Carved.PAD:Carved.PAD + idx.size].view(idx.shape)
            rows.copy_(torch.from_numpy(rows_h))
            torch.cuda.synchronize()
            _step(ctx, c, rows, cap, use_mask)
            assert c.untouched() and bool((rc[:Carved.PAD] == -(1 << 40)).all()) and bool((rc[-Carved.PAD:] == -(1 << 40)).all())
            assert torch.equal(rows.cpu(), torch.from_numpy(rows_h))
            out = _results(c)
            assert np.isfinite(out).all() and out[-1] > 0
            outs.append(out)
            fresh = _carved_problem(cap, 11, skew)
            for k in ("feat", "regret", "mask"):
                assert torch.equal(c[k], fresh[k])                            # the ring is read only
            assert not torch.equal(c["w3"], fresh["w3"]) and not torch.equal(c["b3"], fresh["b3"]) and bool((c["state"] != 0).any())
        assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))   # clamped indices name rows 0 and capacity - 1
    finally:
        ctx.close()


def test_refusals(sl):
    """Each violation of the contract is SCOPA_EINVAL with a message and no launch (nothing changes); n_steps = 0 succeeds and changes nothing."""
    import torch
    cap = 70
    ctx = sl.Context(0)
    try:
        c = _carved_problem(cap, 12)
        rows = torch.zeros((1, 48), dtype=torch.int64, device=DEV)
        before = _results(c)
        bad = [dict(n_rows=0), dict(n_rows=8), dict(n_rows=24), dict(n_rows=(1 << 20) + 16), dict(first_step=0), dict(lr=0.0), dict(n_steps=4097), dict(n_steps=-1),
               dict(w2_shift=4), dict(null="state"), dict(null="rows"), dict(null="b3")]
        for kw in bad:
            with pytest.raises(sl.ScopaError) as e:
                _step(ctx, c, rows, cap, **kw)
            assert e.value.status == sl.SCOPA_EINVAL, (kw, e.value)
            if "null" not in kw:
                assert "scopa_full_sdcfr_train_steps" in str(e.value), (kw, str(e.value))
        with pytest.raises(sl.ScopaError) as e:
            ctx.full_sdcfr_train_steps(rows.data_ptr(), 48, 1, c["feat"].data_ptr(), c["regret"].data_ptr(), 0, 0, tuple(c[k].data_ptr() for k in ("w1", "b1", "w2", "b2", "w3", "b3")),
                                       c["state"].data_ptr(), 1, 5e-4, c["loss"].data_ptr())
        assert e.value.status == sl.SCOPA_EINVAL                                # capacity 0
        _step(ctx, c, rows, cap, n_steps=0)
        assert np.array_equal(_results(c).view(np.uint32), before.view(np.uint32)) and c.untouched()
        _step(ctx, c, rows, cap)                                                # the context still works
        assert c.untouched() and np.isfinite(_results(c)).all() and not np.array_equal(_results(c), before)
    finally:
        ctx.close()


# ---- the solver ---------------------------------------------------------------------------------------------------------------------------------------------
def test_end_to_end_against_the_torch_backend(world):
    """FullChanceDeepCFR(decks, root_actions, batch=16, train_backend="hip").train(3, advantage_epochs=2) against a "torch" solver of the same seed:
    per-iteration losses as tests/test_gpu_sdcfr.py's hip-against-torch check (1e-5 relative to max(1, loss)), weights within 2e-5 after the run;
    then train_batch=48 is honoured."""
    import torch
    from scopa_amd.algorithms.deep_cfr import AdvantageNetwork, FullChanceDeepCFR
    from scopa_amd.algorithms.deep_cfr.full_chance_deep_cfr import FullAdvantageNetwork
    decks, acts = world["r1"]._keep[3], world["r1"]._keep[4]
    ds = {}
    for backend in ("torch", "hip"):
        torch.manual_seed(5)
        d = FullChanceDeepCFR(decks, root_actions=acts, batch=16, seed=SEED, train_backend=backend)
        assert all(type(a) is (FullAdvantageNetwork if backend == "hip" else AdvantageNetwork) for a in d.advantage_nets)
        d.train(3, advantage_epochs=2)
        d._stream.synchronize()
        ds[backend] = d
    try:
        lt, lh = (np.array(ds[b].training_history["losses"]) for b in ("torch", "hip"))
        assert lt.shape == lh.shape == (2, 3) and np.isfinite(lh).all() and (lh > 0).all()
        assert (np.abs(lt - lh) < 1e-5 * np.maximum(1.0, np.abs(lt))).all(), (lt, lh)
        for at, ah in zip(ds["torch"].advantage_nets, ds["hip"].advantage_nets):
            assert ah._hip_step == 6 and at._hip_step == 0 and not ah._warned_torch_path
            assert ah._sample_cache[1].shape == (2, 128)
            for x, y in zip(at.net.parameters(), ah.net.parameters()):
                np.testing.assert_allclose(y.detach().cpu().numpy(), x.detach().cpu().numpy(), atol=2e-5, rtol=0)
        d = ds["hip"]
        d.train(1, advantage_epochs=2, train_batch=48, resume=True)
        d._stream.synchronize()
        assert all(a._sample_cache[1].shape == (2, 48) and a._hip_step == 8 for a in d.advantage_nets)
        assert len(d.strategy_buffers[0]._slots) == 3 and d.exploitability()["exploitability"] >= 0
    finally:
        for d in ds.values():
            d.close()


def test_narrow_net_keeps_its_own_step(sl):
    """AdvantageNetwork(34, 16, train_backend="hip") still goes through scopa_sdcfr_train_steps (two launches, a [2][13776] buffer), not the wide entry."""
    import torch
    from scopa_amd.algorithms.deep_cfr import AdvantageNetwork
    stream = torch.cuda.Stream(device=0)
    ctx = sl.Context(0, stream=stream.cuda_stream)
    calls = []

    class Spy:
        def __getattr__(self, name):
            calls.append(name)
            return getattr(ctx, name)
    try:
        torch.manual_seed(2)
        a = AdvantageNetwork(34, 16, device=DEV, memory_size=64, train_backend="hip")
        a._ctx, a._ctx_stream = Spy(), torch.cuda.ExternalStream(ctx.stream, device=0)
        rng = np.random.default_rng(1)
        for _ in range(48):
            a.add_experience((rng.random(34) > 0.6).astype(np.float32), rng.standard_normal(16).astype(np.float32), (rng.random(16) > 0.5).astype(np.float32))
        before = [p.detach().clone() for p in a.net.parameters()]
        loss = a.train(batch_size=32, epochs=2)
        torch.cuda.synchronize()
        assert calls == ["sdcfr_train_steps"] and a._hip[0].numel() == 2 * 13776 and a._hip_step == 2 and np.isfinite(loss) and loss > 0
        assert all(not torch.equal(p.detach(), q) for p, q in zip(a.net.parameters(), before))
    finally:
        ctx.close()
