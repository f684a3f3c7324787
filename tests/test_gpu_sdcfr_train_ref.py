"""Every form of the Deep CFR optimiser step on the GPU against the float64 restatement of the reference's AdvantageNetwork.train
(oracle/sdcfr_train_ref.py): the eager autograd step, the graph-replayed lean step (graph_training's default), the graph-replayed autograd step and the
hand-written HIP step (train_backend="hip": k_sdcfr_train_grad + k_sdcfr_train_adam), all on the same memory contents.

Method: teacher forcing per train() call.  Before each call the net's weights and Adam state (optimizer.state, or the hand-written step's [2][13776]
moment buffer and step count) are read back; after it, the reference runs the same call from that snapshot on the host's own copy of the deque, and
loss, moments and weights are compared (tolerances and the one exclusion rule: oracle/sdcfr_train_ref.py).  Three calls per net, so Adam's state
carries over and a graph captured on call 0 is replayed on calls 1 and 2; epochs 1 and 3.

Memories: (K) rows written by DeepCFR._traverse_batch (mask = features[:16]); (E) K and add_experience rows with 0/1 masks of their own in a ring that
has wrapped; (F) E with fractional masks; (Z) a memory whose every mask is zero, after one call on E-style rows.  E starts from weights scaled by 3
(||g|| > 1: the clip coefficient is below 1), K and F from the net's own initialisation (||g|| < 1: the coefficient is clamped to 1)."""
import collections
import gc
import warnings

import numpy as np
import pytest

import sdcfr_train_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PATHS = ["eager", "graph_lean", "graph_autograd", "hip"]
_WORST = collections.defaultdict(lambda: collections.defaultdict(float))   # path -> the largest deviation measured, by quantity


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for path in PATHS:
        if path in _WORST:
            w = _WORST[path]
            print(f"\n[float64 reference] {path}: loss {w['loss_rel']:.3g} rel, exp_avg {w['exp_avg']:.3g}, exp_avg_sq {w['exp_avg_sq']:.3g}, "
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
        """Into `mem` IN PLACE (a captured graph keeps pointing at its tensors)."""
        assert mem.capacity == self.cap
        mem.feat.copy_(self.feat)
        mem.regret.copy_(self.regret)
        mem.total = self.total
        if self.side is not None:
            if mem._explicit is None:
                mem.put(slice(0, 0), mem.feat[:0], mem.regret[:0], mem.feat[:0, :16])      # allocates the side arrays
            mem._side_mask.copy_(self.side[0])
            mem._explicit.copy_(self.side[1])
        elif mem._explicit is not None:
            mem._explicit.zero_()


def _traverse(d, host, batch):
    """One traversal call of `batch` traversals into player 0's memory; the rows it wrote go to the host deque with mask = features[:16]."""
    mem = d.advantage_nets[0].buffer
    base = mem.write_base
    d._traverse_batch(0, batch)
    d._iteration += 1
    rows = (base + np.arange(41 * batch)) % mem.capacity
    f, r = mem.feat.cpu().numpy()[rows], mem.regret.cpu().numpy()[rows]
    host.extend(zip(f, r, f[:, :16].copy()))


def _add(a, host, rng, n, masks):
    for i in range(n):
        x = (rng.random(34) > 0.6).astype(np.float32)
        adv = (rng.standard_normal(16) * 3).astype(np.float32)
        m = masks(rng)
        a.add_experience(x, adv, m)
        host.append((x, R.normalise_advantages(adv), m))


def _binary(rng):
    return (rng.random(16) > 0.5).astype(np.float32)


def _fractional(rng):
    if rng.random() < 0.1:
        return np.zeros(16, np.float32)                                  # a row whose every mask entry is zero
    return np.where(rng.random(16) < 0.3, 0, rng.random(16) * 0.9).astype(np.float32)


@pytest.fixture(scope="module")
def world(sl):
    """Two solvers (their library contexts, streams and traversal kernels) and the memory setups."""
    import torch
    from scopa_amd.envs import load_game
    from scopa_amd.algorithms.deep_cfr import DeepCFR
    torch.manual_seed(21)
    big = DeepCFR(load_game("mini_scopa"), num_players=2, device=DEV, batch=128)
    small = DeepCFR(load_game("mini_scopa"), num_players=2, device=DEV, batch=16, memory_size=1500)
    init = {k: v.detach().clone() for k, v in small.advantage_nets[0].net.state_dict().items()}
    snaps = {}
    with torch.cuda.stream(big._stream):
        host = collections.deque(maxlen=big.advantage_nets[0].buffer.capacity)
        _traverse(big, host, 128)                                         # 5 248 kernel rows
        snaps["K"] = Snap(big.advantage_nets[0].buffer, host)
        mem = big.advantage_nets[0].buffer
        total = mem.total
        mem.total = 20                                                    # 20 rows in memory: the reference's min(n, 32) batch
        snaps["K20"] = Snap(mem, list(host)[:20])
        mem.total = total
    with torch.cuda.stream(small._stream):
        rng = np.random.default_rng(23)
        a = small.advantage_nets[0]
        base = {k: v.clone() for k, v in (("feat", a.buffer.feat), ("regret", a.buffer.regret))}
        for name, masks in (("E", _binary), ("F", _fractional)):
            a.buffer.feat.copy_(base["feat"]); a.buffer.regret.copy_(base["regret"])
            a.buffer.total, a.buffer._explicit, a.buffer._side_mask = 0, None, None
            small._iteration = 0
            host = collections.deque(maxlen=1500)
            _traverse(small, host, 16)                                    # 656 kernel rows
            if name == "E":
                snaps["K656"] = Snap(a.buffer, host)                      # (the capture-order case trains on these first)
            _add(a, host, rng, 300, masks)                                # rows with masks of their own
            _traverse(small, host, 16)                                    # the ring wraps: 1 612 rows written into 1 500
            _add(a, host, rng, 100, masks)                                # ... and these overwrite the oldest kernel rows
            assert a.buffer.total == 1712 and len(a.buffer) == 1500 and bool(a.buffer._explicit.any())
            snaps[name] = Snap(a.buffer, host)
        from scopa_amd.algorithms.deep_cfr.deep_cfr import AdvantageNetwork
        z = AdvantageNetwork(34, 16, device=DEV, memory_size=600)
        for name, masks in (("Z0", _binary), ("Z", lambda r: np.zeros(16, np.float32))):
            host = collections.deque(maxlen=600)
            _add(z, host, rng, 600, masks)
            snaps[name] = Snap(z.buffer, host)
    small._stream.synchronize()
    big._stream.synchronize()
    return {"big": big, "small": small, "init": init, "snaps": snaps}


def _net(world, solver, path, snap, scale=1.0):
    import torch
    from scopa_amd.algorithms.deep_cfr.deep_cfr import AdvantageNetwork
    a = AdvantageNetwork(34, 16, device=DEV, memory_size=snap.cap, use_graph=path.startswith("graph"), train_backend="hip" if path == "hip" else "torch")
    if path == "graph_autograd":
        a.lean_step = False
    a._ctx, a._ctx_stream = solver._engine.ctx, solver._stream
    a.net.load_state_dict({k: v * scale if v.dim() == 2 else v for k, v in world["init"].items()})
    snap.load(a.buffer)
    torch.cuda.current_stream().synchronize()
    return a


def _state(a, k):
    """(parameters, exp_avg, exp_avg_sq, step) as float64 arrays: the hand-written step's own state when it takes a k-row batch, else optimizer.state."""
    ps = list(a.net.parameters())
    w = [p.detach().double().cpu().numpy() for p in ps]
    if a.train_backend == "hip" and k % 16 == 0:
        if a._hip is None:
            return w, [np.zeros(p.shape) for p in ps], [np.zeros(p.shape) for p in ps], 0
        mo = a._hip[0].double().cpu().numpy().reshape(2, R.N_PARAMS)
        return w, R.split_flat(mo[0]), R.split_flat(mo[1]), a._hip_step
    st = [a.optimizer.state.get(p, {}) for p in ps]
    if "exp_avg" not in st[0]:
        return w, [np.zeros(p.shape) for p in ps], [np.zeros(p.shape) for p in ps], 0
    return (w, [s["exp_avg"].double().cpu().numpy() for s in st], [s["exp_avg_sq"].double().cpu().numpy() for s in st],
            int(st[0]["step"].item()) if hasattr(st[0]["step"], "item") else int(st[0]["step"]))


def _call(a, snap, batch, epochs, what):
    """One train() call checked against the reference run from the net's own state; returns the reference's per-step (loss, norm, coef, grad)."""
    import torch
    n = len(a.buffer)
    k = R.index_batches(n, batch, 1)[1]
    before = _state(a, k)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        loss = a.train(batch_size=batch, epochs=epochs)
    torch.cuda.current_stream().synchronize()
    if a.train_backend == "hip" and k % 16 and before[3] == 0:          # the first ragged call of the hip backend says that it takes the PyTorch path
        assert any(issubclass(c.category, RuntimeWarning) and "separate" in str(c.message) for c in caught), what
    after = _state(a, k)
    s = R.AdamState(*before)
    info = []
    ref_loss = R.train(s, *snap.host, batch_size=batch, epochs=epochs, info=info)
    assert after[3] == s.step, (what, after[3], s.step)
    dev = R.assert_call_matches(before[0], s, ref_loss, info, loss, after[0], after[1], after[2], what=what)
    path = what.split()[0]
    w = _WORST[path]
    w["loss_rel"] = max(w["loss_rel"], dev["loss"] / max(abs(ref_loss), 1e-30))
    for q in ("exp_avg", "exp_avg_sq", "weight", "weight_kept", "scale"):
        w[q] = max(w[q], dev[q])
    w["excluded"] += dev["excluded"]
    return info


def _run(world, solver, path, snap, batch, scale=1.0, pre=None):
    import torch
    infos = []
    with torch.cuda.stream(solver._stream):
        for epochs in (1, 3):
            a = _net(world, solver, path, pre or snap, scale)
            if pre is not None:
                infos += _call(a, pre, batch, epochs, f"{path} pre-call epochs={epochs}")
                snap.load(a.buffer)
            for call in range(3):
                infos += _call(a, snap, batch, epochs, f"{path} call {call} batch={batch} epochs={epochs}")
            if path.startswith("graph"):                                     # one capture per (batch, epochs, explicit masks allocated)
                assert len(a._graphs) == (1 if pre is None else len({pre.side is None, snap.side is None}))
            if path == "hip" and batch % 16 == 0 and len(a.buffer) >= batch:
                assert a._hip_step == (3 + (pre is not None)) * epochs
            del a
            gc.collect()                                                         # this net's graphs go now, not whenever the cycle collector runs
    return [i[1] for i in infos]


@pytest.mark.parametrize("batch", [16, 48, 128, 528, 4096, "ragged"])
@pytest.mark.parametrize("path", PATHS)
def test_traversal_rows(world, path, batch):
    """(K): rows as the traversal kernel writes them; batches of 1, 3, 8, 33 (one workgroup of the HIP step takes two tiles) and 256 tiles, and the
    reference's min(n, 32) batch on a 20-row memory (the HIP backend takes the PyTorch path there and warns)."""
    if batch == "ragged":
        norms = _run(world, world["big"], path, world["snaps"]["K20"], 128)
    else:
        norms = _run(world, world["big"], path, world["snaps"]["K"], batch)
    assert max(norms) < 1.0                                                   # the clip coefficient is clamped to 1


@pytest.mark.parametrize("batch", [128, 528])
@pytest.mark.parametrize("setup", ["E", "F", "Z"])
@pytest.mark.parametrize("path", PATHS)
def test_add_experience_rows(world, path, setup, batch):
    """(E) 0/1 masks that are not the features, ||g|| > 1; (F) fractional masks, ||g|| < 1; (Z) every mask zero: no gradient, Adam decays its moments."""
    snaps = world["snaps"]
    if setup == "Z":
        norms = _run(world, world["small"], path, snaps["Z"], batch, pre=snaps["Z0"])
        assert all(n > 0 for n in norms[0:1] + norms[4:7]) and sum(n == 0.0 for n in norms) == 3 + 9   # pre-calls (E-style rows), then no gradient
    else:
        norms = _run(world, world["small"], path, snaps[setup], batch, scale=3.0 if setup == "E" else 1.0)
        assert (min(norms) > 1.0) if setup == "E" else (max(norms) < 1.0)


@pytest.mark.parametrize("path", ["graph_lean", "graph_autograd"])
def test_graph_captured_before_add_experience_rows(world, path):
    """A graph captured while the memory held traversal rows only, then rows with masks of their own (not features[:16]) enter the sampled
    batches: the next calls must use those masks (DeviceMemory.gather chooses its form in Python, at capture time)."""
    snaps = world["snaps"]
    _run(world, world["small"], path, snaps["E"], 128, pre=snaps["K656"])
