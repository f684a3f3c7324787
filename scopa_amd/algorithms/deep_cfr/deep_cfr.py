"""Single Deep CFR on MiniScopa with the reference's interface (mirrors src/algorithms/deep_cfr/deep_cfr.py).

What moved to the GPU: the external-sampling traversal (`batch` traversals per call: the deal's decision nodes evaluated once per
call on the matrix cores, the traversals as walks over that policy table -- or a forward pass per visit in one launch, or ply by
ply around a PyTorch forward), feature/mask encoding, regret normalisation and the advantage memory (a device-resident FIFO ring
the kernels write into directly), the strategy snapshots (slots of preallocated tensors) and evaluation vs random (all episodes in
lockstep on the device step kernel).  What stays PyTorch: the advantage MLP, Adam, the MSE loss -- on PyTorch-ROCm, graph-replayed
on request; `train_backend="hip"` swaps the optimiser step for two hand-written launches (opt-in).  `batch=1` is the reference's
shape (one traversal per player per iteration, 41 rows each).  DeepCFR.train keeps the host one iteration ahead of the device.
"""
import gc
import random

import numpy as np
import torch
import torch.nn as nn
import torch.optim as optim

from ...engine import Engine
from ... import _lib
from .nets import FlexibleNet, positive_regret_policy

HIDDEN = [128, 64]
ROWS_PER_TRAVERSAL = 41  # traverser-node visits of one traversal (1 + 4 + 12 + 24)


class DeviceMemory:
    """FIFO advantage memory (the reference's deque(maxlen=100000), deep_cfr.py:52) as device tensors: features [capacity][34] and normalised
    regrets [capacity][16].  MASKS are not stored for the rows the traversal kernels write: at a traverser node the legal actions are the cards
    of the mover's hand (openspiel_mini_scopa.py:36-45) and the first sixteen features are that hand's one-hot (deep_cfr.py:213-275), so such a
    row's mask IS `feat[row, :16]` -- `mask` hands out that strided view, the kernels skip the 64-byte mask stream (a row is 200 bytes of HBM, not
    264) and the training gather reads one array less.  `add_experience` takes a caller-supplied mask that need not equal the features: those
    rows keep a real mask in a side array chosen by a per-row flag (allocated on first use; a traversal overwriting such a row clears the flag).
    num_actions (default 16, MiniScopa's): the width of a regret row and of the mask view -- FullScopa's rows hold 40 regrets and their mask is
    features[0..40)."""

    def __init__(self, capacity, input_dim, device, num_actions=16):
        self.capacity = capacity
        self.num_actions = int(num_actions)
        self.feat = torch.zeros((capacity, input_dim), dtype=torch.float32, device=device)
        self.regret = torch.zeros((capacity, self.num_actions), dtype=torch.float32, device=device)
        self._side_mask = None   # [capacity][16]: masks of rows appended through append() / add_experience
        self._explicit = None    # [capacity] bool: the row's mask lives in _side_mask
        self.total = 0  # rows ever appended

    def __len__(self):
        return min(self.total, self.capacity)

    @property
    def row_bytes(self):
        """HBM bytes a traversal kernel writes per memory row: features and regrets (the mask is a view of the features)."""
        return 4 * (self.feat.shape[1] + self.num_actions)

    @property
    def mask(self):
        """[capacity][16] masks: a strided VIEW of the feature array while every row was written by a traversal kernel; with rows appended through
        append() in the ring, a tensor assembled from that view and the side array."""
        view = self.feat[:, :self.num_actions]
        if self._explicit is None:
            return view
        return torch.where(self._explicit.unsqueeze(1), self._side_mask, view)

    @property
    def mask_ptr(self):
        """What the library's training step takes as d_mask: 0 (mask = features[0..16), scopa_sdcfr.hip sd_mask_note) unless explicit masks exist."""
        if self._explicit is None:
            return 0, None
        m = self.mask.contiguous()
        return m.data_ptr(), m       # (the caller keeps `m` alive until its launches are queued on the same stream)

    def gather(self, rows):
        """(features, regrets, masks) of the ring rows `rows` -- the training batch (deep_cfr.py:88-97)."""
        x = self.feat[rows]
        m = x[..., :self.num_actions]
        if self._explicit is not None:
            m = torch.where(self._explicit[rows].unsqueeze(-1), self._side_mask[rows], m)
        return x, self.regret[rows], m

    @property
    def write_base(self):
        return self.total % self.capacity

    def advance(self, rows):
        """`rows` ring rows from write_base on have just been written by a traversal kernel (on the current stream)."""
        if self._explicit is not None and rows:
            b = self.write_base
            self._explicit[b:b + rows] = False
            if b + rows > self.capacity:
                self._explicit[:b + rows - self.capacity] = False
        self.total += rows

    def put(self, rows, feat, regret, mask):
        """Rows with masks of their own at ring positions `rows` (a slice or index tensor); `total` is the caller's to set."""
        if self._explicit is None:
            self._side_mask = torch.zeros((self.capacity, self.num_actions), dtype=torch.float32, device=self.feat.device)
            self._explicit = torch.zeros(self.capacity, dtype=torch.bool, device=self.feat.device)
        self.feat[rows], self.regret[rows], self._side_mask[rows] = feat, regret, mask
        self._explicit[rows] = True

    def append(self, feat, regret, mask):
        """One row at the deque's append position (the ring slot the traversal kernels would write next), with its own mask."""
        self.put(self.write_base, feat, regret, mask)
        self.total += 1

    def logical_to_physical(self, idx):
        """deque index (0 = oldest) -> ring row."""
        start = self.total % self.capacity if self.total > self.capacity else 0
        return (idx + start) % self.capacity

    def rows(self, idx):
        return self.gather(self.logical_to_physical(idx))

    def __getitem__(self, i):
        f, r, m = self.rows(torch.tensor([i % max(len(self), 1)], device=self.feat.device))
        return f[0].cpu().numpy(), r[0].cpu().numpy(), m[0].cpu().numpy()


_RAW = {}   # the first 32-bit outputs of random.Random() after seed(42) and one 16-element shuffle: the stream every train() call starts from


def reference_sample_stream(n, k, calls, rng=None):
    """`calls` successive `random.sample(range(n), k)` draws from the stream described in AdvantageNetwork.sample_indices, as an int64
    array [calls, k] -- the same indices CPython's `random` produces, computed with numpy (a 128-sample costs CPython 40 us, 4096 samples
    1.3 ms, ten times per iteration).  CPython 3.10 `sample`: with n above its set-size threshold, pick i = the next `_randbelow(n)` not
    picked before; `_randbelow(n)` = the next `getrandbits(n.bit_length())` below n; `getrandbits(b <= 32)` = one MT19937 output >> (32 - b).
    So a sample is the first k DISTINCT accepted values of the raw stream, in order.  Small n (the pool branch of `sample`) and streams
    longer than the cached prefix go through `rng` itself (which must then be in the state seed(42) + shuffle(16) leaves)."""
    import math
    setsize = 21 + (4 ** math.ceil(math.log(k * 3, 4)) if k > 5 else 0)
    if not 0 < k <= n:
        raise ValueError("Sample larger than population or is negative")
    def slow():
        r = rng
        if r is None:
            r = random.Random(); r.seed(42); r.shuffle(list(range(16)))
        return np.array([r.sample(range(n), k) for _ in range(calls)], dtype=np.int64)
    if n <= setsize or n.bit_length() > 32:
        return slow()
    if "raw" not in _RAW:
        r = random.Random(); r.seed(42); r.shuffle(list(range(16)))
        _RAW["raw"] = np.array([r.getrandbits(32) for _ in range(1 << 17)], dtype=np.uint64)
    raw, shift = _RAW["raw"], np.uint64(32 - n.bit_length())
    prefix = min(len(raw), max(1024, 4 * k * calls))        # acceptance is >= 1/2: 4 k calls raw values almost always suffice
    while True:
        vals = raw[:prefix] >> shift
        pos_ok = np.flatnonzero(vals < n)                   # stream positions whose value _randbelow accepts
        acc = vals[pos_ok].astype(np.int64)
        out, start, short = np.empty((calls, k), np.int64), 0, False   # start: index into the accepted values where the next call begins
        for c in range(calls):
            width = k + (3 * k * k) // (2 * n) + 64          # k picks meet ~k^2 / 2n repeats
            while True:
                seg = acc[start:start + width]
                _, first = np.unique(seg, return_index=True) # first occurrence of every distinct value within the segment
                if len(first) >= k:
                    break
                if start + width >= len(acc):
                    short = True
                    break
                width *= 2
            if short:
                break
            first.sort()
            take = first[:k]
            out[c] = seg[take]
            start += int(take[-1]) + 1                       # the next call goes on behind the k-th pick (rejected raw values in between are skipped either way)
        if not short:
            return out
        if prefix == len(raw):
            return slow()                                    # beyond the cached stream (huge k x calls): CPython does it
        prefix = min(len(raw), prefix * 4)


class AdvantageNetwork:
    """Advantage net + Adam + memory for one player (deep_cfr.py:24-116)."""

    def __init__(self, input_dim, num_actions, device="cuda", lr=5e-4, memory_size=100000, use_graph=False, train_backend="torch"):
        self.device = device
        # "torch" (default; north_star: the advantage MLP trains on PyTorch-ROCm) or "hip": the whole optimiser step in two hand-written launches
        # (scopa_sdcfr_train_step: forward, loss, backward on the matrix cores; clip + Adam), on the same tensors, opt-in
        if train_backend not in ("torch", "hip"):
            raise ValueError("train_backend must be 'torch' or 'hip'")
        if train_backend == "hip" and (int(input_dim), int(num_actions)) != (34, 16):
            raise ValueError("train_backend='hip' is the hand-written step of the 34-128-64-16 net only: a %d-128-64-%d net trains with train_backend='torch'"
                             % (int(input_dim), int(num_actions)))
        self.train_backend = train_backend
        self._ctx = None             # the solver's library context (set by DeepCFR): the hip backend launches on its stream
        self._ctx_stream = None      # ... and that stream as a torch stream: _train_hip orders itself against the caller's current stream through it
        self._warned_torch_path = False
        self._hip = None             # hip backend: (moment buffer [2][13776], running loss [1]) and the step count
        self._hip_step = 0
        self._sample_cache = None    # ((rows in memory, batch, epochs), device tensor of the index batches): see _sample_rows
        self._plist = None           # (net object, list of its parameters): walking the module tree costs 25 us a time
        self.use_graph = use_graph   # replay the optimiser step as one HIP graph (same ops, ~10x less launch overhead)
        self.lean_step = True        # graph mode: the step with its backward pass written out (_step_lean: 28 kernels instead of ~45); False = autograd's step in the graph
        self._graphs = {}            # (batch_size, epochs, explicit masks allocated) -> (graph of all the epochs' steps, static index tensor [epochs, batch], static loss tensor [epochs])
        self.num_actions = num_actions
        self.net = FlexibleNet(mode="mlp", input_shape=(input_dim,), output_dim=num_actions, mlp_hidden=HIDDEN,
                               mlp_act="relu", mlp_norm="none", mlp_dropout=0.0).to(device)
        for layer in self.net.modules():
            if isinstance(layer, nn.Linear):
                nn.init.xavier_uniform_(layer.weight)
                nn.init.constant_(layer.bias, 0.1)
        # graph mode: the single-kernel ("fused") Adam of PyTorch-ROCm -- the same update rule in one launch instead of ~15 foreach
        # kernels per step; eager mode keeps the reference's default implementation
        self.optimizer = (optim.Adam(self.net.parameters(), lr=lr, capturable=True, fused=True) if use_graph and str(device).startswith("cuda")
                          else optim.Adam(self.net.parameters(), lr=lr, capturable=bool(use_graph)))
        self.criterion = nn.MSELoss()
        self.buffer = DeviceMemory(memory_size, input_dim, device, num_actions=num_actions)
        self._rng = random.Random()
        self.grad_sync = None  # set by DeepCFR for N>1: callable(parameters) averaging the gradients over ranks
        # Counts the events that change the net's weights THROUGH THIS CLASS: every train() call (eager or graph-replayed -- a
        # replayed HIP graph updates the parameters without touching their autograd version counters) and every load_state_dict.
        # DeepCFR keys the traversal kernel's packed weight image on it.
        self.weights_epoch = 0
        self.net.register_load_state_dict_post_hook(lambda module, incompatible: self._weights_changed())

    def _weights_changed(self):
        self.weights_epoch += 1

    def param_list(self):
        """The net's parameters in net.parameters() order, looked up once per net object."""
        if self._plist is None or self._plist[0] is not self.net:
            self._plist = (self.net, list(self.net.parameters()))
        return self._plist[1]

    def get_advantages(self, state_features, legal_actions_mask):
        with torch.no_grad():
            x = torch.as_tensor(np.asarray(state_features), dtype=torch.float32, device=self.device)
            m = torch.as_tensor(np.asarray(legal_actions_mask), dtype=torch.float32, device=self.device)
            if x.dim() == 1:
                x, m = x.unsqueeze(0), m.unsqueeze(0)
            adv = self.net(x)
            return (adv * m - 1e6 * (1 - m)).cpu().numpy()

    def add_experience(self, state_features, advantages, legal_actions_mask):
        """deep_cfr.py:70-75 for callers that fill the memory themselves: the advantages are divided by max|adv| + 1e-8 when that
        maximum is positive (float32 arithmetic, as numpy does on the reference's float32 arrays) and the row is appended to the
        device-resident FIFO ring -- the same ring the traversal kernels write."""
        adv = torch.as_tensor(np.asarray(advantages), dtype=torch.float32, device=self.device).reshape(-1)
        peak = adv.abs().max()
        if float(peak) > 0:
            adv = adv / (peak + torch.tensor(1e-8, dtype=torch.float32, device=self.device))
        self.buffer.append(torch.as_tensor(np.asarray(state_features), dtype=torch.float32, device=self.device).reshape(-1), adv,
                           torch.as_tensor(np.asarray(legal_actions_mask), dtype=torch.float32, device=self.device).reshape(-1))

    def sample_indices(self, n, batch_size):
        """The reference's `random.sample(self.buffer, batch_size)` (:88).  There the global `random` stream was last
        seeded by a MiniDeck() built during the traversal (seed 42 + one 16-card shuffle, mini_scopa_game.py:25-28), so
        the sample is a deterministic function of the buffer length; the same stream is rebuilt here privately."""
        return self._rng.sample(range(n), batch_size)

    def train(self, batch_size=128, epochs=1, defer=False):
        """deep_cfr.py:77-116.  defer=True (the solver's own loop): the graph-replayed and the hand-written paths return the mean loss as a 0-dim DEVICE
        tensor instead of waiting for it -- the caller reads it after it has queued the rest of the iteration."""
        n = len(self.buffer)
        if n < batch_size:
            batch_size = min(n, 32)
            if batch_size == 0:
                return 0.0
        self._rng.seed(42)
        self._rng.shuffle(list(range(16)))
        self._weights_changed()
        if self.train_backend == "hip":
            if self.grad_sync is None and batch_size % 16 == 0 and batch_size >= 16:
                return self._train_hip(n, batch_size, epochs, defer)
            if not self._warned_torch_path:
                # the two paths keep SEPARATE Adam states (the hand-written step's moment buffer and step count / torch.optim.Adam's): a run that mixes them
                # continues each from where that path left off -- say so once instead of doing it silently
                import warnings
                warnings.warn("AdvantageNetwork(train_backend='hip'): this train() call takes the PyTorch optimiser (ragged batch of %d rows or gradient all-reduce); "
                              "its Adam state is separate from the hand-written step's" % batch_size, RuntimeWarning, stacklevel=2)
                self._warned_torch_path = True
        if self.use_graph and self.grad_sync is None:
            return self._train_graphed(n, batch_size, epochs, defer)
        rows_all = self._sample_rows(n, batch_size, epochs)
        total_loss = 0.0
        for e in range(epochs):
            total_loss += self._step(rows_all[e]).item()
        return total_loss / epochs

    def _train_hip(self, n, batch_size, epochs, defer=False):
        """The same steps through scopa_sdcfr_train_step (two launches per step, none of them PyTorch's): the net's own parameter tensors are
        updated in place, Adam's moments live in one [2][13776] buffer.  Ragged batches (not a multiple of 16 rows) and N > 1 take the PyTorch path."""
        if self._ctx is None:
            raise RuntimeError("train_backend='hip' needs the solver's library context (construct the net through DeepCFR)")
        params = self.param_list()
        if any(p.dtype != torch.float32 or not p.is_contiguous() for p in params):
            raise RuntimeError("train_backend='hip' needs contiguous float32 parameters")
        grp = self.optimizer.param_groups[0]   # the kernel implements torch.optim.Adam's defaults: anything else must not be dropped silently
        if tuple(grp.get("betas", (0.9, 0.999))) != (0.9, 0.999) or grp.get("eps", 1e-8) != 1e-8 or grp.get("weight_decay", 0) != 0 or grp.get("amsgrad", False) \
                or grp.get("maximize", False):
            raise RuntimeError("train_backend='hip' implements Adam(betas=(0.9, 0.999), eps=1e-8, weight_decay=0): other settings need train_backend='torch'")
        # Stream contract: the launches go to the solver's stream (the library context's).  Called from another current stream, order this call behind
        # what that stream has queued (the rows a traversal wrote, a zeroed loss) and the caller's later work behind this call's launches.
        cur = torch.cuda.current_stream(self.device) if self._ctx_stream is not None else None
        foreign = cur is not None and cur.cuda_stream != self._ctx_stream.cuda_stream
        if foreign:
            self._ctx_stream.wait_stream(cur)
            with torch.cuda.stream(self._ctx_stream):
                out = self._train_hip_on_stream(params, n, batch_size, epochs, defer)
            cur.wait_stream(self._ctx_stream)
            return out
        return self._train_hip_on_stream(params, n, batch_size, epochs, defer)

    def _train_hip_on_stream(self, params, n, batch_size, epochs, defer):
        if self._hip is None:
            self._hip = (torch.zeros(2 * sum(p.numel() for p in params), dtype=torch.float32, device=self.device),
                         torch.zeros(1, dtype=torch.float32, device=self.device))
        state, loss = self._hip
        rows_all = self._sample_rows(n, batch_size, epochs).contiguous()
        loss.zero_()
        lr = float(self.optimizer.param_groups[0]["lr"])
        ptrs = tuple(p.data_ptr() for p in params)
        mask_ptr, _keep = self.buffer.mask_ptr
        self._ctx.sdcfr_train_steps(rows_all.data_ptr(), batch_size, epochs, self.buffer.feat.data_ptr(), self.buffer.regret.data_ptr(), mask_ptr,
                                    self.buffer.capacity, ptrs, state.data_ptr(), self._hip_step + 1, lr, loss.data_ptr())
        self._hip_step += epochs
        return loss[0] / epochs if defer else float(loss.item()) / epochs

    def _sample_rows(self, n, batch_size, epochs):
        """All `epochs` index batches of one train() call in ONE upload ([epochs, batch] ring rows): the reference draws them one after
        the other from the same `random` stream (:88), so drawing them up front gives the same batches; a per-step list -> device copy
        made the optimiser step host-bound."""
        # Every train() call re-seeds the stream (seed 42 + one shuffle, as the reference's MiniDeck() does), so the index batches are a pure
        # function of (rows in memory, batch, epochs): once the ring is full they are the SAME deque positions call after call (the reference's
        # own artefact) and the device copy of the last draw is reused -- only the ring's start moves (logical_to_physical).
        key = (n, batch_size, epochs)
        if self._sample_cache is None or self._sample_cache[0] != key:
            self._sample_cache = (key, torch.from_numpy(reference_sample_stream(n, batch_size, epochs, self._rng)).to(self.device))
        return self.buffer.logical_to_physical(self._sample_cache[1])

    def _step(self, rows):
        """One optimiser step on the ring rows `rows` (deep_cfr.py:99-112); returns the loss tensor."""
        states, target_adv, masks = self.buffer.gather(rows)
        self.optimizer.zero_grad(set_to_none=True)   # fresh gradient tensors each step: no zero-fill and no accumulate-add kernels (9 of ~45 per step)
        pred_adv = self.net(states)
        loss = self.criterion(pred_adv * masks, target_adv * masks)
        loss.backward()
        if self.grad_sync is not None:
            self.grad_sync(self.net.parameters())
        torch.nn.utils.clip_grad_norm_(self.net.parameters(), max_norm=1.0)
        self.optimizer.step()
        return loss

    def _lean_setup(self):
        """Gradients of the six parameter tensors as views of ONE flat buffer (so the clip's norm and its scaling are one kernel each)."""
        params = list(self.net.parameters())
        flat = torch.zeros(sum(p.numel() for p in params), dtype=torch.float32, device=self.device)
        off = 0
        for p in params:
            p.grad = flat[off:off + p.numel()].view_as(p)
            off += p.numel()
        self._lean = (flat, params, torch.zeros((), dtype=torch.float32, device=self.device))

    def _step_lean(self, rows):
        """The same optimiser step (deep_cfr.py:99-112) with the backward pass of the 34-128-64-16 MLP written out in PyTorch ops instead
        of recorded by autograd -- graph mode only.  An Adam step on a 128-row batch is launch-bound (every kernel of it costs the 4-5 us
        of a dependent launch whatever it does), so what counts is the NUMBER of kernels: autograd's step is ~45 (accumulate / fill /
        per-tensor norm / foreach kernels included), this one 28.  Same arithmetic: MSE over all 16 outputs of pred * mask - target * mask
        (written (pred - target) * mask: the same numbers for 0 / 1 masks), its gradient 2 (pred - target) mask^2 / N, relu backward by aten's threshold_backward, clip_grad_norm_'s
        min(1, 1 / (norm + 1e-6)) on the 2-norm of all gradients, the optimizer's own (fused) Adam."""
        if getattr(self, "_lean", None) is None or self._lean[1][0].grad is None or self._lean[1][0].grad.data_ptr() != self._lean[0].data_ptr():
            self._lean_setup()                                               # (first use, or autograd's step has replaced the .grad tensors since)
        flat, (w1, b1, w2, b2, w3, b3), zero = self._lean
        with torch.no_grad():
            x, t, m = self.buffer.gather(rows)
            h1 = torch._addmm_activation(b1, x, w1.t())                   # relu(x W1^T + b1), one kernel
            h2 = torch._addmm_activation(b2, h1, w2.t())
            y = torch.addmm(b3, h2, w3.t())
            e = (y - t) * m
            loss = (e * e).mean()
            d = torch.addcmul(zero, e, m, value=2.0 / e.numel())            # dL/dy = 2 (y - t) m m / N: a fractional mask enters twice (one kernel)
            torch.mm(d.t(), h2, out=w3.grad)
            torch.sum(d, 0, out=b3.grad)
            dz2 = torch.ops.aten.threshold_backward(torch.mm(d, w3), h2, 0)
            torch.mm(dz2.t(), h1, out=w2.grad)
            torch.sum(dz2, 0, out=b2.grad)
            dz1 = torch.ops.aten.threshold_backward(torch.mm(dz2, w2), h1, 0)
            torch.mm(dz1.t(), x, out=w1.grad)
            torch.sum(dz1, 0, out=b1.grad)
            flat.mul_(torch.clamp(torch.reciprocal(torch.linalg.vector_norm(flat) + 1e-6), max=1.0))   # clip_grad_norm_(max_norm=1.0)
        self.optimizer.step()
        return loss

    def _train_graphed(self, n, batch_size, epochs, defer=False):
        """The same steps -- all `epochs` of a train() call -- captured once per (batch size, epochs) into ONE HIP graph and replayed with
        fresh row indices: one upload of the [epochs, batch] index batches, one replay, one read-back of the mean loss.  DeviceMemory.gather
        decides in Python whether a batch's masks come from the features alone or also from the side array of add_experience rows, so the
        graph is keyed on that too: the first put() after a capture leads to one new capture, and traversal-only memories keep the lean gather."""
        key = (batch_size, epochs, self.buffer._explicit is not None)
        if key not in self._graphs:
            rows = torch.zeros((epochs, batch_size), dtype=torch.long, device=self.device)
            losses = torch.zeros(epochs, dtype=torch.float32, device=self.device)
            side = torch.cuda.Stream(device=self.device)
            side.wait_stream(torch.cuda.current_stream())
            # warm-up runs real optimiser steps: snapshot parameters and Adam state BY VALUE first and restore them IN PLACE afterwards
            # (the graph keeps pointing at these very tensors), so capturing changes nothing
            params = list(self.net.parameters())
            saved_p = [p.detach().clone() for p in params]
            saved_s = {i: {k: v.clone() for k, v in self.optimizer.state[p].items() if torch.is_tensor(v)}
                       for i, p in enumerate(params) if p in self.optimizer.state}
            step = self._step_lean if self.lean_step else self._step
            with torch.cuda.stream(side):
                for _ in range(3):
                    step(rows[0])
            torch.cuda.current_stream().wait_stream(side)
            g = torch.cuda.CUDAGraph()
            # no garbage collection while capturing: an AdvantageNetwork is a reference cycle (its load_state_dict hook), so a dead one's graphs are
            # freed by the cycle collector, and a graph destroyed while a stream captures aborts the process (hipErrorStreamCaptureUnsupported)
            gc.collect()
            was_enabled = gc.isenabled()
            gc.disable()
            try:
                with torch.cuda.graph(g):
                    for e in range(epochs):
                        losses[e].copy_(step(rows[e]))
            finally:
                if was_enabled:
                    gc.enable()
            with torch.no_grad():
                for i, p in enumerate(params):
                    p.copy_(saved_p[i])
                    for k, v in self.optimizer.state[p].items():
                        if torch.is_tensor(v):
                            if i in saved_s and k in saved_s[i]:
                                v.copy_(saved_s[i][k])
                            else:
                                v.zero_()   # a fresh optimiser: moments and step count start at zero
            self._graphs[key] = (g, rows, losses)
        g, rows, losses = self._graphs[key]
        rows.copy_(self._sample_rows(n, batch_size, epochs))
        g.replay()
        return losses.sum() / epochs if defer else float(losses.sum().item()) / epochs


class _SnapshotView:
    """One stored snapshot of a StrategyBuffer: views of its six parameter tensors; callable like the net it was copied from."""

    def __init__(self, tensors):
        self._t = tensors

    def parameters(self):
        return iter(self._t)

    def __call__(self, x):
        w1, b1, w2, b2, w3, b3 = self._t
        return torch.addmm(b3, torch.relu(torch.addmm(b2, torch.relu(torch.addmm(b1, x, w1.t())), w2.t())), w3.t())


class StrategyBuffer:
    """<= max_size net snapshots, weight = iteration + 1 (deep_cfr.py:119-160).  The reference keeps a list of deep-copied modules; here a snapshot is
    one slot of six preallocated tensors [max_size][...] on the nets' device: adding one is a single multi-tensor copy (building a module per
    iteration and player was 3 ms of a 4.6 ms iteration), and the average policy of a small batch is three batched matrix products over ALL
    snapshots instead of a forward pass per snapshot (500 launches per ply of an evaluation)."""

    def __init__(self, max_size=100):
        self.weights, self.max_size = [], max_size
        self._slots, self._free, self._store = [], list(range(max_size)), None
        self._gathered = None        # (the stored snapshots' tensors in FIFO order, their normalised weights): rebuilt after the next add_strategy
        self._device_args = None     # (slots int32, coefficients float32) on the device, for policy_table_device: rebuilt after the next add_strategy

    @property
    def strategies(self):
        return [_SnapshotView([t[k] for t in self._store]) for k in self._slots]

    def add_strategy(self, strategy_net, iteration, params=None):
        """Stores a COPY of strategy_net's parameters (the reference's callers pass a deep copy they made; the copy made here makes that unnecessary).
        params: the net's parameter list, if the caller has it at hand."""
        params = [p.detach() for p in (strategy_net.parameters() if params is None else params)]
        with torch.no_grad():
            if self._store is None:
                self._store = [torch.empty((self.max_size,) + tuple(p.shape), dtype=p.dtype, device=p.device) for p in params]
            if len(self._slots) >= self.max_size:
                self._free.append(self._slots.pop(0))
                self.weights.pop(0)
            slot = self._free.pop(0)
            torch._foreach_copy_([t[slot] for t in self._store], params)
        self._slots.append(slot)
        self.weights.append(iteration + 1)
        self._gathered = None
        self._device_args = None

    def average_policy_batch(self, feats, masks):
        """[N,34],[N,16] device tensors -> [N,16] weighted average of the snapshots' regret-matching policies."""
        if not self._slots:
            return masks / masks.sum(dim=-1, keepdim=True)
        total = float(sum(self.weights))
        with torch.no_grad():
            if len(self._slots) * feats.shape[0] <= 65536:   # all snapshots at once: [S, N, 128] activations (S x N rows: 32 MB at the gate; 100 snapshots x 4096 rows were 0.5 GB per ply)
                if self._gathered is None:                   # once per buffer state (an evaluation asks eight times, a ply each)
                    idx = torch.tensor(self._slots, device=feats.device)
                    self._gathered = (tuple(t[idx] for t in self._store), torch.tensor(self.weights, dtype=torch.float32, device=feats.device) / total)
                (w1, b1, w2, b2, w3, b3), wk = self._gathered
                x = feats.unsqueeze(0).expand(len(self._slots), -1, -1)
                h = torch.relu(torch.baddbmm(b1.unsqueeze(1), x, w1.transpose(1, 2)))
                h = torch.relu(torch.baddbmm(b2.unsqueeze(1), h, w2.transpose(1, 2)))
                adv = torch.baddbmm(b3.unsqueeze(1), h, w3.transpose(1, 2))
                return (positive_regret_policy(adv, masks.unsqueeze(0)) * wk.view(-1, 1, 1)).sum(0)
            out = torch.zeros_like(masks)                    # large batches: a forward pass per snapshot (large kernels, no [S, N, 128] intermediate)
            for net, w in zip(self.strategies, self.weights):
                out += positive_regret_policy(net(feats), masks) * (w / total)
        return out

    def policy_table_device(self, ctx, player, out):
        """The average policy at every infoset of `player` of ctx's deal, into the rows of out ([n_infosets][4] float64 device tensor, hand order),
        normalised with the uniform fallback of evaluate_vs_random (scopa_sdcfr_average_policy: two launches on ctx's stream, no wait)."""
        n = len(self._slots)
        if n and self._device_args is None:
            total = float(sum(self.weights))
            dev = self._store[0].device
            self._device_args = (torch.tensor(self._slots, dtype=torch.int32, device=dev),
                                 torch.tensor([w / total for w in self.weights], dtype=torch.float32, device=dev))   # float32(weight / total), as the reference's product rounds it
        slots, coef = self._device_args if n else (None, None)
        ctx.sdcfr_average_policy(player, n, [t.data_ptr() for t in self._store] if n else [0] * 6, self.max_size,
                                 slots.data_ptr() if n else 0, coef.data_ptr() if n else 0, out.data_ptr())

    def get_average_policy(self, state_features, legal_actions_mask):
        dev = self._store[0].device if self._store is not None else "cpu"
        f = torch.as_tensor(np.asarray(state_features), dtype=torch.float32, device=dev).unsqueeze(0)
        m = torch.as_tensor(np.asarray(legal_actions_mask), dtype=torch.float32, device=dev).unsqueeze(0)
        return self.average_policy_batch(f, m)[0].cpu().numpy()


class RandomPolicy:
    def action_probabilities(self, state, player_id=None):
        if state.is_terminal():
            return {}
        if player_id is None:
            player_id = state.current_player()
        legal_actions = state.legal_actions(player_id)
        prob = 1.0 / len(legal_actions)
        return {action: prob for action in legal_actions}


class DeepCFR:
    """`DeepCFR(game, num_players=2, device="cuda").train(iterations, advantage_epochs, eval_freq)`."""

    def __init__(self, game, num_players=2, device="cuda", batch=1, seed=0x5C09A, stream=None, rank=0, world=1,
                 memory_size=None, graph_training=False, fused_traversal=None, train_backend="torch"):
        """rank/world: data parallelism over torch.distributed (one process per GPU).  Each rank traverses `batch`
        traversals with global ids [rank*batch, (rank+1)*batch) into its own memory ring and the advantage-net
        gradients are averaged with one all-reduce per optimiser step (55 104 B), so every replica's nets stay equal."""
        if not str(device).startswith("cuda"):
            raise ValueError("the SDCFR traversal runs on the GPU (HIP kernels): device must be a cuda device")
        self.game = game
        self.num_players = num_players
        self.device = device
        self.batch = int(batch)
        dev_index = torch.device(device).index or 0
        self._stream = stream if stream is not None else torch.cuda.Stream(device=dev_index)
        self._engine = Engine(game, device=dev_index, stream=self._stream.cuda_stream)
        self._engine.ctx.mccfr_seed(seed)
        self.input_dim = self._estimate_input_dim()
        print(f"Estimated input dimension: {self.input_dim}")
        with torch.cuda.stream(self._stream):
            # the reference keeps 100 000 rows (~2 400 traversals); a batch of B traversals appends 41*B rows at once,
            # so large batches get a ring of >= 8 iterations' worth (FIFO semantics unchanged)
            if memory_size is None:
                memory_size = max(100000, 8 * ROWS_PER_TRAVERSAL * self.batch)
            if memory_size < ROWS_PER_TRAVERSAL * self.batch:
                raise ValueError("memory_size must hold at least one batch of traversals (41 rows each)")
            self.advantage_nets = [AdvantageNetwork(self.input_dim, 16, device, memory_size=memory_size, use_graph=graph_training, train_backend=train_backend)
                                   for _ in range(num_players)]
            for a in self.advantage_nets:
                a._ctx, a._ctx_stream = self._engine.ctx, self._stream
        self.strategy_buffers = [StrategyBuffer() for _ in range(num_players)]
        self.training_history = {"losses": [[] for _ in range(num_players)], "values": [[] for _ in range(num_players)],
                                 "buffer_sizes": [[] for _ in range(num_players)], "eval_rewards": [], "eval_scopas": []}
        self._iteration = 0
        self._eval_calls = 0
        # the library's traversal call (scopa_sdcfr_traverse_fused: the deal's decision nodes evaluated once per launch on the matrix cores, then the
        # traversals as walks over that policy table) is the faster path at every batch size measured (1.6e10 visits/s at B=4096, 3.1-3.8e10 at
        # B=32768 against 3.2e8 / 9e8 for the ply-by-ply path around a PyTorch forward); the latter stays selectable
        self.fused_traversal = True if fused_traversal is None else bool(fused_traversal)
        self.rank, self.world = int(rank), int(world)
        if self.world > 1:
            import torch.distributed as dist
            from ...distributed import allreduce_gradients, broadcast_parameters

            def _ar(t):
                with torch.cuda.stream(self._stream):
                    dist.all_reduce(t, op=dist.ReduceOp.SUM)

            def _bc(t):
                with torch.cuda.stream(self._stream):
                    dist.broadcast(t, src=0)

            for a in self.advantage_nets:
                broadcast_parameters(a.net, _bc)
                a.grad_sync = lambda params: allreduce_gradients(params, self.world, _ar)

    # ---- encoders (host-facing, single state) ----------------------------------------------------------------------
    def _estimate_input_dim(self):
        return len(self._state_to_features(self.game.new_initial_state(), 0))

    def _state_to_features(self, state, player):
        """f32[34] = hand one-hot | table multi-hot | [player == current_player, 0] (deep_cfr.py:213-275)."""
        f = np.zeros(34, np.float32)
        if state.is_terminal():
            return f
        g = state.env.game
        for c in g.players[player].hand:
            f[c.id] = 1
        for c in g.table:
            f[16 + c.id] = 1
        f[32] = float(player == state.current_player())
        return f

    def _get_legal_actions_mask(self, state, player):
        mask = np.zeros(16, dtype=np.float32)
        mask[state.legal_actions(player)] = 1.0
        return mask

    # ---- the traversal ----------------------------------------------------------------------------------------------
    _PACK_KEYS = ("backbone.0.fc.weight", "backbone.0.fc.bias", "backbone.1.fc.weight", "backbone.1.fc.bias", "head.weight", "head.bias")

    @property
    def _ctx(self):
        """The library context whose stream the traversal launches and the packed weight image go to."""
        return self._engine.ctx

    def _packed_weights(self):
        """Both players' nets as the fused kernel keeps them in LDS (`scopa_sdcfr_pack_weights`: the operand layout of the
        16x16x4 MFMA), in one persistent buffer [2][13520].  A net's half is rebuilt -- ONE small launch -- only when the net
        has changed: `AdvantageNetwork.weights_epoch` counts train() calls (a replayed HIP graph updates the parameters without
        bumping their autograd version counters, so those alone would leave the image stale from the second graphed train()
        on) and load_state_dict; the parameters' storage and version counters catch in-place edits made around the class."""
        ctx = self._ctx
        if getattr(self, "_wpack", None) is None:
            self._wpack = torch.empty((len(self.advantage_nets), _lib.lib().scopa_sdcfr_image_floats()), dtype=torch.float32, device=self.device)
            self._wver = [None] * len(self.advantage_nets)
            self._wparams = [None] * len(self.advantage_nets)
        for p, a in enumerate(self.advantage_nets):
            if self._wparams[p] is None or self._wparams[p][0] is not a.net:      # the six parameters in the image's order, looked up once per net object
                named = dict(a.net.named_parameters())
                self._wparams[p] = (a.net, [named[k] for k in self._PACK_KEYS])
            tensors = self._wparams[p][1]                                          # (a Parameter replaced by ANOTHER object around the class would go unseen: load_state_dict and in-place edits do not do that)
            ver = (a.weights_epoch,) + tuple((t.data_ptr(), t._version) for t in tensors)
            if ver != self._wver[p]:
                if any(t.dtype != torch.float32 or not t.is_contiguous() for t in tensors):
                    tensors = [t.detach().to(torch.float32).contiguous() for t in tensors]
                ctx.sdcfr_pack_weights(p, *(t.data_ptr() for t in tensors), self._wpack.data_ptr())
                self._wver[p] = ver
        return self._wpack

    def _traverse_batch_fused(self, player, batch, uniforms=None, sync=True):
        """The library's traversal call: k_sdcfr_policy + k_sdcfr_walk (every decision node of the deal evaluated once per launch, the traversals as
        walks over that table), or k_sdcfr_traverse (a forward pass per visit in one launch) under `ctx.sdcfr_mode(1)` and for replayed draws.
        sync=False leaves the launches on the solver's stream (the training loop: the host goes on to draw the training batches while they run)."""
        ctx, dev = self._engine.ctx, self.device
        mem = self.advantage_nets[player].buffer
        with torch.cuda.stream(self._stream), torch.no_grad():
            w = self._packed_weights()
            vals = torch.empty(batch, dtype=torch.float32, device=dev)
            u = None
            if uniforms is not None:   # {ply: [batch * width]} -> [batch][8][24]
                u = torch.zeros((batch, 8, 24), dtype=torch.float64, device=dev)
                for ply, t in uniforms.items():
                    wd = t.numel() // batch
                    u[:, ply, :wd] = t.view(batch, wd)
            timed = getattr(self, "kernel_events", None)      # bench.py: [(start, stop)] torch events around the kernel launch itself
            if timed is not None:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(self._stream)
            ctx.sdcfr_traverse_fused(player, batch, w.data_ptr(), mem.feat.data_ptr(), mem.regret.data_ptr(), 0,   # no mask stream: DeviceMemory.mask
                                     mem.capacity, mem.write_base, vals.data_ptr(), u.data_ptr() if u is not None else 0,
                                     self._iteration, self.rank * batch)
            if timed is not None:
                e1.record(self._stream)
                timed.append((e0, e1))
            mem.advance(batch * ROWS_PER_TRAVERSAL)
        if sync:
            self._stream.synchronize()
        return vals

    def _traverse_batch(self, player, batch, uniforms=None, advantage_fn=None, fused=None, sync=True):
        """`batch` external-sampling traversals for `player` from the root; returns the root values [batch] (float32).
        uniforms: optional {ply: float64 tensor [n]} of draws for the opponent plies (replay / tests);
        advantage_fn(cur_player, feats, mask) -> raw advantages, default the current nets (forces the ply-by-ply path)."""
        if fused is None:
            fused = self.fused_traversal
        if fused and advantage_fn is None:
            return self._traverse_batch_fused(player, batch, uniforms, sync=sync)
        ctx, dev = self._engine.ctx, self.device
        mem = self.advantage_nets[player].buffer
        with torch.cuda.stream(self._stream), torch.no_grad():
            idx = torch.zeros(batch, dtype=torch.int32, device=dev)
            saved = []
            for ply in range(8):
                n = idx.numel()
                cur = ply & 1
                nl = 4 - (ply >> 1)
                feats = torch.empty((n, 34), dtype=torch.float32, device=dev)
                mask = torch.empty((n, 16), dtype=torch.float32, device=dev)
                ctx.sdcfr_features(ply, n, idx.data_ptr(), feats.data_ptr(), mask.data_ptr())
                adv = (advantage_fn(cur, feats, mask) if advantage_fn else self.advantage_nets[cur].net(feats)).contiguous()
                child = torch.empty(n * nl if cur == player else n, dtype=torch.int32, device=dev)
                pol = torch.empty((n, 4), dtype=torch.float32, device=dev)
                u = uniforms.get(ply) if uniforms else None
                ctx.sdcfr_expand(ply, player, n, idx.data_ptr(), adv.data_ptr(), child.data_ptr(), pol.data_ptr(),
                                 u.data_ptr() if u is not None else 0, self._iteration, self.rank * batch)
                saved.append((idx, pol, feats, mask))
                idx = child
            val = torch.empty(idx.numel(), dtype=torch.float32, device=dev)
            ctx.sdcfr_terminal_values(player, idx.numel(), idx.data_ptr(), val.data_ptr())
            for ply in range(7, -1, -1):
                nidx, pol, feats, mask = saved[ply]
                out = torch.empty(nidx.numel(), dtype=torch.float32, device=dev)
                ctx.sdcfr_backward(ply, player, nidx.numel(), nidx.data_ptr(), pol.data_ptr(), val.data_ptr(), out.data_ptr(),
                                   feats.data_ptr(), mask.data_ptr(), mem.feat.data_ptr(), mem.regret.data_ptr(), 0,
                                   mem.capacity, mem.write_base)
                val = out
            mem.advance(batch * ROWS_PER_TRAVERSAL)
        self._stream.synchronize()
        return val

    def _external_sampling_cfr(self, state, player, depth=0, prob=1.0):
        """One traversal from the initial state (the only way the reference calls it, deep_cfr.py:442-443)."""
        if state.is_terminal():
            return float(state.rewards()[player])
        if getattr(state, "action_history", None):
            raise NotImplementedError("_external_sampling_cfr starts at the initial state (as every reference caller does)")
        return float(self._traverse_batch(player, 1)[0].item())

    # ---- evaluation ----------------------------------------------------------------------------------------------------
    def get_policy(self, state, player):
        return self.strategy_buffers[player].get_average_policy(self._state_to_features(state, player),
                                                                self._get_legal_actions_mask(state, player))

    def evaluate_vs_random(self, num_episodes=100):
        """Average policy vs uniform random, seats swapped at half time (deep_cfr.py:367-429); all episodes advance in
        lockstep on the device (k_eval_step on packed states); the trained seat's policy is one batched forward per ply."""
        ctx, dev = self._engine.ctx, self.device
        n = int(num_episodes)
        self._eval_calls += 1
        with torch.cuda.stream(self._stream), torch.no_grad():
            states = torch.zeros((n, 4), dtype=torch.int32, device=dev)  # 16-byte packed states
            ctx.eval_init_states(states.data_ptr(), n)
            seat = (torch.arange(n, device=dev) >= (n + 1) // 2).to(torch.int32)     # episode e < n / 2: the trained agent sits in seat 0 (deep_cfr.py:386-389)
            feats = torch.empty((n, 34), dtype=torch.float32, device=dev)
            mask = torch.empty((n, 16), dtype=torch.float32, device=dev)
            for ply in range(8):
                ctx.features_from_states(states.data_ptr(), n, feats.data_ptr(), mask.data_ptr())
                probs = self.strategy_buffers[ply & 1].average_policy_batch(feats, mask).contiguous()
                ctx.eval_step(states.data_ptr(), n, probs.data_ptr(), seat.data_ptr(), 8, (self._eval_calls << 4) | ply)
            raw = states.cpu().numpy().view(_lib.STATE_DTYPE).reshape(-1)
        self._stream.synchronize()
        seat_h = (np.arange(n) >= (n + 1) // 2).astype(np.int64)
        r = raw["ncap"].astype(np.int64) + 2 * raw["scopas"].astype(np.int64)
        total = r.sum(1)
        rewards = np.where(total[:, None] == 0, 0.0, r - total[:, None] / 2.0)   # evaluate_game (mini_scopa_game.py:106-114)
        ar = np.arange(n)
        avg_reward = float(rewards[ar, seat_h].mean()) if n else 0.0
        trained = float(raw["scopas"][ar, seat_h].mean()) if n else 0.0
        rnd = float(raw["scopas"][ar, 1 - seat_h].mean()) if n else 0.0
        self.training_history["eval_rewards"].append(avg_reward)
        self.training_history["eval_scopas"].append([trained, rnd])
        from ..evaluation import match_halves
        self.last_eval_by_seat = match_halves(rewards[ar, seat_h], raw["scopas"][ar, seat_h].astype(np.float64),
                                              raw["scopas"][ar, 1 - seat_h].astype(np.float64), seat_h) if n else []
        return avg_reward, [trained, rnd]

    def policy_table(self):
        """The average policy (StrategyBuffer.get_average_policy, deep_cfr.py:137-160) at every infoset of the deal, normalised with the uniform
        fallback evaluate_vs_random plays (:391-397): [n_infosets][4] float64, hand order -- the tabular format of ctx.exploitability and of
        evaluate_agent_device(d, n, policy=d.policy_table()).  Queued on the solver's stream, behind any iteration queued before it."""
        ctx = self._engine.ctx
        with torch.cuda.stream(self._stream), torch.no_grad():
            out = torch.empty((ctx.n_infosets, 4), dtype=torch.float64, device=self.device)
            for player in range(self.num_players):
                self.strategy_buffers[player].policy_table_device(ctx, player, out)
            host = out.cpu()
        return host.numpy()

    def exploitability(self):
        """-> dict(exploitability, br0, br1, value_p0) of the average policy (policy_table), by the exact tabular evaluation the CFR solvers use."""
        return self._engine.ctx.exploitability(self.policy_table())

    def _queue_iteration(self, advantage_epochs, train_batch=128, loop_index=None):
        """One iteration's device work, QUEUED on the solver's stream and not waited for: per player the traversal call and the optimiser epochs (the
        other player's traversal reads the nets just trained: stream order), then the iteration's strategy snapshots.  Returns what `_resolve` reads
        back: per player (mean loss, mean root value) as device scalars (or floats, on the eager path) and an event behind all of it."""
        pending = []
        for player in range(self.num_players):
            vals = self._traverse_batch(player, self.batch, sync=False)
            with torch.cuda.stream(self._stream):
                loss = self.advantage_nets[player].train(batch_size=train_batch, epochs=advantage_epochs, defer=True)
                pending.append((loss, vals.mean(), len(self.advantage_nets[player].buffer)))
        # the snapshot rule counts iterations of THIS train() call, as the reference's loop variable does (deep_cfr.py:431, 460-471): none at its
        # first iteration, weight = loop index + 1 (the kernels' draws are keyed by the solver's own running count, self._iteration)
        loop_index = self._iteration if loop_index is None else loop_index
        if loop_index > 0:
            self._snapshot_strategies(loop_index)
        done = torch.cuda.Event()
        done.record(self._stream)
        self._iteration += 1
        return pending, done

    def _resolve(self, queued):
        """Waits for a queued iteration and appends its figures to training_history; returns (losses, values) per player."""
        pending, done = queued
        done.synchronize()
        losses, values = [], []
        for player, (loss, mean_value, rows) in enumerate(pending):
            loss, value = float(loss), float(mean_value.item())
            losses.append(loss)
            values.append(value)
            self.training_history["losses"][player].append(loss)
            self.training_history["values"][player].append(value)
            self.training_history["buffer_sizes"][player].append(rows)
        return losses, values

    # ---- training loop (deep_cfr.py:431-495) -------------------------------------------------------------------------
    def train(self, iterations=100, advantage_epochs=10, eval_freq=5, verbose=False, exploitability_freq=None):
        """The host stays ONE iteration ahead of the device: iteration t + 1 is queued before iteration t's losses are read back, so the GPU never waits
        for Python between iterations (it did for a sixth of every iteration); an evaluation (every eval_freq iterations) drains the queue first.
        exploitability_freq=k: at every iteration i with i % k == 0 the queue is drained the same way and (i, exploitability of the average policy)
        appended to training_history["exploitability"]."""
        if exploitability_freq is not None and (int(exploitability_freq) != exploitability_freq or exploitability_freq < 1):
            raise ValueError("exploitability_freq must be None or a positive integer")
        ahead = None
        for iteration in range(iterations):
            queued = self._queue_iteration(advantage_epochs, loop_index=iteration)
            if ahead is not None:
                self._resolve(ahead)
            ahead = queued
            if iteration % eval_freq == 0:
                iteration_losses, _ = self._resolve(ahead)
                ahead = None
                eval_reward, eval_scopas = self.evaluate_vs_random(num_episodes=50)
                if verbose:
                    print(f"iter {iteration}: P0 loss {iteration_losses[0]:.4f} P1 loss {iteration_losses[1]:.4f} "
                          f"eval vs random {eval_reward:.3f} scopas {eval_scopas[0]:.2f}/{eval_scopas[1]:.2f}")
            if exploitability_freq is not None and iteration % exploitability_freq == 0:
                if ahead is not None:
                    self._resolve(ahead)
                    ahead = None
                expl = self.exploitability()["exploitability"]
                self.training_history.setdefault("exploitability", []).append((iteration, expl))
                if verbose:
                    print(f"iter {iteration}: exploitability {expl:.5f}")
        if ahead is not None:
            self._resolve(ahead)

    def _snapshot_strategies(self, iteration):
        """A copy of every player's advantage net into its strategy buffer, weight iteration + 1 (deep_cfr.py:460-471): one multi-tensor copy each."""
        with torch.cuda.stream(self._stream):
            for player in range(self.num_players):
                self.strategy_buffers[player].add_strategy(self.advantage_nets[player].net, iteration, self.advantage_nets[player].param_list())

    def plot_training_progress(self, path="deep_cfr_training.png"):
        try:
            import matplotlib
            matplotlib.use("Agg")
            import matplotlib.pyplot as plt
        except ImportError:
            return
        fig, axes = plt.subplots(2, 2, figsize=(16, 12))
        for p in range(self.num_players):
            axes[0][0].plot(self.training_history["losses"][p], label=f"Player {p}")
            axes[0][1].plot(self.training_history["values"][p], label=f"Player {p}")
            axes[1][0].plot(self.training_history["buffer_sizes"][p], label=f"Player {p}")
        axes[0][0].set_title("Advantage Network Loss"); axes[0][1].set_title("Traversal value"); axes[1][0].set_title("Memory rows")
        axes[1][1].plot(self.training_history["eval_rewards"]); axes[1][1].set_title("Eval reward vs random")
        for a in axes.flat:
            a.grid(True)
        fig.savefig(path, dpi=120)


if __name__ == "__main__":
    from scopa_amd.envs import load_game
    d = DeepCFR(load_game("mini_scopa"), num_players=2, device="cuda")
    d.train(iterations=10, advantage_epochs=5, eval_freq=5, verbose=True)
    print(d.evaluate_vs_random(100))
