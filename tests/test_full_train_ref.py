"""The float64 statement of the 96-128-64-40 optimiser step (tests/full_train_ref.py) on the CPU, and what the hand-written step adds on the host.

1. the restatement against torch float64: its gradient against autograd, three train() calls against MSELoss / clip_grad_norm_ / torch.optim.Adam;
2. the exclusion cap of assert_call_matches (at most 8 weights per call at float32 gradient resolution) as a condition on the INPUTS: PyTorch's own
   float32 step on the CPU stays within it on every memory recipe and batch of tests/test_gpu_full_train.py (synthetic rows where that suite's come
   from a traversal kernel: features of real key pairs, mask = features[:40], normalised random regrets on the mask), three teacher-forced calls each;
3. FullAdvantageNetwork refuses Adam settings the kernel does not implement; FullChanceDeepCFR refuses an unknown train_backend; the bindings."""
import copy
import os
import re

import numpy as np
import pytest

import full_train_ref as T

from conftest import ROOT

_CACHE = {}


def _net64(seed):
    import torch
    from scopa_amd.algorithms.deep_cfr.nets import FlexibleNet
    torch.manual_seed(seed)
    return FlexibleNet(mode="mlp", input_shape=(96,), output_dim=40, mlp_hidden=[128, 64], mlp_act="relu", mlp_norm="none", mlp_dropout=0.0).double()


def _random_memory(seed, n, kind):
    rng = np.random.default_rng(seed)
    x = (rng.random((n, 96)) > 0.7).astype(np.float32)
    x[:, 92:] = rng.standard_normal((n, 4))
    t = np.stack([T.normalise_advantages(r) for r in rng.standard_normal((n, 40))])
    m = np.stack([{"binary": T.binary_mask, "fractional": T.fractional_mask, "zero": T.zero_mask}[kind](rng) for _ in range(n)])
    return x, t, m


def test_shapes_and_parameter_count():
    from scopa_amd.algorithms.deep_cfr.full_chance_deep_cfr import FULL_TRAIN_PARAMS
    assert T.N_PARAMS == 23272 == FULL_TRAIN_PARAMS
    assert [tuple(p.shape) for p in _net64(0).parameters()] == T.SHAPES
    flat = np.arange(T.N_PARAMS, dtype=np.float64)
    assert np.array_equal(np.concatenate([a.reshape(-1) for a in T.split_flat(flat)]), flat)


@pytest.mark.parametrize("kind", ["binary", "fractional"])
def test_gradient_against_autograd_float64(kind):
    import torch
    net = _net64(5)
    x, t, m = _random_memory(6, 80, kind)
    loss, grads = T.loss_and_grad([p.detach().numpy() for p in net.parameters()], x, t, m)
    xb, tb, mb = (torch.from_numpy(np.asarray(a, np.float64)) for a in (x, t, m))
    lt = torch.nn.MSELoss()(net(xb) * mb, tb * mb)
    lt.backward()
    assert abs(loss - lt.item()) <= 1e-12 * abs(lt.item())
    for g, p in zip(grads, net.parameters()):
        ref = p.grad.numpy()
        assert np.max(np.abs(g - ref)) <= 1e-12 * np.max(np.abs(ref))


@pytest.mark.parametrize("kind,n,batch,scale", [("fractional", 300, 128, 1.0), ("binary", 300, 128, 100.0), ("zero", 200, 64, 1.0), ("fractional", 20, 128, 1.0)])
def test_train_calls_against_torch_float64(kind, n, batch, scale):
    """Three calls of 1 and of 3 epochs, clip and Adam included (moments and step count carry over), against torch in float64 to 1e-10."""
    import torch
    net = _net64(11)
    x, t, m = _random_memory(7, n, kind)
    t = t * scale                                           # (x 100: ||g|| above 1, the clip coefficient below 1)
    for epochs in (1, 3):
        tn = copy.deepcopy(net)
        opt = torch.optim.Adam(tn.parameters(), lr=5e-4)
        crit = torch.nn.MSELoss()
        s = T.AdamState([p.detach().numpy() for p in net.parameters()])
        for call in range(3):
            info = []
            lr_ = T.train(s, x, t, m, batch, epochs, info=info)
            batches, k = T.index_batches(n, batch, epochs)
            assert k == (batch if n >= batch else min(n, 32))
            total, norms = 0.0, []
            for idx in batches:
                xb, tb, mb = (torch.from_numpy(np.asarray(a, np.float64)[idx]) for a in (x, t, m))
                opt.zero_grad()
                loss = crit(tn(xb) * mb, tb * mb)
                loss.backward()
                norms.append(float(torch.nn.utils.clip_grad_norm_(tn.parameters(), max_norm=1.0)))
                opt.step()
                total += loss.item()
            assert abs(lr_ - total / epochs) <= 1e-10 * max(1.0, abs(total))
            np.testing.assert_allclose([i[1] for i in info], norms, rtol=1e-10, atol=1e-15)
            if kind == "zero":
                assert lr_ == 0.0 and all(i[1] == 0.0 and i[2] == 1.0 for i in info)
            elif kind == "binary":
                assert all(i[1] > 1 and i[2] < 1 for i in info)
            for i, (p, q) in enumerate(zip(s.params, tn.parameters())):
                st = opt.state[q]
                np.testing.assert_allclose(p, q.detach().numpy(), rtol=0, atol=1e-10)
                np.testing.assert_allclose(s.exp_avg[i], st["exp_avg"].numpy(), rtol=0, atol=1e-10)
                np.testing.assert_allclose(s.exp_avg_sq[i], st["exp_avg_sq"].numpy(), rtol=0, atol=1e-10)
                assert int(st["step"]) == s.step == (call + 1) * epochs


# ---- 2. the exclusion cap on the GPU suite's memories -------------------------------------------------------------------------------------------------
def _key_feats(sl, oracle, R):
    """features (host call) of the key pairs of real states: every node of 3 decks of a packet below a random root with R rounds to go"""
    import full_chance_exploit_ref as X
    import full_chance_sdcfr_ref as S
    import full_mccfr_ref as F
    from scopa_amd.algorithms import packet_decks
    if R not in _CACHE:
        r0 = 6 - R
        deck = oracle.full_deal_py_seed(42)
        st, _ = F.random_root(deck, r0, np.random.RandomState(100 * r0 + 42))
        decks = packet_decks(deck, r0, 3, 5, fix_seat=None if R == 1 else 0)
        forest = S.Forest(X.tree_of(st, decks, R), R)
        _CACHE[R] = sl.full_chance_sdcfr_features(np.ascontiguousarray(forest.keys, np.uint64))
        assert _CACHE[R].shape[1] == 96 and not _CACHE[R][:, 92:].any()
    return _CACHE[R]


def _cpu_memory(sl, oracle, name):
    """(host rows in deque order, which of them carry a mask of their own, capacity) of the GPU suite's memory `name`, kernel rows synthetic"""
    rng = np.random.default_rng(T.SEEDS[name.rstrip("0")] if name != "K20" else T.SEEDS["K"])
    if name in ("K", "K20"):
        f, r, m = T.synthetic_kernel_rows(rng, T.K_CALLS * T.ROWS_R2, _key_feats(sl, oracle, 2))
        n = 20 if name == "K20" else len(f)
        return (f[:n], r[:n], m[:n]), np.zeros(n, bool), 100000
    if name == "K1":
        f, r, m = T.synthetic_kernel_rows(rng, T.ROWS_R1, _key_feats(sl, oracle, 1))
        return (f, r, m), np.zeros(len(f), bool), 100000
    import collections
    if name in ("E", "F"):
        kf = _key_feats(sl, oracle, 2)
        host = collections.deque(maxlen=T.E_CAPACITY)
        T.fill_experience_memory(rng, T.binary_mask if name == "E" else T.fractional_mask, kf,
                                 lambda: host.extend((f, r, m, False) for f, r, m in zip(*T.synthetic_kernel_rows(rng, T.ROWS_R2, kf))),
                                 lambda x, adv, m: host.append((x, T.normalise_advantages(adv), m, True)))
        cap = T.E_CAPACITY
    else:                                                                     # Z0: the pre-call's rows (0/1 masks), then Z: every mask zero, from one generator
        kf = _key_feats(sl, oracle, 2)
        both = {k: [(x, T.normalise_advantages(adv), m, True) for x, adv, m in (T.experience_row(rng, masks, kf) for _ in range(T.Z_CAPACITY))]
                for k, masks in (("Z0", T.binary_mask), ("Z", T.zero_mask))}
        host, cap = both[name], T.Z_CAPACITY
    f, r, m, ex = (np.stack(c) for c in zip(*host))
    assert len(f) == cap
    return (f, r, m), ex, cap


def _cpu_net(host, explicit, cap, scale, seed=21):
    import torch
    from scopa_amd.algorithms.deep_cfr.deep_cfr import AdvantageNetwork
    torch.manual_seed(seed)
    a = AdvantageNetwork(96, 40, device="cpu", memory_size=cap)
    with torch.no_grad():
        for p in a.net.parameters():
            if p.dim() == 2:
                p.mul_(scale)
    _load(a, host, explicit)
    return a


def _load(a, host, explicit):
    import torch
    f, r, m = (torch.from_numpy(np.ascontiguousarray(x, np.float32)) for x in host)
    n = len(f)
    a.buffer.feat[:n], a.buffer.regret[:n] = f, r
    a.buffer.total = n
    a.buffer._explicit = a.buffer._side_mask = None
    if explicit.any():
        idx = torch.from_numpy(np.flatnonzero(explicit))
        a.buffer.put(idx, f[idx], r[idx], m[idx])
    fm = a.buffer.rows(torch.arange(n))[2].numpy()
    assert np.array_equal(fm, host[2])                                        # kernel-style rows: their mask IS features[:40]


CASES = ([("K", b, 1.0) for b in T.BATCHES_K] + [("K20", 128, 1.0)] + [("K1", b, 1.0) for b in T.BATCHES_K[:2]] +
         [(s, b, 3.0 if s == "E" else 1.0) for s in ("E", "F", "Z") for b in T.BATCHES_E])


@pytest.mark.parametrize("name,batch,scale", CASES)
def test_float32_torch_step_stays_within_the_exclusion_cap(sl, oracle, name, batch, scale):
    """The check on MAX_EXCLUDED = 8: PyTorch's float32 CPU step passes assert_call_matches on every memory and batch of the GPU suite."""
    host, explicit, cap = _cpu_memory(sl, oracle, name)
    worst = 0
    for epochs in (1, 3):
        if name == "Z":
            pre = _cpu_memory(sl, oracle, "Z0")
            a = _cpu_net(pre[0], pre[1], cap, scale)
            T.checked_call(a, pre[0], batch, epochs, f"cpu Z pre-call epochs={epochs}")
            _load(a, host, explicit)
        else:
            a = _cpu_net(host, explicit, cap, scale)
        for call in range(3):
            info, dev, _ = T.checked_call(a, host, batch, epochs, f"cpu {name} call {call} batch={batch} epochs={epochs}")
            worst = max(worst, dev["excluded"])
            if name == "E":
                assert all(i[1] > 1.0 for i in info)                          # the clip coefficient is below 1
            elif name == "Z":
                assert all(i[1] == 0.0 and i[2] == 1.0 for i in info)
            else:
                assert all(i[1] < 1.0 for i in info)
    assert worst <= T.MAX_EXCLUDED
    print(f"{name} batch {batch}: at most {worst} weights excluded per call")


# ---- 3. the host side of the feature -----------------------------------------------------------------------------------------------------------------
def test_subclass_refuses_other_adam_settings():
    import torch
    from scopa_amd.algorithms.deep_cfr import AdvantageNetwork
    from scopa_amd.algorithms.deep_cfr.full_chance_deep_cfr import FullAdvantageNetwork
    x, t, m = _random_memory(9, 32, "binary")
    for change in ({"betas": (0.8, 0.999)}, {"eps": 1e-6}, {"weight_decay": 0.01}, {"amsgrad": True}):
        a = FullAdvantageNetwork("cpu", memory_size=64)
        assert isinstance(a, AdvantageNetwork) and a.train_backend == "hip" and a.num_actions == 40 and a.buffer.feat.shape == (64, 96)
        for i in range(32):
            a.add_experience(x[i], t[i], m[i])
        a._ctx = object()                                                     # (never reached: the settings are checked before any launch)
        a.optimizer.param_groups[0].update(change)
        before = [p.detach().clone() for p in a.net.parameters()]
        with pytest.raises(RuntimeError, match="other settings need train_backend='torch'"):
            a.train(batch_size=32, epochs=1)
        assert all(torch.equal(p, q) for p, q in zip(a.net.parameters(), before)) and a._hip is None and a._hip_step == 0
    a = FullAdvantageNetwork("cpu", memory_size=64)
    for i in range(32):
        a.add_experience(x[i], t[i], m[i])
    with pytest.raises(RuntimeError, match="library context"):
        a.train(batch_size=32, epochs=1)                                      # without a solver's context there is nothing to launch on: an error, not PyTorch
    with pytest.raises(ValueError):
        AdvantageNetwork(96, 40, "cpu", memory_size=8, train_backend="hip")   # the base class keeps its refusal


def test_solver_rejects_unknown_train_backend():
    from scopa_amd.algorithms.deep_cfr import FullChanceDeepCFR
    with pytest.raises(ValueError, match="train_backend"):
        FullChanceDeepCFR(np.zeros((1, 40), np.uint8), train_backend="cuda")  # (refused before anything touches a device)
    import inspect
    assert inspect.signature(FullChanceDeepCFR.__init__).parameters["train_backend"].default == "torch"
    assert inspect.signature(FullChanceDeepCFR.train).parameters["train_batch"].default == 128


def test_bindings_and_header(sl):
    new = ("scopa_full_sdcfr_train_params", "scopa_full_sdcfr_train_steps")
    with open(os.path.join(ROOT, "include", "scopa.h")) as fh:
        header = fh.read()
    L = sl.lib()
    for name in new:
        assert name in sl.SYMBOLS and hasattr(L, name) and re.search(r"\b%s\(" % name, header)
    assert L.scopa_full_sdcfr_train_params() == T.N_PARAMS
    assert L.scopa_sdcfr_train_params() == 13776
    # a null context is refused on the host, without a device
    assert L.scopa_full_sdcfr_train_steps(None, None, 16, 1, None, None, None, 1, None, None, None, None, None, None, None, 1, 5e-4, None) == sl.SCOPA_EINVAL
    with open(os.path.join(ROOT, "scopa_amd", "build.py")) as fh:
        assert '"scopa_full_train.hip"' in fh.read()
