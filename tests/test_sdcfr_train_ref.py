"""The float64 restatement of the Deep CFR optimiser step (oracle/sdcfr_train_ref.py) on the CPU: against the reference's own numbers
(tests/golden/sdcfr.npz), against torch's float64 MSELoss / clip_grad_norm_ / Adam, and holding the product's eager step (_step) and graph mode's
written-out step (_step_lean) to it at 0/1 masks equal to the features, 0/1 masks of their own and fractional masks."""
import copy

import numpy as np
import pytest

import sdcfr_train_ref as R


def _golden_state(g):
    return R.AdamState([g[f"net0__{k}"] for k in g["net0_names"]])


def test_reference_train_reproduces_the_golden_run(golden):
    """The reference's DeepCFR: 41 rows of one traversal in memory, train(epochs=2) -> two Adam steps on min(41, 32)-row samples."""
    g = golden.npz("sdcfr.npz")
    s = _golden_state(g)
    assert int(g["train_buffer_len"][0]) == 41
    loss = R.train(s, g["trav0_row_feat"], g["trav0_row_regret"], g["trav0_row_mask"], batch_size=128, epochs=2)
    assert abs(loss - float(g["train_loss_p0_epochs2"][0])) < 1e-5
    assert s.step == 2
    for p, k in zip(s.params, g["net0_names"]):
        np.testing.assert_allclose(p, g[f"net0_after__{k}"], atol=1e-5, rtol=0)


def test_normalise_advantages_is_float32():
    a = np.array([0.5, -2.0, 0.0, 1.25] + [0.0] * 12, np.float32)
    out = R.normalise_advantages(a)
    assert out.dtype == np.float32 and np.array_equal(out, a / (np.float32(2.0) + np.float32(1e-8)))
    assert np.array_equal(R.normalise_advantages(np.zeros(16)), np.zeros(16, np.float32))


def _memory(seed, n, mask_kind):
    rng = np.random.default_rng(seed)
    x = (rng.random((n, 34)) > 0.6).astype(np.float32)
    t = np.stack([R.normalise_advantages(r) for r in rng.standard_normal((n, 16))])
    if mask_kind == "fractional":
        m = (rng.random((n, 16)) * 0.9).astype(np.float32)
        m[rng.random((n, 16)) < 0.3] = 0
        m[: n // 8] = 0                                     # rows whose every mask entry is zero
    elif mask_kind == "zero":
        m = np.zeros((n, 16), np.float32)
    elif mask_kind == "small":
        m = (rng.random((n, 16)) * 0.05).astype(np.float32)  # ||g|| well below 1: the clip coefficient is clamped to 1
    else:
        m = (rng.random((n, 16)) > 0.5).astype(np.float32)
    return x, t, m


def _torch_train(net, opt, x, t, m, batch_size, epochs):
    """The reference's train() written with torch's own float64 MSELoss, clip_grad_norm_ and Adam."""
    import torch
    batches, k = R.index_batches(len(x), batch_size, epochs)
    crit = torch.nn.MSELoss()
    total, norms = 0.0, []
    for idx in batches:
        xb, tb, mb = (torch.from_numpy(np.asarray(a, np.float64)[idx]) for a in (x, t, m))
        opt.zero_grad()
        loss = crit(net(xb) * mb, tb * mb)
        loss.backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(net.parameters(), max_norm=1.0)))
        opt.step()
        total += loss.item()
    return total / epochs, norms


@pytest.mark.parametrize("mask_kind,n,batch", [("fractional", 300, 128), ("binary", 300, 128), ("zero", 200, 64), ("small", 300, 128),
                                               ("fractional", 20, 128)])
def test_reference_against_torch_float64(mask_kind, n, batch):
    """Three calls of 1 and of 3 epochs (Adam's moments and step count carry over) against torch in float64: loss, norms, moments, weights to 1e-12."""
    import torch
    from scopa_amd.algorithms.deep_cfr.nets import FlexibleNet
    torch.manual_seed(11)
    net = FlexibleNet(mode="mlp", input_shape=(34,), output_dim=16, mlp_hidden=[128, 64], mlp_act="relu", mlp_norm="none", mlp_dropout=0.0).double()
    x, t, m = _memory(7, n, mask_kind)
    if mask_kind == "binary":
        t = t * 100.0                                     # larger errors: ||g|| above 1, the clip coefficient below 1
    for epochs in (1, 3):
        tn = copy.deepcopy(net)
        opt = torch.optim.Adam(tn.parameters(), lr=5e-4)
        s = R.AdamState([p.detach().numpy() for p in net.parameters()])
        for call in range(3):
            info = []
            lr_ = R.train(s, x, t, m, batch, epochs, info=info)
            lt, norms = _torch_train(tn, opt, x, t, m, batch, epochs)
            assert abs(lr_ - lt) <= 1e-12 * max(1.0, abs(lt))
            np.testing.assert_allclose([i[1] for i in info], norms, rtol=1e-12, atol=1e-15)
            if mask_kind == "zero":
                assert lr_ == 0.0 and all(i[1] == 0.0 and i[2] == 1.0 for i in info)    # no gradient: the clip coefficient is clamped, Adam takes 0 / eps
            elif mask_kind == "small":
                assert all(0 < i[1] < 1 and i[2] == 1.0 for i in info)
            elif mask_kind == "binary":
                assert all(i[1] > 1 and i[2] < 1 for i in info)
            for p, q in zip(s.params, tn.parameters()):
                np.testing.assert_allclose(p, q.detach().numpy(), rtol=0, atol=1e-12)
            for i, q in enumerate(tn.parameters()):
                st = opt.state[q]
                np.testing.assert_allclose(s.exp_avg[i], st["exp_avg"].numpy(), rtol=0, atol=1e-12)
                np.testing.assert_allclose(s.exp_avg_sq[i], st["exp_avg_sq"].numpy(), rtol=0, atol=1e-12)
                assert int(st["step"]) == s.step == (call + 1) * epochs


def _snapshot(a):
    """(parameters, exp_avg, exp_avg_sq, step) of a torch-optimised AdvantageNetwork, as float64 arrays."""
    ps = list(a.net.parameters())
    st = [a.optimizer.state.get(p, {}) for p in ps]
    w = [p.detach().cpu().double().numpy() for p in ps]
    ea = [s["exp_avg"].detach().cpu().double().numpy() if "exp_avg" in s else np.zeros(p.shape) for s, p in zip(st, ps)]
    eb = [s["exp_avg_sq"].detach().cpu().double().numpy() if "exp_avg_sq" in s else np.zeros(p.shape) for s, p in zip(st, ps)]
    step = int(st[0]["step"]) if "step" in st[0] else 0
    return w, ea, eb, step


@pytest.mark.parametrize("lean", [False, True], ids=["step", "step_lean"])
@pytest.mark.parametrize("mask_kind", ["features", "binary", "fractional"])
def test_product_step_on_the_cpu_against_the_reference(lean, mask_kind):
    """AdvantageNetwork._step (autograd) and _step_lean (graph mode's step with the backward pass written out), one train() call's epochs at a time,
    each call checked against the float64 reference started from the net's own weights and moments.  Masks: features[:16] (rows as a traversal
    writes them), explicit 0/1 masks that are not the features, fractional masks (the lean step once dropped their second factor)."""
    import torch
    from scopa_amd.algorithms.deep_cfr.deep_cfr import AdvantageNetwork
    torch.manual_seed(3)
    a = AdvantageNetwork(34, 16, device="cpu", memory_size=256)
    n = 200
    rng = np.random.default_rng(5)
    x = (rng.random((n, 34)) > 0.6).astype(np.float32)
    t = np.stack([R.normalise_advantages(r) for r in rng.standard_normal((n, 16))])
    if mask_kind == "features":
        m = x[:, :16].copy()
        a.buffer.feat[:n], a.buffer.regret[:n] = torch.from_numpy(x), torch.from_numpy(t)
        a.buffer.advance(n)                                       # kernel-style rows: no mask array, mask = features[:16]
    else:
        m = ((rng.random((n, 16)) > 0.5).astype(np.float32) if mask_kind == "binary" else
             np.where(rng.random((n, 16)) < 0.3, 0, rng.random((n, 16)) * 0.9).astype(np.float32))
        for i in range(n):
            a.add_experience(x[i], t[i], m[i])
        assert a.buffer._explicit is not None
    step = a._step_lean if lean else a._step
    for epochs in (1, 3, 3):
        before = _snapshot(a)
        s = R.AdamState(before[0], before[1], before[2], before[3])
        info = []
        ref_loss = R.train(s, x, t, m, 128, epochs, info=info)
        a._rng.seed(42)
        a._rng.shuffle(list(range(16)))                                # what train() does before it draws the batches
        rows = a._sample_rows(n, 128, epochs)
        loss = sum(float(step(rows[e]).detach()) for e in range(epochs)) / epochs
        after = _snapshot(a)
        assert after[3] == s.step
        R.assert_call_matches(before[0], s, ref_loss, info, loss, after[0], after[1], after[2], what=f"{'lean' if lean else 'autograd'} {mask_kind} {epochs}")
