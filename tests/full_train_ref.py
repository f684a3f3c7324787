"""Float64 statement of one optimiser step of FullScopa's 96-128-64-40 advantage net: oracle/sdcfr_train_ref.py's shape-free functions (forward,
loss_and_grad, step, index_batches, normalise_advantages: the masked MSE over batch x outputs, clip_grad_norm_(1), Adam) on the wide net's shapes.

TEST INFRASTRUCTURE.  AdamState, split_flat, train and assert_call_matches are restated here because the oracle's are written around the narrow net's
13 776 parameters; the tolerances are the oracle's own, imported, not re-chosen."""
import numpy as np

from sdcfr_train_ref import (LOSS_RTOL, LR, MAX_EXCLUDED, MOMENT_FLOOR, MOMENT_RTOL, RESOLUTION, SCALE_TOL, WEIGHT_ATOL, forward, index_batches,  # noqa: F401
                             loss_and_grad, normalise_advantages, step)

SHAPES = [(128, 96), (128,), (64, 128), (64,), (40, 64), (40,)]
N_PARAMS = sum(int(np.prod(s)) for s in SHAPES)   # 23 272
FEATURES, ACTIONS = 96, 40


class AdamState:
    """Parameters, exp_avg, exp_avg_sq (lists of six float64 arrays in net.parameters() order) and Adam's step count."""

    def __init__(self, params, exp_avg=None, exp_avg_sq=None, step=0):
        self.params = [np.array(p, dtype=np.float64).reshape(s) for p, s in zip(params, SHAPES)]
        zeros = lambda: [np.zeros(s) for s in SHAPES]
        self.exp_avg = zeros() if exp_avg is None else [np.array(a, dtype=np.float64).reshape(s) for a, s in zip(exp_avg, SHAPES)]
        self.exp_avg_sq = zeros() if exp_avg_sq is None else [np.array(a, dtype=np.float64).reshape(s) for a, s in zip(exp_avg_sq, SHAPES)]
        self.step = int(step)

    @staticmethod
    def from_flat(params, moments, step):
        """From the hand-written step's layout: a moment buffer [2][23 272] (exp_avg, then exp_avg_sq, each the six tensors flattened in order)."""
        mo = np.asarray(moments, dtype=np.float64).reshape(2, N_PARAMS)
        return AdamState(params, split_flat(mo[0]), split_flat(mo[1]), step)


def split_flat(flat):
    """A flat [23 272] vector -> the six parameter-shaped arrays."""
    out, off = [], 0
    for s in SHAPES:
        k = int(np.prod(s))
        out.append(np.asarray(flat[off:off + k], dtype=np.float64).reshape(s))
        off += k
    assert off == len(flat)
    return out


def train(state, feats, targets, masks, batch_size=128, epochs=1, lr=LR, info=None):
    """One train() call on a memory whose rows are feats [n][96], targets [n][40], masks [n][40] in deque order (0 = oldest): `epochs` steps in place
    on `state`; returns the mean loss (0.0 on an empty memory).  info: an optional list that receives what step() returns, per step."""
    feats, targets, masks = (np.asarray(a, dtype=np.float64) for a in (feats, targets, masks))
    batches, k = index_batches(len(feats), batch_size, epochs)
    if k == 0:
        return 0.0
    total = 0.0
    for idx in batches:
        out = step(state, feats[idx], targets[idx], masks[idx], lr)
        if info is not None:
            info.append(out)
        total += out[0]
    return total / epochs


def assert_call_matches(before, ref, ref_loss, info, loss, params, exp_avg, exp_avg_sq, what=""):
    """oracle/sdcfr_train_ref.py's assert_call_matches on 23 272 parameters: one train() call of a float32 implementation against the reference run
    from the same starting point, same bounds, same exclusion rule (at most MAX_EXCLUDED weights whose clipped float64 gradient was at most
    RESOLUTION max|g| at some step may miss WEIGHT_ATOL).  Returns the largest deviations measured."""
    out = {"loss": abs(float(loss) - ref_loss)}
    assert out["loss"] <= LOSS_RTOL * abs(ref_loss), f"{what}: loss {loss!r} vs float64 {ref_loss!r}"
    for name, dev, r64 in (("exp_avg", exp_avg, ref.exp_avg), ("exp_avg_sq", exp_avg_sq, ref.exp_avg_sq)):
        worst = 0.0
        for i, (d, x) in enumerate(zip(dev, r64)):
            err = np.abs(np.asarray(d, dtype=np.float64).reshape(x.shape) - x)
            bound = MOMENT_RTOL * np.abs(x) + MOMENT_FLOOR * np.max(np.abs(x))
            bad = np.flatnonzero(err > bound)
            assert bad.size == 0, f"{what}: {name} of parameter {i}: {bad.size} elements off, worst {err.flat[bad[0]]:.3g} at {bad[0]} (float64 {x.flat[bad[0]]:.6g})"
            worst = max(worst, float(err.max()) if err.size else 0.0)
        out[name] = worst
    tiny = np.zeros(N_PARAMS, dtype=bool)
    for _, _, _, g in info:
        tiny |= np.abs(g) <= RESOLUTION * np.max(np.abs(g))
    p_dev = np.concatenate([np.asarray(p, dtype=np.float64).reshape(-1) for p in params])
    p_ref = np.concatenate([p.reshape(-1) for p in ref.params])
    p_0 = np.concatenate([np.asarray(p, dtype=np.float64).reshape(-1) for p in before])
    assert p_dev.shape == p_ref.shape == p_0.shape == (N_PARAMS,)
    assert np.isfinite(p_dev).all(), f"{what}: a weight is not finite"
    err = np.abs(p_dev - p_ref)
    off = err > WEIGHT_ATOL
    excluded = np.flatnonzero(off & tiny)
    bad = np.flatnonzero(off & ~tiny)
    assert bad.size == 0, f"{what}: {bad.size} weights off by more than {WEIGHT_ATOL}, worst {err[bad].max():.3g} (element {bad[np.argmax(err[bad])]})"
    assert excluded.size <= MAX_EXCLUDED, f"{what}: {excluded.size} weights off at float32 gradient resolution (at most {MAX_EXCLUDED})"
    out["weight"] = float(err.max())
    out["weight_kept"] = float(err[~(off & tiny)].max())
    out["excluded"] = int(excluded.size)
    d_ref, d_dev = p_ref - p_0, p_dev - p_0
    big = (np.abs(d_ref) >= 0.1 * LR) & ~tiny
    out["scale"] = 0.0
    if big.sum() >= 100 and ref.step > len(info):                # (the call did not start from a fresh optimiser: see the oracle's note)
        out["scale"] = float(abs(np.median(d_dev[big] / d_ref[big]) - 1.0))
        assert out["scale"] <= SCALE_TOL, f"{what}: the update is {out['scale']:.3g} off in size (median ratio to the float64 update)"
    return out


# ---- teacher forcing: one train() call of an AdvantageNetwork checked against the reference run from the net's own state ----
def net_state(a, k):
    """(parameters, exp_avg, exp_avg_sq, step) of an AdvantageNetwork as float64 arrays: the hand-written step's own state when it takes a k-row
    batch, else optimizer.state."""
    ps = list(a.net.parameters())
    w = [p.detach().double().cpu().numpy() for p in ps]
    zeros = lambda: [np.zeros(p.shape) for p in ps]
    if a.train_backend == "hip" and k % 16 == 0:
        if a._hip is None:
            return w, zeros(), zeros(), 0
        mo = a._hip[0].double().cpu().numpy().reshape(2, N_PARAMS)
        return w, split_flat(mo[0]), split_flat(mo[1]), a._hip_step
    st = [a.optimizer.state.get(p, {}) for p in ps]
    if "exp_avg" not in st[0]:
        return w, zeros(), zeros(), 0
    return (w, [s["exp_avg"].double().cpu().numpy() for s in st], [s["exp_avg_sq"].double().cpu().numpy() for s in st],
            int(st[0]["step"].item()) if hasattr(st[0]["step"], "item") else int(st[0]["step"]))


def checked_call(a, host, batch, epochs, what, sync=lambda: None):
    """One a.train(batch, epochs) against the reference's call from the same weights, moments and step count on `host` = (feats, targets, masks) in
    deque order.  Returns (the reference's per-step (loss, norm, coef, grad), the deviations assert_call_matches measured, the warnings caught)."""
    import warnings
    k = index_batches(len(a.buffer), batch, 1)[1]
    before = net_state(a, k)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        loss = a.train(batch_size=batch, epochs=epochs)
    sync()
    after = net_state(a, k)
    s = AdamState(*before)
    info = []
    ref_loss = train(s, *host, batch_size=batch, epochs=epochs, info=info)
    assert after[3] == s.step, (what, after[3], s.step)
    dev = assert_call_matches(before[0], s, ref_loss, info, loss, after[0], after[1], after[2], what=what)
    dev["loss_rel"] = dev["loss"] / max(abs(ref_loss), 1e-30)
    return info, dev, caught


# ---- the memories of tests/test_gpu_full_train.py, as functions of a seed (the CPU suite holds PyTorch's float32 step to the exclusion cap on the same recipes) ----
P_CAP = 256                                   # the hand-written step's partial cap: workgroups of its gradient launch
ROWS_R1, ROWS_R2 = 4 * 3 * 16, 28 * 3 * 16    # rows of one traversal call of the two solvers: R = 1 and R = 2 on 3 decks, 16 traversals a deck
BATCHES_K = [16, 48, 16 * (P_CAP + 1)]        # one tile; fewer tiles than partials; one workgroup takes two tiles and the others one
BATCHES_E = [48, 128]
K_CALLS = 4                                   # traversal calls of the R = 2 solver in memory K: 5 376 rows, above the largest batch
E_CAPACITY = 1500                             # just above one iteration's 1 344 rows: the ring of memories E and F wraps
Z_CAPACITY = 600
SEEDS = {"K": 41, "K1": 42, "E": 43, "F": 44, "Z": 45}


def fill_experience_memory(rng, masks, key_feats, traverse, add):
    """memories E and F: a traversal call's rows, 300 rows with masks of their own, a second call (the ring wraps), 100 more rows over the oldest"""
    traverse()
    for _ in range(300):
        add(*experience_row(rng, masks, key_feats))
    traverse()
    for _ in range(100):
        add(*experience_row(rng, masks, key_feats))


def synthetic_kernel_rows(rng, n, key_feats):
    """n rows shaped like a traversal kernel's, for the CPU suite: the features of real key pairs (columns 92..95 zero), mask = features[:40],
    normalised random regrets supported on the mask -> (features, regrets, masks)"""
    f = np.asarray(key_feats, np.float32)[rng.integers(len(key_feats), size=n)]
    m = f[:, :ACTIONS].copy()
    adv = rng.standard_normal((n, ACTIONS)).astype(np.float32) * m
    return f, np.stack([normalise_advantages(a) for a in adv]), m


def binary_mask(rng):
    return (rng.random(ACTIONS) > 0.5).astype(np.float32)


def fractional_mask(rng):
    if rng.random() < 0.1:
        return np.zeros(ACTIONS, np.float32)                               # a row whose every mask entry is zero
    return np.where(rng.random(ACTIONS) < 0.3, 0, rng.random(ACTIONS) * 0.9).astype(np.float32)


def zero_mask(rng):
    return np.zeros(ACTIONS, np.float32)


def experience_row(rng, masks, key_feats):
    """(features, raw advantages, mask) of one add_experience row: the features of a real key pair with RANDOM values in columns 92..95 (which the
    traversal kernels leave 0), advantages supported on the mask."""
    x = np.array(key_feats[rng.integers(len(key_feats))], np.float32)
    x[92:96] = rng.standard_normal(4).astype(np.float32)
    m = masks(rng)
    adv = (rng.standard_normal(ACTIONS) * 3).astype(np.float32) * (m > 0)
    return x, adv, m
