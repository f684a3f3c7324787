"""Float64 statement of one optimiser step of FullScopa's 96-128-64-40 advantage net: oracle/sdcfr_train_ref.py's shape-free functions (forward,
loss_and_grad, step, index_batches, normalise_advantages: the masked MSE over batch x outputs, clip_grad_norm_(1), Adam) on the wide net's shapes.

TEST INFRASTRUCTURE.  AdamState, split_flat and assert_call_matches are the oracle's, bound to the wide net's six shapes; train is the oracle's as it is
(the widths come from the state); the tolerances are the oracle's own, imported, not re-chosen."""
import functools

import numpy as np

import sdcfr_train_ref as R
from sdcfr_train_ref import (LOSS_RTOL, LR, MAX_EXCLUDED, MOMENT_FLOOR, MOMENT_RTOL, RESOLUTION, SCALE_TOL, WEIGHT_ATOL, forward, index_batches,  # noqa: F401
                             loss_and_grad, normalise_advantages, step, train)

SHAPES = [(128, 96), (128,), (64, 128), (64,), (40, 64), (40,)]
N_PARAMS = sum(int(np.prod(s)) for s in SHAPES)   # 23 272
FEATURES, ACTIONS = 96, 40


class AdamState(R.AdamState):
    def __init__(self, params, exp_avg=None, exp_avg_sq=None, step=0):
        super().__init__(params, exp_avg, exp_avg_sq, step, shapes=SHAPES)


split_flat = functools.partial(R.split_flat, shapes=SHAPES)
assert_call_matches = functools.partial(R.assert_call_matches, shapes=SHAPES)


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
