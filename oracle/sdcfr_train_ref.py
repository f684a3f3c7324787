"""Float64 restatement of the Deep CFR advantage net's optimiser step (the reference's AdvantageNetwork.train, deep_cfr.py:77-116), in numpy.

TEST INFRASTRUCTURE: written from the definitions of the operations, not from any implementation of them, so that every form of the step the
product has (autograd, the written-out lean step, their graph replays, the hand-written HIP launches) can be held to one independent statement:
  - the 34-128-64-16 ReLU MLP, parameters in net.parameters() order (W1 [128][34], b1, W2 [64][128], b2, W3 [16][64], b3);
  - loss = mean over batch x 16 of (pred m - target m)^2, whose gradient with respect to pred is 2 (pred - target) m^2 / (batch x 16);
  - clip_grad_norm_(max_norm=1): every gradient scaled by min(1, 1 / (||g||_2 + 1e-6)), ||g|| the 2-norm over all six tensors;
  - Adam (lr, betas (0.9, 0.999), eps 1e-8, no weight decay): m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g^2,
    p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps);
  - one train() call: with fewer than `batch_size` rows in memory the batch is min(n, 32); the index batches come from CPython's `random`
    seeded 42 followed by one shuffle of range(16) (the reference's MiniDeck()), then one sample(range(n), batch) per epoch.
The state is explicit (AdamState), so a test can start the reference from any snapshot of a device's weights and moments."""
import random

import numpy as np

SHAPES = [(128, 34), (128,), (64, 128), (64,), (16, 64), (16,)]
N_PARAMS = sum(int(np.prod(s)) for s in SHAPES)   # 13 776
LR, BETA1, BETA2, EPS, MAX_NORM, CLIP_EPS = 5e-4, 0.9, 0.999, 1e-8, 1.0, 1e-6


class AdamState:
    """Parameters, exp_avg, exp_avg_sq (lists of six float64 arrays in net.parameters() order) and Adam's step count.  shapes: the six parameter
    shapes of the net (the narrow net's unless given)."""

    def __init__(self, params, exp_avg=None, exp_avg_sq=None, step=0, shapes=SHAPES):
        self.shapes = list(shapes)
        shaped = lambda arrays: [np.array(a, dtype=np.float64).reshape(s) for a, s in zip(arrays, self.shapes)]
        zeros = lambda: [np.zeros(s) for s in self.shapes]
        self.params = shaped(params)
        self.exp_avg = zeros() if exp_avg is None else shaped(exp_avg)
        self.exp_avg_sq = zeros() if exp_avg_sq is None else shaped(exp_avg_sq)
        self.step = int(step)

    @staticmethod
    def from_flat(params, moments, step, shapes=SHAPES):
        """From the hand-written step's layout: a moment buffer [2][n_params] (exp_avg, then exp_avg_sq, each the six tensors flattened in order)."""
        mo = np.asarray(moments, dtype=np.float64).reshape(2, n_params(shapes))
        return AdamState(params, split_flat(mo[0], shapes), split_flat(mo[1], shapes), step, shapes)


def n_params(shapes):
    return sum(int(np.prod(s)) for s in shapes)


def split_flat(flat, shapes=SHAPES):
    """A flat [n_params] vector -> the six parameter-shaped arrays."""
    out, off = [], 0
    for s in shapes:
        k = int(np.prod(s))
        out.append(np.asarray(flat[off:off + k], dtype=np.float64).reshape(s))
        off += k
    assert off == len(flat)
    return out


def normalise_advantages(adv):
    """add_experience's normalisation (deep_cfr.py:70-75) in float32: adv / (max|adv| + 1e-8) when that maximum is positive."""
    a = np.asarray(adv, dtype=np.float32)
    peak = np.max(np.abs(a))
    return a / (peak + np.float32(1e-8)) if peak > 0 else a


def forward(params, x):
    """(pre-activations z1, z2, hidden h1, h2, output y) of the MLP on rows x [B][34]."""
    w1, b1, w2, b2, w3, b3 = params
    z1 = x @ w1.T + b1
    h1 = np.maximum(z1, 0.0)
    z2 = h1 @ w2.T + b2
    h2 = np.maximum(z2, 0.0)
    return z1, z2, h1, h2, h2 @ w3.T + b3


def loss_and_grad(params, x, t, m):
    """The masked MSE of one batch and its exact gradient (six arrays): float64 rows x [B][34], targets t and masks m [B][16]."""
    x, t, m = (np.asarray(a, dtype=np.float64) for a in (x, t, m))
    z1, z2, h1, h2, y = forward(params, x)
    r = y * m - t * m
    n = r.size
    loss = float(np.sum(r * r) / n)
    dy = 2.0 * r * m / n                      # d/dy of (y m - t m)^2 / n
    dz2 = (dy @ params[4]) * (z2 > 0)
    dz1 = (dz2 @ params[2]) * (z1 > 0)
    grads = [dz1.T @ x, dz1.sum(0), dz2.T @ h1, dz2.sum(0), dy.T @ h2, dy.sum(0)]
    return loss, grads


def step(state, x, t, m, lr=LR):
    """One optimiser step on a batch, in place on `state`.  Returns (loss, the gradient's 2-norm before clipping, the clip coefficient, the clipped
    gradient as one flat vector)."""
    loss, grads = loss_and_grad(state.params, x, t, m)
    norm = float(np.sqrt(sum(float(np.sum(g * g)) for g in grads)))
    coef = min(1.0, MAX_NORM / (norm + CLIP_EPS))
    state.step += 1
    bc1, bc2 = 1.0 - BETA1 ** state.step, 1.0 - BETA2 ** state.step
    for i, g in enumerate(grads):
        g = g * coef
        state.exp_avg[i] = BETA1 * state.exp_avg[i] + (1.0 - BETA1) * g
        state.exp_avg_sq[i] = BETA2 * state.exp_avg_sq[i] + (1.0 - BETA2) * g * g
        state.params[i] = state.params[i] - (lr / bc1) * state.exp_avg[i] / (np.sqrt(state.exp_avg_sq[i]) / np.sqrt(bc2) + EPS)
    return loss, norm, coef, np.concatenate([g.reshape(-1) for g in grads]) * coef


def index_batches(n, batch_size, epochs):
    """The reference's batch rule and index draws for one train() call on a memory of n rows: ([epochs][k] deque positions, k)."""
    k = batch_size if n >= batch_size else min(n, 32)
    if k == 0:
        return [], 0
    rng = random.Random()
    rng.seed(42)
    rng.shuffle(list(range(16)))
    return [rng.sample(range(n), k) for _ in range(epochs)], k


def train(state, feats, targets, masks, batch_size=128, epochs=1, lr=LR, info=None):
    """One train() call on a memory whose rows are feats [n][inputs], targets [n][outputs], masks [n][outputs] (34 and 16 for the narrow net; the
    widths are those of `state`'s shapes) in deque order (0 = oldest): `epochs` steps in place on `state`; returns the mean loss (0.0 on an empty
    memory).  info: an optional list that receives what step() returns, per step."""
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


# ---- holding a float32 implementation of the step to this one (teacher forcing: the reference starts each train() call from the implementation's own
#      weights and moments, so errors do not compound from call to call) ----
LOSS_RTOL = 1e-5          # loss: relative
MOMENT_RTOL, MOMENT_FLOOR = 1e-4, 1e-6   # exp_avg, exp_avg_sq: |d| <= 1e-4 |x64| + 1e-6 max|x64| (max over the parameter tensor)
WEIGHT_ATOL = 1e-5        # weights: absolute
RESOLUTION = 1e-4         # exclusion rule: a weight whose clipped float64 gradient was <= 1e-4 max|g| at some step of the call
MAX_EXCLUDED = 8          # ... may miss WEIGHT_ATOL (a float32 gradient that small is rounding noise, and Adam turns its sign into a +-lr step);
                          #     at most this many per call
SCALE_TOL = 2e-6          # median over the weights of (update made) / (float64 update): the size of Adam's step (lr, bias corrections)


def assert_call_matches(before, ref, ref_loss, info, loss, params, exp_avg, exp_avg_sq, what="", shapes=SHAPES):
    """One train() call of a float32 implementation against the reference run from the same starting point.
    before: the implementation's parameters before the call (six arrays); ref: the AdamState after the reference's call; ref_loss, info: what
    train() returned and recorded; loss, params, exp_avg, exp_avg_sq: the implementation's loss and state after the call; shapes: the net's six
    parameter shapes.
    Returns the largest deviations measured: {"loss", "exp_avg", "exp_avg_sq", "weight", "weight_kept", "excluded", "scale"}."""
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
    # weights: the exclusion rule is the float64 gradient's own size (info: per step (loss, norm, coef, clipped gradient as a flat vector))
    tiny = np.zeros(n_params(shapes), dtype=bool)
    for _, _, _, g in info:
        tiny |= np.abs(g) <= RESOLUTION * np.max(np.abs(g))
    p_dev = np.concatenate([np.asarray(p, dtype=np.float64).reshape(-1) for p in params])
    p_ref = np.concatenate([p.reshape(-1) for p in ref.params])
    p_0 = np.concatenate([np.asarray(p, dtype=np.float64).reshape(-1) for p in before])
    assert p_dev.shape == p_ref.shape == p_0.shape == tiny.shape
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
    # the size of the step: Adam's normalisation hides a uniformly scaled gradient, not a mis-scaled update (bias corrections, lr)
    d_ref, d_dev = p_ref - p_0, p_dev - p_0
    # (not on a state's first Adam step: there every update is +-lr (m / sqrt(v) = sign g), so its float32 rounding is the same for all the weights of
    # one binade and biases the median; from the second step on the updates vary from weight to weight)
    big = (np.abs(d_ref) >= 0.1 * LR) & ~tiny
    out["scale"] = 0.0
    if big.sum() >= 100 and ref.step > len(info):                # (the call did not start from a fresh optimiser)
        out["scale"] = float(abs(np.median(d_dev[big] / d_ref[big]) - 1.0))
        assert out["scale"] <= SCALE_TOL, f"{what}: the update is {out['scale']:.3g} off in size (median ratio to the float64 update)"
    return out
