"""Float64 restatement of the Deep CFR forward pass and what is built on it, in numpy: the features of a node (deep_cfr.py:213-282), the
34-128-64-16 advantage MLP (nets.py:296-331), positive_regret_policy (nets.py:93-101), one external-sampling traversal (deep_cfr.py:284-365,
add_experience :70-75) and the StrategyBuffer average policy (:119-160) as the tabular policy evaluate_vs_random plays (:391-397).

TEST INFRASTRUCTURE: written from the definitions of the operations, not from any implementation of them.  It does not import the product;
the deal's tree, states, legal actions, infosets and payoffs come from oracle.Tree.

Tolerances.  Every float value comes with the float64 sum S of the absolute values of the terms it is made of, propagated forward:
  layer l:  S_l = |b_l| + |W_l| @ (|h_{l-1}| + S_{l-1} * live_{l-1})   (S_0 = 0: the features are exact; live = the unit's pre-activation
            lies above -tol, so ReLU can pass its error on; a unit below that passes nothing),
and a float32 implementation that sums those terms in any order is held to  tol = k * 2^-24 * S.  Built on it:
  - regret matching p_a = x_a / max(z, 1e-8), x = relu(adv) * mask, z = sum x:  tol_adv = k 2^-24 sum_a S_a over the masked actions whose
    advantage could be positive, and tol_p = tol_adv (1 + p) / max(z, 1e-8) + k 2^-24 p: an ill-conditioned node (z near 0) gets a wide
    tolerance and needs no exclusion list;
  - a sampling boundary r_k = cdf_k / cdf_last = (x_0 + .. + x_k) / z:  tol_adv (1 + r_k) / z + k 2^-24 r_k;
  - a traverser value v = sum p_a c_a:  sum (tol_p |c| + (p + tol_p) tol_c) + k 2^-24 sum |p c|;  a normalised regret d / (max|d| + 1e-8),
    d = cfv - v:  (tol_d + |r| max tol_d) / (max|d| + 1e-8) + k 2^-24 |r|;
  - an average-policy entry sum_s c_s p_s (FIFO, float32): sum_s c_s (tol_p_s + k 2^-24 p_s) + k 2^-24 * (the running sums of the FIFO order),
    then normalised over the legal slots like a sampling boundary.
The constants 1e-8 of clamp_min and of add_experience are float32 in the reference (float32 tensors and arrays), so they are float32(1e-8) here.

Draws.  The product keys an opponent's draw by (frontier slot + 1024 ply, traversal id, iteration, 4 + traverser) through Philox4x32-10 and
takes u = u53 of its first two words (oracle/scopa_oracle.c: og_philox4x32_10, og_sdcfr_traverse).  A draw that lies closer to a boundary
r_k than r_k's tolerance is AMBIGUOUS: float32 and float64 may honestly choose different actions there, so `traverse` raises AmbiguousDraw
naming the traversal instead of following one of the two paths; so does an opponent node whose positive mass z is within tolerance of 0 (the
uniform branch or not).

Measured on an MI355X (tests/test_gpu_sdcfr_policy_ref.py, K = 4), the largest |float32 - float64| / tolerance:
  regrets 0.028 and root values 0.0014 (walk, per-visit, ply-by-ply on the fixture's, perturbed and shifted nets); the walk's policy table 0.0135;
  exact-arithmetic nets: regrets 0.066, root values 0.067 (their advantages and policies are bit-exact); the average-policy table 0.0032.
  The bounds are worst-case sums, so these ratios sit far below 1; no element needed excluding."""
import numpy as np

import oracle as O

K = 4.0                                   # tolerance = K * 2^-24 * (the value's sum of |terms|)
U24 = 2.0 ** -24
EPS32 = float(np.float32(1e-8))           # clamp_min(1e-8) on float32 tensors; add_experience's + 1e-8 on float32 arrays
LEVEL_OFF = (0, 1, 5, 21, 69, 213, 501, 1077)
N_DECISION = 1653
SD_KEYS = ("backbone.0.fc.weight", "backbone.0.fc.bias", "backbone.1.fc.weight", "backbone.1.fc.bias", "head.weight", "head.bias")
SHAPES = ((128, 34), (128,), (64, 128), (64,), (16, 64), (16,))
N_PARAMS = sum(int(np.prod(s)) for s in SHAPES)    # 13 776


class AmbiguousDraw(AssertionError):
    pass


# ---- the net -------------------------------------------------------------------------------------------------------------------------------
def net_params(net):
    """A state dict (keys SD_KEYS; numpy or torch values), a list of six arrays in that order, or the oracle's flat [13 776] layout
    -> six float64 arrays holding float32 values."""
    if isinstance(net, dict):
        net = [net[k] for k in SD_KEYS]
    if not isinstance(net, (list, tuple)):
        flat = np.asarray(net, dtype=np.float32).reshape(-1)
        assert flat.size == N_PARAMS
        net, off = [], 0
        for s in SHAPES:
            n = int(np.prod(s))
            net.append(flat[off:off + n])
            off += n
    out = []
    for a, s in zip(net, SHAPES):
        a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
        out.append(np.asarray(a, dtype=np.float32).astype(np.float64).reshape(s))
    return out


def forward(params, x, k=K):
    """The MLP on rows x [n][34] (0/1 features): (advantages [n][16] float64, S [n][16] the propagated sums of |terms|)."""
    w1, b1, w2, b2, w3, b3 = params
    x = np.asarray(x, dtype=np.float64)
    z1 = x @ w1.T + b1
    s1 = np.abs(x) @ np.abs(w1).T + np.abs(b1)
    h1 = np.maximum(z1, 0.0)
    e1 = s1 * (z1 > -k * U24 * s1)
    z2 = h1 @ w2.T + b2
    s2 = (h1 + e1) @ np.abs(w2).T + np.abs(b2)
    h2 = np.maximum(z2, 0.0)
    e2 = s2 * (z2 > -k * U24 * s2)
    return h2 @ w3.T + b3, (h2 + e2) @ np.abs(w3).T + np.abs(b3)


def positive_regret_policy(adv, mask, S=None, k=K):
    """relu(adv) * mask / clamp_min(sum, 1e-8) on [n][16] rows -> (p, tol_p, z, tol_adv); without S the tolerances are zero."""
    adv, mask = np.asarray(adv, np.float64), np.asarray(mask, np.float64)
    pos = np.maximum(adv, 0.0) * mask
    z = pos.sum(-1, keepdims=True)
    den = np.maximum(z, EPS32)
    p = pos / den
    if S is None:
        return p, np.zeros_like(p), z[..., 0], np.zeros(z.shape[:-1])
    t = k * U24 * np.asarray(S, np.float64)
    tol_adv = (t * (mask > 0) * (adv > -t)).sum(-1, keepdims=True)
    tol_p = tol_adv * (1.0 + p) / den + k * U24 * p
    return p, tol_p, z[..., 0], tol_adv[..., 0]


# ---- the deal's decision nodes ---------------------------------------------------------------------------------------------------------------
def state_features(st, v, player):
    """(feat [34], mask [16]) float32 of node v of tree.states() `st` for `player` (the mover or not): hand one-hot | table multi-hot |
    [player == current player, 0]; the mask is the player's hand."""
    feat, mask = np.zeros(34, np.float32), np.zeros(16, np.float32)
    for c in st["hands"][v, player, :st["nh"][v, player]]:
        feat[c] = mask[c] = 1.0
    for c in st["table"][v, :st["nt"][v]]:
        feat[16 + c] = 1.0
    feat[32] = float(player == (st["step"][v] & 1))
    return feat, mask


def features(tree):
    """(feat [n_nodes][34], mask [n_nodes][16]) float32 for the player to move at every node of oracle.Tree `tree` (zero rows at terminals)."""
    st = tree.states()
    feat, mask = np.zeros((tree.n_nodes, 34), np.float32), np.zeros((tree.n_nodes, 16), np.float32)
    for v in np.nonzero(tree.term == 0)[0]:
        feat[v], mask[v] = state_features(st, v, int(tree.player[v]))
    return feat, mask


def level_index(tree):
    """[n_nodes] index of every decision node in the product's level order (ply d, then j: the children of node j of ply d are j nl + i,
    i = the legal actions in hand order), -1 at terminals."""
    out = np.full(tree.n_nodes, -1, np.int64)
    stack = [(0, 0, 0)]
    while stack:
        v, d, j = stack.pop()
        if tree.term[v]:
            continue
        out[v] = LEVEL_OFF[d] + j
        nl = int(tree.nlegal[v])
        for i in range(nl):
            stack.append((int(tree.child[v, i]), d + 1, j * nl + i))
    return out


class NodeTable:
    """Both players' nets evaluated in float64 at every decision node of `tree` (an oracle.Tree, or a deal seed; the mover's net at each node)."""

    def __init__(self, tree, nets, k=K, exact=False):
        """exact: nets whose every product and partial sum is exact in float32 (dyadic weights; exact_net): the advantages carry no tolerance,
        the policy is float32(x / max(z, 1e-8)) as the reference rounds it, and an opponent samples with the reference's own arithmetic
        (float32 probabilities and sum, a float64 cdf), so no draw is ambiguous."""
        if not isinstance(tree, O.Tree):
            tree = O.Tree(seed=int(tree))
        self.tree, self.k, self.exact = tree, k, exact
        self.params = [net_params(n) for n in nets]
        self.feat, self.mask = features(tree)
        n = tree.n_nodes
        self.adv, self.S = np.zeros((n, 16)), np.zeros((n, 16))
        dec = np.nonzero(tree.term == 0)[0]
        for p in (0, 1):
            sel = dec[tree.player[dec] == p]
            self.adv[sel], self.S[sel] = forward(self.params[p], self.feat[sel], k)
        if exact:
            assert np.array_equal(self.adv, self.adv.astype(np.float32)), "exact nets: an advantage is not a float32 value"
            self.S[:] = 0.0
        self.pol, self.tol_p, self.z, self.tol_adv = positive_regret_policy(self.adv, self.mask, self.S, k)
        if exact:
            assert np.array_equal(self.z, self.z.astype(np.float32)), "exact nets: a positive sum is not a float32 value"
            self.pol = self.pol.astype(np.float32).astype(np.float64)
        self.level = level_index(tree)

    def by_level(self):
        """(policy [1653][4], tolerance [1653][4], positive mass z [1653], tol_adv [1653]) in the product's level order, actions in hand order."""
        t = self.tree
        P, T, Z, TA = np.zeros((N_DECISION, 4)), np.zeros((N_DECISION, 4)), np.zeros(N_DECISION), np.zeros(N_DECISION)
        for v in np.nonzero(t.term == 0)[0]:
            i, nl = self.level[v], int(t.nlegal[v])
            lg = t.legal[v, :nl]
            P[i, :nl], T[i, :nl], Z[i], TA[i] = self.pol[v, lg], self.tol_p[v, lg], self.z[v], self.tol_adv[v]
        return P, T, Z, TA


# ---- Philox4x32-10 and the product's draws ------------------------------------------------------------------------------------------------------
def philox4x32_10(c0, c1, c2, c3, seed):
    """Vectorised over the counter words (broadcast uint32 arrays); key = (seed low, seed high)."""
    M = np.uint64(0xFFFFFFFF)
    c = [np.asarray(x, np.uint64) & M for x in (c0, c1, c2, c3)]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & M, p1 & M, ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & M, p0 & M]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M, (k1 + np.uint64(0xBB67AE85)) & M
    return c


def draws(traverser, ids, seed, iteration):
    """u [len(ids)][8][24] float64: the draw of frontier slot s at ply d of traversal ids[b] (every ply, both movers)."""
    ids = np.asarray(ids, np.uint64).reshape(-1, 1, 1)
    d = np.arange(8, dtype=np.uint64).reshape(1, 8, 1)
    s = np.arange(24, dtype=np.uint64).reshape(1, 1, 24)
    o = philox4x32_10(s + np.uint64(1024) * d, ids, np.uint64(iteration), np.uint64(4 + traverser), int(seed))
    return ((o[0] >> np.uint64(5)).astype(np.float64) * 67108864.0 + (o[1] >> np.uint64(6)).astype(np.float64)) / 9007199254740992.0


# ---- one traversal ------------------------------------------------------------------------------------------------------------------------------
class Traversal:
    """The rows (reference order: DFS post-order), their tolerances, the root value and its tolerance, and the margins of the draws."""

    def __init__(self):
        self.feat, self.mask, self.regret, self.tol_regret = [], [], [], []
        self.value = self.tol_value = 0.0
        self.margins = []        # per sampled opponent visit with two or more legal actions: (distance of u to the nearest boundary, its tolerance)


def traverse(nt, traverser, u, label=""):
    """One traversal for `traverser` over NodeTable nt with draws u[ply][slot] (float64 [8][24], or a dict {ply: [width]}).
    Raises AmbiguousDraw when a draw lies within tolerance of a sampling boundary."""
    t, k = nt.tree, nt.k
    out = Traversal()

    def rec(v, ply, slot):
        if t.term[v]:
            return 0.5 * float(t.r2[v, traverser]), 0.0
        p, nl = int(t.player[v]), int(t.nlegal[v])
        lg = t.legal[v, :nl]
        pol, tol = nt.pol[v], nt.tol_p[v]
        if p == traverser:
            c = np.zeros(16)
            tc = np.zeros(16)
            for i in range(nl):
                c[lg[i]], tc[lg[i]] = rec(int(t.child[v, i]), ply + 1, slot * nl + i)
            pv, tp = pol[lg], tol[lg]
            val = float(np.dot(pv, c[lg]))
            tval = float(np.sum(tp * np.abs(c[lg]) + (pv + tp) * tc[lg]) + k * U24 * np.sum(np.abs(pv * c[lg])))
            dlt = c - val
            tol_d = tc + tval + k * U24 * np.abs(dlt)
            mx = np.max(np.abs(dlt))
            if mx > 0:
                r = dlt / (mx + EPS32)
                tr = (tol_d + np.abs(r) * np.max(tol_d)) / (mx + EPS32) + k * U24 * np.abs(r)
            else:
                r, tr = dlt, tol_d / EPS32
            out.feat.append(nt.feat[v]); out.mask.append(nt.mask[v]); out.regret.append(r); out.tol_regret.append(tr)
            return val, tval
        uu = float(u[ply][slot])
        if nl == 1:
            a = 0
        elif nt.exact:                                      # action_probs / action_probs.sum() in float32, np.random.choice's float64 cdf
            ap = pol[lg].astype(np.float32)
            tot = ap[0]
            for i in range(1, nl):
                tot = np.float32(tot + ap[i])
            if tot == 0:
                a = min(int(uu * nl), nl - 1)
            else:
                cdf = np.cumsum((ap / tot).astype(np.float64))
                a = min(int(np.searchsorted(cdf / cdf[-1], uu, side="right")), nl - 1)
        else:
            x = np.maximum(nt.adv[v, lg], 0.0)
            zz, ta = float(x.sum()), float(nt.tol_adv[v])
            if zz <= ta and ta > 0:
                raise AmbiguousDraw(f"{label}: the opponent node at ply {ply}, slot {slot} has positive mass {zz:.3g} within its tolerance {ta:.3g}")
            if zz == 0.0:
                a = min(int(uu * nl), nl - 1)
            else:
                r = np.cumsum(x)[:-1] / zz
                a = int(np.searchsorted(r, uu, side="right"))
                tr = ta * (1.0 + r) / zz + k * U24 * r
                gap = np.abs(uu - r)
                j = int(np.argmin(gap - tr))
                out.margins.append((float(gap[j]), float(tr[j])))
                if gap[j] <= tr[j]:
                    raise AmbiguousDraw(f"{label}: draw {uu!r} at ply {ply}, slot {slot} lies {gap[j]:.3g} from boundary {r[j]!r} (tolerance {tr[j]:.3g})")
        return rec(int(t.child[v, a]), ply + 1, slot)

    out.value, out.tol_value = rec(0, 0, 0)
    out.feat, out.mask = np.array(out.feat, np.float32), np.array(out.mask, np.float32)
    out.regret, out.tol_regret = np.array(out.regret), np.array(out.tol_regret)
    return out


def traverse_batch(nt, traverser, ids, seed, iteration):
    """Traversals ids (the product's Philox draws) -> a list of Traversal."""
    u = draws(traverser, ids, seed, iteration)
    return [traverse(nt, traverser, u[i], label=f"traverser {traverser}, traversal {int(b)}, iteration {iteration}") for i, b in enumerate(ids)]


# ---- the average policy as a table ---------------------------------------------------------------------------------------------------------------
def average_policy_table(tree, snapshots, weights, players=(0, 1), k=K, feat=None):
    """StrategyBuffer.get_average_policy at every infoset of `players`: sum over the snapshots (FIFO order) of (w_s / W) prm(net_s(x)),
    normalised over the legal slots (hand order, tree.infoset_legal) with evaluate_vs_random's uniform fallback (sum <= 0).
    snapshots[p]: list of nets of player p; weights[p]: their weights.  Returns (table [n_infosets][4], tol [n_infosets][4], raw [n_infosets][4]
    the unnormalised mix, raw_tol); rows of other players' infosets are NaN.  A row whose legal mass is within tolerance of 0 gets tolerance 1."""
    if feat is None:
        feat = features(tree)
    f, m = feat
    I = tree.n_infosets
    table, tol = np.full((I, 4), np.nan), np.full((I, 4), np.nan)
    raw, raw_tol = np.full((I, 4), np.nan), np.full((I, 4), np.nan)
    for p in players:
        dec = np.nonzero((tree.term == 0) & (tree.player == p))[0]
        _, first = np.unique(tree.infoset[dec], return_index=True)
        nodes = dec[first]
        n = len(nodes)
        acc, acc_tol, run = np.zeros((n, 16)), np.zeros((n, 16)), np.zeros((n, 16))
        W = float(sum(weights[p]))
        for net, w in zip(snapshots[p], weights[p]):
            c = w / W
            adv, S = forward(net_params(net), f[nodes], k)
            pp, tp, _, _ = positive_regret_policy(adv, m[nodes], S, k)
            acc += c * pp
            acc_tol += c * (tp + 2 * k * U24 * pp)          # the term's tolerance, float32(w / W) and the product rounded
            run += acc                                      # the running sums of the FIFO order: the float32 sum's rounding
        if len(weights[p]) == 0:
            acc = m[nodes].astype(np.float64)
        acc_tol += k * U24 * run
        for r, v in enumerate(nodes):
            i, nl = int(tree.infoset[v]), int(tree.infoset_nlegal[tree.infoset[v]])
            lg = tree.infoset_legal[i, :nl]
            a, ta = acc[r, lg], acc_tol[r, lg]
            raw[i], raw_tol[i] = 0.0, 0.0
            raw[i, :nl], raw_tol[i, :nl] = a, ta
            s, ts = float(a.sum()), float(ta.sum())
            table[i], tol[i] = 0.0, 0.0
            if s > 0 and np.isfinite(s):
                table[i, :nl] = a / s
                tol[i, :nl] = (ts * (1.0 + a / s) / s + k * U24 * a / s) if len(weights[p]) else 0.0   # (no snapshot: the mask's exact uniform)
            else:
                table[i, :nl] = 1.0 / nl
            if 0 < s <= ts or (s == 0 and ts > 0):
                tol[i, :nl] = 1.0
    return table, tol, raw, raw_tol


def exact_net(values, const=0.25, out_bias=-0.25):
    """A net whose arithmetic is exact in float32 in any order: layer 1 copies features 0..31 to units 0..31 and the constant feature 32 to unit
    32 (W1[32][32] = 1; W1[:, 33] is non-zero too, but feature 33 is always 0: a bias fold that took column 33 would be seen), layer 2 copies
    units 0..32, the head gives adv[a] = values[a] x_a + const * 1 + out_bias.  values, const, out_bias: small dyadic numbers.
    -> the six arrays (float32) in state-dict order."""
    w1, b1 = np.zeros((128, 34), np.float32), np.zeros(128, np.float32)
    for i in range(33):
        w1[i, i] = 1.0
    w1[32:40, 33] = 0.5
    w1[40, 33] = -0.0625
    w2, b2 = np.zeros((64, 128), np.float32), np.zeros(64, np.float32)
    for i in range(33):
        w2[i, i] = 1.0
    w3, b3 = np.zeros((16, 64), np.float32), np.full(16, out_bias, np.float32)
    w3[np.arange(16), np.arange(16)] = np.asarray(values, np.float32)
    w3[:, 32] = const
    return [w1, b1, w2, b2, w3, b3]
