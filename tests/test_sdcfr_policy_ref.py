"""The float64 restatement of the Deep CFR forward pass, traversal and average policy (oracle/sdcfr_policy_ref.py) on the CPU, pinned before it
judges any kernel: against the reference's own numbers (tests/golden/sdcfr.npz), against the float32 oracle's traversal (og_sdcfr_traverse) on
Philox draws and three deals, and against torch's float64 FlexibleNet and positive_regret_policy."""
import numpy as np
import pytest

import philox_words as W
import sdcfr_policy_ref as R
from conftest import sdcfr_nets

SEED = 0x5C09A


def _ratio(err, tol):
    err, tol = np.asarray(err, np.float64), np.asarray(tol, np.float64)
    assert (err[tol == 0] == 0).all(), "a value with tolerance 0 (exact in float32) differs"
    return float(np.max(np.divide(err, tol, out=np.zeros_like(err), where=tol > 0), initial=0.0))


def _opponent_draw_order(trav):
    """(ply, slot) of every opponent visit in the reference's DFS order (one np.random.choice each)."""
    order = []

    def rec(ply, slot):
        if ply == 8:
            return
        n = 4 - (ply >> 1)
        if (ply & 1) == trav:
            for k in range(n):
                rec(ply + 1, slot * n + k)
        else:
            order.append((ply, slot))
            rec(ply + 1, slot)
    rec(0, 0)
    return order


def test_features_masks_and_policy_along_the_golden_line(oracle, golden):
    """feat_line (both players at every state of the first-legal line) and mask_line (the mover's: a player whose hand is empty gets the
    reference's legal-action fallback there, which no traversal asks for) exactly; policy_line (get_policy with one snapshot of weight 1 per
    player) within the float32 tolerance of regret matching."""
    g = golden.npz("sdcfr.npz")
    nt = R.NodeTable(oracle.Tree(seed=42), sdcfr_nets(g))
    t, st = nt.tree, nt.tree.states()
    v, k, line = 0, 0, []
    while not t.term[v]:
        for pl in (0, 1):
            f, m = R.state_features(st, v, pl)
            assert np.array_equal(f, g["feat_line"][k]), k
            assert pl != t.player[v] or np.array_equal(m, g["mask_line"][k]), k
            k += 1
        line.append(v)
        v = int(t.child[v, 0])
    assert k == len(g["feat_line"]) == 16 and len(line) == len(g["policy_line"])
    for r, v in enumerate(line):
        assert np.array_equal(nt.feat[v], g["feat_line"][2 * r + int(t.player[v])])
    assert _ratio(np.abs(nt.pol[line] - g["policy_line"]), nt.tol_p[line]) <= 1.0
    assert (nt.pol[line].sum(1) > 0.99).all()       # the fixture's nets: a positive advantage at every node of the line


@pytest.mark.parametrize("trav", [0, 1])
def test_visit_advantages_and_rows_of_the_reference_run(oracle, golden, trav):
    """Every advantage the reference computed in its traversal (trav{0,1}_visit_adv) within k 2^-24 S of the float64 forward pass; the traversal
    replayed with the fixture's own draws: the 41 rows (features and masks exactly, regrets within their tolerance) and the root value."""
    g = golden.npz("sdcfr.npz")
    nt = R.NodeTable(oracle.Tree(seed=42), sdcfr_nets(g))
    pl, f, m = g[f"trav{trav}_visit_player"], g[f"trav{trav}_visit_feat"], g[f"trav{trav}_visit_mask"]
    for p in (0, 1):
        adv, S = R.forward(nt.params[p], f[pl == p])
        legal = m[pl == p] > 0                  # get_advantages returns adv * mask - 1e6 (1 - mask) (deep_cfr.py:54-67)
        assert (g[f"trav{trav}_visit_adv"][pl == p][~legal] == -1e6).all()
        assert _ratio(np.abs(adv - g[f"trav{trav}_visit_adv"][pl == p])[legal], (R.K * R.U24 * S)[legal]) <= 1.0
    order = _opponent_draw_order(trav)
    u = np.random.RandomState(100 + trav).random_sample(len(order))
    uni = {ply: np.zeros(24) for ply in range(8)}
    for (ply, slot), x in zip(order, u):
        uni[ply][slot] = x
    out = R.traverse(nt, trav, uni, label=f"fixture traversal {trav}")
    assert np.array_equal(out.feat, g[f"trav{trav}_row_feat"]) and np.array_equal(out.mask, g[f"trav{trav}_row_mask"])
    assert _ratio(np.abs(out.regret - g[f"trav{trav}_row_regret"]), out.tol_regret) <= 1.0
    assert _ratio(abs(out.value - float(g[f"trav{trav}_value"][0])), out.tol_value) <= 1.0


def test_philox_draws_are_the_oracles():
    import oracle as O
    u = R.draws(1, [0, 7, 4095, 32767], SEED, 9)
    for i, b in enumerate((0, 7, 4095, 32767)):
        for ply, slot in ((0, 0), (2, 3), (4, 11), (6, 23), (7, 5)):
            assert u[i, ply, slot] == O.philox_uniform(SEED, slot + 1024 * ply, b, 9, 5)
    # ... and at the wide words of tests/philox_words.py: a high key word, iterations with bit 31 set, ids up to 2^32 - 1
    for seed, iteration, b0 in W.SD_WORD_CASES + [W.CH_WIDE[:3], W.CH_LAST[:3]]:
        ids = [b0, b0 + 1, b0 + W.SD_BATCH - 1] if b0 + W.SD_BATCH <= 1 << 32 else [b0, b0 + 6 * W.CH_BATCH - 1]
        for trav in (0, 1):
            u = R.draws(trav, ids, seed, iteration)
            for i, b in enumerate(ids):
                for ply, slot in ((0, 0), (3, 7), (6, 23), (7, 5)):
                    assert u[i, ply, slot] == O.philox_uniform(seed, slot + 1024 * ply, b, iteration, 4 + trav), (hex(seed), iteration, b)


def _feature_rows(t, nets, trav, seed, iteration, ids):
    """the oracle's feature rows of the traversals `ids`, in order: what the GPU tests compare exactly"""
    if ids == list(range(ids[0], ids[0] + len(ids))):
        return t.sdcfr_traverse(nets, trav, seed=seed, iteration=iteration, b0=ids[0], nb=len(ids))[0]
    return np.concatenate([t.sdcfr_traverse(nets, trav, seed=seed, iteration=iteration, b0=b, nb=1)[0] for b in ids])


def _assert_separates(t, nets, trav, seed, iteration, b0, nb):
    want = _feature_rows(t, nets, trav, seed, iteration, W.ids_of(b0, nb))
    variants = W.narrowed(seed, iteration, b0, nb)
    assert variants
    for what, s, it, ids in variants:
        assert not np.array_equal(_feature_rows(t, nets, trav, s, it, ids), want), (what, trav, nb)


@pytest.mark.parametrize("seed,iteration,b0", W.SD_WORD_CASES, ids=W.case_id)
def test_wide_word_traversals_separate(oracle, golden, seed, iteration, b0):
    """a condition on the inputs of tests/test_gpu_sdcfr.py::test_traversal_batch_at_wide_philox_words_vs_oracle: the feature rows it compares exactly
    differ from those of the same batch with the seed, the iteration or the ids narrowed (tests/philox_words.py)"""
    nets, t = sdcfr_nets(golden.npz("sdcfr.npz")), oracle.Tree(seed=42)
    for trav in (0, 1):
        _assert_separates(t, nets, trav, seed, iteration, b0, W.SD_BATCH)


def test_the_extreme_tuple_separates_at_the_form_batches(oracle, golden):
    """the same for the tuple the form-against-form tests of tests/test_gpu_sdcfr.py add, at their batches with more than one traversal (a single
    traversal can sample the same line under two keys: its case rides on the others)"""
    nets, t = sdcfr_nets(golden.npz("sdcfr.npz")), oracle.Tree(seed=42)
    seed, iteration, _ = W.SD_EXTREME
    for nb in W.SD_FORM_BATCHES:
        for trav in (0, 1):
            if nb > 1:
                _assert_separates(t, nets, trav, seed, iteration, W.sd_last_b0(nb), nb)


@pytest.mark.parametrize("seed,iteration,b0,deals", [W.CH_WIDE, W.CH_LAST], ids=["wide", "last-b0"])
def test_chance_form_wide_words_separate(oracle, seed, iteration, b0, deals):
    """tests/test_gpu_chance_sdcfr.py under the wide seed and at the accepted end of b0, with its own deals and nets: the rows of every listed deal's ids
    b0 + deal * batch + i differ from those of the narrowed words"""
    import torch
    import test_gpu_chance_sdcfr as G
    gen = torch.Generator().manual_seed(G.NET_SEED)
    nets = np.stack([np.concatenate([x.numpy().reshape(-1) for x in G.random_net_cpu(gen)]) for _ in range(2)]).astype(np.float32)
    for d in deals:
        t = oracle.Tree(perm=G.SIX[d])
        for trav in ((0, 1) if deals == W.CH_WIDE[3] else (0,)):
            first = b0 + d * W.CH_BATCH
            want = _feature_rows(t, nets, trav, seed, iteration, W.ids_of(first, W.CH_BATCH))
            for what, s, it, _ in W.narrowed(seed, iteration, b0, W.CH_BATCH):       # the words are narrowed BEFORE deal * batch is added, as a kernel would
                ids = W.ids_of(first, W.CH_BATCH)
                if what.startswith("b0 cut"):
                    ids = W.ids_of((b0 & ((1 << int(what.split()[-2])) - 1)) + d * W.CH_BATCH, W.CH_BATCH)
                elif what.startswith("b0 + i"):
                    ids = W.ids_of(first, W.CH_BATCH, 1 << 31)
                assert not np.array_equal(_feature_rows(t, nets, trav, s, it, ids), want), (what, d, trav)


@pytest.mark.parametrize("seed", [42, 7, 123])
def test_traversals_against_the_float32_oracle(oracle, golden, seed):
    """A few hundred Philox traversals per traverser on three deals against og_sdcfr_traverse (float32, the reference's operation order): the same
    rows in the same order, regrets and root values within the computed tolerance, and no ambiguous draw on these ids."""
    g = golden.npz("sdcfr.npz")
    nets = sdcfr_nets(g)
    t = oracle.Tree(seed=seed)
    nt = R.NodeTable(t, nets)
    for trav in (0, 1):
        for b0, n in ((0, 150), (4095, 1), (6143, 2), (20000, 1), (32767, 1)):             # iteration 35: no ambiguous draw on these ids, deals, nets
            feat, reg, mask, vals, _ = t.sdcfr_traverse(nets, trav, seed=SEED, iteration=35, b0=b0, nb=n)
            got = R.traverse_batch(nt, trav, range(b0, b0 + n), SEED, 35)
            assert np.array_equal(np.concatenate([x.feat for x in got]), feat) and np.array_equal(np.concatenate([x.mask for x in got]), mask)
            assert _ratio(np.abs(np.concatenate([x.regret for x in got]) - reg), np.concatenate([x.tol_regret for x in got])) <= 1.0
            assert _ratio(np.abs(np.array([x.value for x in got]) - vals), np.array([x.tol_value for x in got])) <= 1.0


def test_ambiguous_draws_are_refused(oracle, golden):
    """A draw placed on a sampling boundary of the float64 policy raises AmbiguousDraw naming the traversal instead of choosing a side."""
    g = golden.npz("sdcfr.npz")
    nt = R.NodeTable(oracle.Tree(seed=42), sdcfr_nets(g))
    t = nt.tree
    u = np.full((8, 24), 0.5)
    v = 0                                                   # traverser 1: the root is the opponent's (traverser 0's) node
    x = np.maximum(nt.adv[v, t.legal[v, :4]], 0.0)
    u[0, 0] = x[0] / x.sum()
    with pytest.raises(R.AmbiguousDraw, match="traversal 1234"):
        R.traverse(nt, 1, u, label="traversal 1234")
    u[0, 0] = x[0] / x.sum() + 1e-3
    R.traverse(nt, 1, u)


def _torch_net(params):
    import torch
    from scopa_amd.algorithms.deep_cfr.nets import FlexibleNet
    net = FlexibleNet(mode="mlp", input_shape=(34,), output_dim=16, mlp_hidden=[128, 64], mlp_act="relu", mlp_norm="none", mlp_dropout=0.0).double()
    net.load_state_dict({k: torch.from_numpy(p) for k, p in zip(R.SD_KEYS, params)})
    return net


def _perturbed(nets, seed, scale=0.05, shift=0.0):
    rng = np.random.default_rng(seed)
    out = []
    for p in range(2):
        w = np.asarray(nets[p], np.float32) + (scale * rng.standard_normal(R.N_PARAMS)).astype(np.float32)
        w[-16:] -= np.float32(shift)
        out.append(w)
    return out


def test_forward_and_regret_matching_against_torch_float64(oracle, golden):
    """The forward pass at every decision node of two deals and regret matching on crafted rows (ties, no positive advantage, positive advantages
    only outside the mask, a positive sum below 1e-8) against FlexibleNet(...).double() and positive_regret_policy, to 1e-12."""
    import torch
    from scopa_amd.algorithms.deep_cfr.nets import positive_regret_policy
    g = golden.npz("sdcfr.npz")
    for seed in (42, 7):
        for nets in (sdcfr_nets(g), _perturbed(sdcfr_nets(g), seed)):
            nt = R.NodeTable(oracle.Tree(seed=seed), nets)
            dec = np.nonzero(nt.tree.term == 0)[0]
            for p in (0, 1):
                sel = dec[nt.tree.player[dec] == p]
                with torch.no_grad():
                    adv = _torch_net(nt.params[p])(torch.from_numpy(nt.feat[sel].astype(np.float64))).numpy()
                np.testing.assert_allclose(nt.adv[sel], adv, rtol=0, atol=1e-12)
                pt = positive_regret_policy(torch.from_numpy(adv), torch.from_numpy(nt.mask[sel].astype(np.float64)), eps=R.EPS32).numpy()
                np.testing.assert_allclose(nt.pol[sel], pt, rtol=0, atol=1e-12)
    adv = np.zeros((6, 16))
    mask = np.zeros((6, 16))
    mask[:, [1, 4, 9, 12]] = 1
    adv[0, [1, 4, 9, 12]] = -0.5                       # no positive advantage: the all-zero row
    adv[1, [0, 2, 3]] = 2.0                            # positive advantages only outside the mask
    adv[2, [1, 4]] = 2.0 ** -30                        # positive sum 2^-29 < 1e-8: the clamp
    adv[3, [1, 4, 9]] = 0.25                           # ties
    adv[4, 9] = 0.75                                   # one positive action
    adv[5, [1, 4, 9]] = [0.5, 0.25, 0.25]
    p, tol, z, _ = R.positive_regret_policy(adv, mask)
    pt = positive_regret_policy(torch.from_numpy(adv), torch.from_numpy(mask), eps=R.EPS32).numpy()
    np.testing.assert_allclose(p, pt, rtol=0, atol=1e-12)
    assert (p[0] == 0).all() and (p[1] == 0).all() and p[2, 1] == 2.0 ** -30 / R.EPS32 and p[2].sum() < 0.19
    assert np.array_equal(p[3, [1, 4, 9]], [1 / 3] * 3) and p[4, 9] == 1.0 and np.array_equal(p[5, [1, 4, 9]], [0.5, 0.25, 0.25])


def test_average_policy_table_against_torch_float64(oracle, golden):
    """sum_s (w_s / W) prm(net_s(x)) over a FIFO of snapshots, against the same sum in torch float64, at every infoset of both players; the table
    normalised over the legal slots in hand order, uniform where the mix is all zero."""
    import torch
    from scopa_amd.algorithms.deep_cfr.nets import positive_regret_policy
    g = golden.npz("sdcfr.npz")
    t = oracle.Tree(seed=7)
    base = sdcfr_nets(g)
    snaps = [[], []]
    for s in range(5):
        for p, w in enumerate(_perturbed(base, 100 + s, shift=0.3 * (s % 3))):
            snaps[p].append(w)
    weights = [[1, 5, 9, 1000, 999999], [2, 2, 2, 2, 3]]
    table, tol, raw, _ = R.average_policy_table(t, snaps, weights)
    feat, mask = R.features(t)
    dec = np.nonzero(t.term == 0)[0]
    for p in (0, 1):
        sel = dec[t.player[dec] == p]
        acc = torch.zeros((sel.size, 16), dtype=torch.float64)
        for w, net in zip(weights[p], snaps[p]):
            with torch.no_grad():
                adv = _torch_net(R.net_params(net))(torch.from_numpy(feat[sel].astype(np.float64)))
            acc += positive_regret_policy(adv, torch.from_numpy(mask[sel].astype(np.float64)), eps=R.EPS32) * (w / sum(weights[p]))
        acc = acc.numpy()
        for r, v in enumerate(sel):
            i = t.infoset[v]
            nl = t.infoset_nlegal[i]
            a = acc[r, t.infoset_legal[i, :nl]]
            np.testing.assert_allclose(raw[i, :nl], a, rtol=0, atol=1e-12)
            want = a / a.sum() if a.sum() > 0 else np.full(nl, 1.0 / nl)
            np.testing.assert_allclose(table[i, :nl], want, rtol=0, atol=1e-12)
    assert np.isfinite(table).all() and np.allclose(table.sum(1), 1.0, rtol=0, atol=1e-12)
    assert (tol < 1.0).mean() > 0.9
    empty, etol, _, _ = R.average_policy_table(t, [[], []], [[], []])
    assert np.array_equal(empty, np.where(np.arange(4) < t.infoset_nlegal[:, None], 1.0 / t.infoset_nlegal[:, None], 0.0)) and (etol == 0).all()
