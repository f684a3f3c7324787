"""CPU checks of tests/full_chance_sdcfr_ref.py, the restatement the GPU suite of Deep CFR on FullScopa over decks (test_gpu_full_chance_sdcfr.py) is
held to, and of what the feature adds on the host: the features call, the bindings, DeviceMemory's regret width.

The restatement's level-by-level walk is held to a plain depth-first recursive external-sampling traversal over real states, per deck, driven by
the same draws and the same policy table; the features to a per-key statement, to the library's host call and to full_wide_key_fields' decoding."""
import os
import re

import numpy as np
import pytest

import full_chance_exploit_ref as X
import full_chance_ref as W
import full_chance_sdcfr_ref as S
import full_mccfr_ref as F

from conftest import ROOT

SEED = 0x5C09A
NEW = ("scopa_full_chance_sdcfr_features", "scopa_full_chance_sdcfr_traverse", "scopa_full_chance_sdcfr_visits", "scopa_full_chance_sdcfr_policy_get",
       "scopa_full_chance_sdcfr_average_policy", "scopa_full_chance_debug_sdcfr")
_CACHE = {}


def forest_of(oracle, R, n):
    """(Forest, decks, root state) of n decks of a packet below a fixed random root with R rounds to go"""
    from scopa_amd.algorithms import packet_decks
    if (R, n) not in _CACHE:
        r0 = 6 - R
        deck = oracle.full_deal_py_seed(42)
        st, _ = F.random_root(deck, r0, np.random.RandomState(100 * r0 + 42))
        decks = packet_decks(deck, r0, n, 5, fix_seat=0)
        _CACHE[(R, n)] = (S.Forest(X.tree_of(st, decks, R), R), decks, st)
    return _CACHE[(R, n)]


def tables_of(forest, seed):
    """a float32 policy table and its thresholds from two Xavier nets, the mover's at each level"""
    nets = [S.xavier_net(seed), S.xavier_net(seed + 1, head_bias=-0.05)]
    pol = np.zeros((len(forest.keys), 3), np.float32)
    for k in range(forest.L):
        sl_ = slice(forest.off[k], forest.off[k + 1])
        pol[sl_] = S.node_policy(nets[k & 1], forest.keys[sl_], forest.n_act[sl_])[0].astype(np.float32)
    return pol, S.thresholds_all(pol, forest.n_act)


def test_features_vs_host_call_and_key_decoding(sl, oracle):
    forest, _, _ = forest_of(oracle, 2, 5)
    keys = forest.keys
    feat = S.features(keys)
    assert feat.shape == (len(keys), 96) and feat.dtype == np.float32
    assert np.array_equal(sl.full_chance_sdcfr_features(keys), feat)
    uniq = np.unique(keys, axis=0)
    for a, b in uniq[:: max(1, len(uniq) // 300)].tolist():
        f = S.features_of(a, b)
        assert np.array_equal(f, S.features(np.array([[a, b]], np.uint64))[0])
        d = sl.full_wide_key_fields(a, b)
        assert [c for c in range(40) if f[c]] == d["hand"] and [c for c in range(40) if f[40 + c]] == d["table"]
        assert f[80 + d["round"]] == 1.0 and f[80:86].sum() == 1.0 and f[89] == d["player"] and not f[90:].any()
        assert f[86] * 64 == d["ncap"][d["player"]] and f[87] * 32 == d["scopas"][d["player"]] and f[88] * 32 == d["scopas"][1 - d["player"]]
        assert sl.full_wide_key_to_string(a, b) == W.key_to_string((a, b))
    assert (feat[:, :40].sum(1) == forest.n_act).all()                      # the hand one-hot is the legal-action mask
    assert sl.lib().scopa_full_chance_sdcfr_features(None, 1, None) == sl.SCOPA_EINVAL
    assert sl.lib().scopa_full_chance_sdcfr_features(None, -1, None) == sl.SCOPA_EINVAL
    assert sl.lib().scopa_full_chance_sdcfr_features(None, 0, None) == sl.SCOPA_OK


def test_thresholds_vectorised_equals_the_one_node_statement():
    rng = np.random.RandomState(3)
    pol = rng.rand(200, 3).astype(np.float32)
    n_act = rng.randint(2, 4, 200).astype(np.int32)
    pol[n_act == 2, 2] = 0.0
    pol[:20] = 0.0                                                         # zero policies: the uniform branch
    pol[20:40, 1] = 0.0
    pol = (pol / np.maximum(pol.sum(1, keepdims=True), 1e-8)).astype(np.float32)
    got = S.thresholds_all(pol, n_act)
    for i in range(200):
        assert np.array_equal(got[i], S.thresholds(pol[i], int(n_act[i]))), i
    assert (got[:20, 0] == S.ZERO_SUM).all()


def dfs(forest, decks, root, pol, thr, trav, deck, tid, iteration):
    """a depth-first recursive external-sampling traversal of deck `deck` on real states -> (value, rows {rank: (node, regret [40])}, visits)"""
    tree = [s // forest.n for s in forest.size]
    rank0, width, w, r = {}, {}, 1, 0
    for k in range(forest.L):
        width[k] = w
        if (k & 1) == trav:
            rank0[k] = r
            r += w
            w *= S.CARDS[k & 3]
    rows, visits = {}, [0]

    def rec(st, k, i, q):
        if st.s.terminal:
            v = np.float32(st.s.r2[0] / 2.0)
            return v if trav == 0 else np.float32(-v)
        p = int(st.s.step) & 1
        hand = sorted(F.hand(st, p))
        if len(hand) == 1:
            return rec(F.child(st, hand[0]), k, i, q)
        n = len(hand)
        g = deck * tree[k] + i
        idx = int(forest.off[k] + g)
        assert W.wide_key(st, p) == tuple(int(x) for x in forest.keys[idx]) and p == (k & 1) and n == S.CARDS[k & 3]
        visits[0] += 1
        if p != trav:
            a = S.action_of(thr[idx], S.draw_N(k, g, tid, iteration, trav, SEED), n)
            return rec(F.child(st, hand[a]), k + 1, i * n + a, q)
        av = [rec(F.child(st, hand[a]), k + 1, i * n + a, q * n + a) for a in range(n)]
        v, ri, d = S.row_of(pol[idx], av, n)
        rank = rank0[k] + q
        assert rank not in rows and q < width[k]
        rows[rank] = (idx, S.regret_row(forest.keys[idx, 1], ri, d))
        return v

    return rec(W.root_on(root, decks[deck]), 0, 0, 0), rows, visits[0]


@pytest.mark.parametrize("R,n", [(1, 3), (2, 5)])
def test_walk_equals_depth_first_recursion(oracle, R, n):
    forest, decks, root = forest_of(oracle, R, n)
    pol, thr = tables_of(forest, 11)
    thr[forest.off[1]:forest.off[1] + 2, 0] = S.ZERO_SUM                 # two nodes on the uniform branch
    for trav in (0, 1):
        for deck, tid in ((0, 0), (n - 1, 7), (1, (1 << 32) - 1)):
            got = S.walk(forest, pol, thr, trav, deck, tid, 5, SEED)
            value, rows, visits = dfs(forest, decks, root, pol, thr, trav, deck, tid, 5)
            assert np.float32(got["value"]).tobytes() == np.float32(value).tobytes()
            assert visits == got["visits"] == S.visits_per_traversal(R, trav)
            assert sorted(rows) == sorted(got["rows"]) == list(range(S.rows_per_traversal(R)))
            for rank, (idx, reg) in rows.items():
                assert got["rows"][rank][0] == idx and got["rows"][rank][1].tobytes() == reg.tobytes(), (trav, deck, rank)
    assert [S.rows_per_traversal(r) for r in (1, 2, 3, 4)] == [4, 28, 172, 1036]


def test_new_symbols_are_declared_bound_and_exported(sl):
    hdr = open(os.path.join(ROOT, "include", "scopa.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = sl.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in sl.SYMBOLS and hasattr(L, name) and getattr(L, name).argtypes is not None
    assert "#define SCOPA_FULL_SDCFR_FEATURES 96" in hdr and "#define SCOPA_FULL_SDCFR_ACTIONS 40" in hdr
    from scopa_amd.algorithms.deep_cfr import FullChanceDeepCFR
    from scopa_amd.algorithms.deep_cfr.full_chance_deep_cfr import default_memory_size, rows_per_traversal
    assert [rows_per_traversal(r) for r in (1, 2, 3, 4)] == [4, 28, 172, 1036]
    assert default_memory_size(1, 3, 5) == 100000 and default_memory_size(3, 8, 64) == 8 * 172 * 8 * 64
    assert FullChanceDeepCFR.__mro__[1].__name__ == "DeepCFR"


def test_device_memory_default_width_is_unchanged():
    import torch
    from scopa_amd.algorithms.deep_cfr import AdvantageNetwork, DeviceMemory
    old, new, wide = DeviceMemory(8, 34, "cpu"), DeviceMemory(8, 34, "cpu", num_actions=16), DeviceMemory(8, 96, "cpu", num_actions=40)
    assert old.regret.shape == new.regret.shape == (8, 16) and old.row_bytes == new.row_bytes == 200 and old.mask.shape == new.mask.shape == (8, 16)
    assert wide.regret.shape == (8, 40) and wide.mask.shape == (8, 40) and wide.row_bytes == 4 * 136
    g = torch.Generator().manual_seed(1)
    for mem in (old, new):
        mem.feat.copy_(torch.rand(8, 34, generator=torch.Generator().manual_seed(1)))
        mem.advance(5)
        mem.append(torch.ones(34), torch.full((16,), 0.5), torch.arange(16.0))
    for a, b in zip(old.gather(torch.tensor([0, 5, 7])), new.gather(torch.tensor([0, 5, 7]))):
        assert torch.equal(a, b)
    assert torch.equal(old.mask, new.mask) and old.total == new.total == 6 and old.mask_ptr[1].shape == (8, 16)
    wide.feat.copy_(torch.rand(8, 96, generator=g))
    assert wide.mask.data_ptr() == wide.feat.data_ptr() and torch.equal(wide.gather(torch.tensor([3]))[2], wide.feat[[3], :40])
    wide.append(torch.ones(96), torch.zeros(40), torch.arange(40.0))
    assert torch.equal(wide.mask[0], torch.arange(40.0))
    with pytest.raises(ValueError):
        AdvantageNetwork(96, 40, "cpu", memory_size=8, train_backend="hip")
    net = AdvantageNetwork(96, 40, "cpu", memory_size=8)
    assert net.buffer.regret.shape == (8, 40) and [tuple(p.shape) for p in net.param_list()] == [tuple(s) for s in S.SHAPES]
    assert AdvantageNetwork(34, 16, "cpu", memory_size=8, train_backend="hip").buffer.regret.shape == (8, 16)
