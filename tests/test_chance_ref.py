"""CPU checks of the chance game's float64 restatement (tests/chance_ref.py) that need no GPU: with ONE deal it is the C oracle's synchronous CFR
and exploitability, compared through the index map with np.array_equal -- which pins the restatement the GPU kernels are held to
(tests/test_gpu_chance.py) to code that is already pinned to the reference -- plus its keys, the deal sets of scopa_amd.algorithms.chance and
the entry points' presence in the header and the binding."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from chance_ref import ChanceRef, tree_keys


@pytest.fixture(scope="module")
def one(oracle):
    t = oracle.Tree(seed=42)
    return t, ChanceRef([t])


def test_keys_are_the_infoset_strings_and_the_index_is_their_rank(one, sl):
    t, ref = one
    keys = tree_keys(t)
    assert [sl.key_to_string(k) for k in keys] == t.infoset_strings
    assert ref.G == t.n_infosets == ref.n_occ and np.array_equal(ref.keys, np.sort(keys))
    assert np.array_equal(ref.keys[ref.map[0, :t.n_infosets]], keys) and (ref.map[0, t.n_infosets:] == -1).all()
    assert np.array_equal(ref.nlegal[ref.map[0, :t.n_infosets]], t.infoset_nlegal)
    assert np.array_equal(ref.player[ref.map[0, :t.n_infosets]], t.infoset_player)


@pytest.mark.parametrize("iters", [1, 5])
def test_one_deal_is_the_oracles_sync_cfr(one, iters):
    t, ref = one
    m = ref.map[0, :t.n_infosets]
    R, S = ref.tables()
    ref.run(R, S, np.ones((iters, 3)))
    Ro, So, _ = t.tables()
    t.cfr_sync(Ro, So, iters)
    assert np.array_equal(R[m], Ro) and np.array_equal(S[m], So)


def test_one_deal_is_the_oracles_exploitability(one):
    t, ref = one
    m = ref.map[0, :t.n_infosets]
    R, S = ref.tables()
    for S_now in (S.copy(), ref.run(R, S, np.ones((5, 3)))[1]):             # the uniform policy of an empty table, then a solved one
        P = ref.average_policy(S_now)
        assert np.array_equal(P[m], t.average_policy(np.ascontiguousarray(S_now[m])))
        e, br = t.exploitability(np.ascontiguousarray(P[m]))
        out = ref.exploitability(P)
        assert out[0] == e and np.array_equal(out[1:3], br) and out[3] == t.policy_value(np.ascontiguousarray(P[m]))


def test_the_same_deal_twice_doubles_the_tables(one, oracle):
    t, ref1 = one
    ref2 = ChanceRef([t, oracle.Tree(seed=42)])
    assert ref2.G == ref1.G and ref2.n_occ == 2 * ref1.n_occ and np.array_equal(ref2.map[0], ref2.map[1])
    w = np.array([[1.0, 0.0, 0.5], [1.0, 0.0, 2.0 / 3.0], [1.0, 0.0, 0.75]])
    R1, S1 = ref1.run(*ref1.tables(), w, True)
    R2, S2 = ref2.run(*ref2.tables(), w, True)
    assert np.array_equal(R2, 2.0 * R1) and np.array_equal(S2, 2.0 * S1)
    assert np.array_equal(ref2.exploitability(ref2.average_policy(S2)), ref1.exploitability(ref1.average_policy(S1)))


def test_hidden_hand_deals():
    from scopa_amd.algorithms.chance import hidden_hand_deals
    p = hidden_hand_deals([0, 5, 10, 15])
    assert p.shape == (495, 16) and p.dtype == np.uint8 and len({bytes(r) for r in p}) == 495
    assert (p[:, :4] == [0, 5, 10, 15]).all() and (np.sort(p, 1) == np.arange(16)).all()
    assert (np.diff(p[:, 4:8].astype(int), axis=1) > 0).all() and (np.diff(p[:, 8:].astype(int), axis=1) > 0).all()
    assert p[0].tolist() == [0, 5, 10, 15, 1, 2, 3, 4, 6, 7, 8, 9, 11, 12, 13, 14]
    with pytest.raises(ValueError):
        hidden_hand_deals([0, 0, 1, 2])


def test_entry_points_are_declared_and_bound(sl):
    names = ["scopa_chance_create", "scopa_chance_destroy", "scopa_chance_counts", "scopa_chance_index_get", "scopa_chance_tables_reset",
             "scopa_chance_tables_get", "scopa_chance_tables_set", "scopa_chance_cfr_iterate_weighted", "scopa_chance_exploitability",
             "scopa_chance_policy_for_deal"]
    with open(os.path.join(ROOT, "include", "scopa.h")) as f:
        header = f.read()
    for name in names:
        assert re.search(r"\b%s\(" % name, header) and name in sl.SYMBOLS and hasattr(sl.lib(), name), name
    assert sl.lib().scopa_chance_create(None, None) == sl.SCOPA_EINVAL and sl.lib().scopa_chance_destroy(None) == sl.SCOPA_EINVAL
