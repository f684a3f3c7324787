"""CPU checks of the restatement of Team MiniScopa over a set of deals (tests/team_chance_ref.py) against tests/team_cfr_ref.py's Ref, of the index
it builds, of algorithms.team_chance's key helpers, and of the entry points' declaration, binding and export."""
import os
import re

import numpy as np
import pytest

import team_cfr_ref as T
import team_chance_ref as TC
from conftest import ROOT

PACKETS = [[0, 5, 10, 15], [1, 4, 11, 14], [2, 7, 8, 13], [3, 6, 9, 12]]
W = np.array([[0.5, 0.25, 0.75], [1.0, 0.0, 0.5]])


@pytest.fixture(scope="module")
def deals(oracle):
    from scopa_amd.algorithms.team_chance import packet_deals
    return packet_deals(PACKETS)


def rotations(deals):
    """four of the 24 packet deals whose seat-0 hands are pairwise disjoint: the cyclic shifts of the packets"""
    pick = [d for d in deals if [int(d[4 * s]) for s in range(4)] in ([0, 1, 2, 3], [1, 2, 3, 0], [2, 3, 0, 1], [3, 0, 1, 2])]
    assert len(pick) == 4
    return np.array(pick)


def test_walk_gives_the_enumerated_payoffs(oracle):
    perm = oracle.deal_py_seed(42)
    keys, r2 = TC.walk(perm)
    assert np.array_equal(r2, T.leaves(perm))
    assert len(np.unique(keys)) == T.N_CHOICE and np.array_equal(TC.key_depth(keys), np.repeat(np.arange(12), T.WIDTH[:12]))


def test_one_deal_is_the_one_deal_solver(oracle):
    perm = oracle.deal_py_seed(42)
    cr, ref = TC.ChanceRef([perm]), T.Ref(perm)
    assert cr.G == T.N_CHOICE
    R, S, sig = cr.tables()
    tabs = ref.tables()
    for kw in (dict(n_iters=2), dict(weights=W)):
        assert np.array_equal(cr.iterate(R, S, sig, **kw), ref.iterate(*tabs, **kw))
        for mine, theirs in zip((R, S, sig), tabs):
            assert np.array_equal(mine[cr.map[0]], theirs)
    pol = ref.average_policy(tabs[1])
    out, brs, _ = cr.exploitability(cr.average_policy(S))
    want, tables = ref.exploitability(pol, want_tables=True)
    np.testing.assert_allclose(out, want, rtol=0, atol=1e-12)   # opp * u may round a near-tie differently from the per-node maximum
    assert out[3] == want[3]


def test_disjoint_seat0_hands_share_no_row(deals):
    perms = rotations(deals)
    cr = TC.ChanceRef(perms)
    assert cr.G == 4 * T.N_CHOICE and np.all(np.diff(cr.occ_off) == 1)
    R, S, sig = cr.tables()
    rv = cr.iterate(R, S, sig, weights=W)
    roots = []
    for d, perm in enumerate(perms):
        ref = TC.ref_of(perm)
        tabs = ref.tables()
        roots.append(ref.iterate(*tabs, weights=W))
        for mine, theirs in zip((R, S, sig), tabs):
            assert np.array_equal(mine[cr.map[d]], theirs), d
    assert np.array_equal(rv, (((roots[0] + roots[1]) + roots[2]) + roots[3]) / 4.0)


def test_index_of_the_swap_set(deals):
    from scopa_amd.algorithms.team_chance import packet_deals
    perms = packet_deals(PACKETS, fix_seat0=True)[:2]
    assert np.array_equal(perms[0, :8], perms[1, :8]) and np.array_equal(perms[0, 8:12], perms[1, 12:]) and np.array_equal(perms[0, 12:], perms[1, 8:12])
    cr = TC.ChanceRef(perms)
    cnt = np.diff(cr.occ_off)
    assert np.all(cnt[cr.depth <= 1] == 2) and cr.depth_off[2] == 5          # seats 0 and 1 cannot tell the two deals apart
    assert np.all(cnt[cr.depth >= 2] == 1)                                    # seats 2 and 3 see their own hand; later the history names the deal
    assert cr.G == 2 * T.N_CHOICE - 5 and cr.occ_off[-1] == 2 * T.N_CHOICE
    assert np.all(np.diff(cr.gkey.astype(np.uint64)) > 0)
    for g in range(5):
        o = cr.occ[cr.occ_off[g]:cr.occ_off[g + 1]]
        assert np.all(np.diff(o) > 0) and np.all(cr.map.reshape(-1)[o] == g)
    inner = np.ones(len(cr.occ), bool)
    inner[cr.occ_off[1:-1]] = False                                           # positions that start a new row's list
    assert np.all((np.diff(cr.occ) > 0)[inner[1:]])
    assert np.array_equal(np.sort(cr.occ), np.arange(2 * T.N_CHOICE))


def test_key_of_against_the_index(sl, deals):
    from scopa_amd.algorithms.team_chance import key_of, make_key
    perms = deals[[0, 7, 23]]
    cr = TC.ChanceRef(perms)
    rng = np.random.default_rng(5)
    for deal, perm in enumerate(perms):
        for _ in range(20):
            s, path = sl.TeamState(perm=perm), []
            for d in range(12):
                key = key_of(s)
                assert key == int(cr.gkey[cr.map[deal, T.OFFSET[d] + T.path_index(path)]])
                assert key == make_key(d, perm[4 * (d & 3):4 * (d & 3) + 4], s.history()) == TC.make_key(d, perm[4 * (d & 3):4 * (d & 3) + 4], s.history())
                c = int(rng.integers(T.branch(d)))
                path.append(c)
                s.step(s.legal()[c])
            with pytest.raises(ValueError):
                key_of(s)


def test_best_response_is_at_least_the_value(deals):
    from scopa_amd.algorithms.team_chance import packet_deals
    cr = TC.ChanceRef(packet_deals(PACKETS, fix_seat0=True)[:3])
    rng = np.random.default_rng(11)
    pol = rng.random((cr.G, 4)) * (np.arange(4)[None, :] < cr.nleg[:, None])
    pol /= pol.sum(1, keepdims=True)
    for p in (pol, cr.average_policy(np.zeros((cr.G, 4)))):
        out, brs, per_deal = cr.exploitability(p)
        assert out[1] >= out[3] and out[2] >= -out[3] and out[0] >= 0.0
        for t, br in enumerate(brs):                                          # following the returned table reproduces the best response
            v, _ = cr.value_pass(br, None)
            assert cr.mean(v if t == 0 else -v) == out[1 + t]


def test_packet_deals_contract():
    from scopa_amd.algorithms.team_chance import packet_deals
    all24, six = packet_deals(PACKETS), packet_deals(PACKETS, fix_seat0=True)
    assert all24.shape == (24, 16) and six.shape == (6, 16) and len({bytes(d) for d in all24}) == 24
    assert all(sorted(d) == list(range(16)) for d in all24) and np.array_equal(six, all24[:6]) and np.all(six[:, :4] == PACKETS[0])
    for bad in ([[0, 1, 2, 3]] * 4, [[3, 2, 1, 0], [4, 5, 6, 7], [8, 9, 10, 11], [12, 13, 14, 15]], PACKETS[:3]):
        with pytest.raises(ValueError):
            packet_deals(bad)


def test_entry_points_are_declared_bound_and_exported(sl):
    names = ["create", "destroy", "debug_image_budget", "counts", "index_get", "tables_reset", "tables_get", "tables_set", "sigma_get", "cfr_iterate", "cfr_launch", "exploitability",
             "policy_for_deal"]
    hdr = open(os.path.join(ROOT, "include", "scopa.h")).read()
    L = sl.lib()
    for n in names:
        sym = "scopa_team_chance_" + n
        assert re.search(r"\b" + sym + r"\s*\(", hdr), f"{sym} is not declared"
        assert sym in sl.SYMBOLS and hasattr(L, sym) and getattr(L, sym).argtypes is not None, sym
    for m in ("index", "tables_get", "tables_set", "tables_reset", "cfr_iterate", "exploitability", "policy_for_deal"):
        assert callable(getattr(sl.TeamChanceGame, m))
    import scopa_amd.algorithms as A
    for f in ("solve", "packet_deals", "key_of", "policy_by_key"):
        assert callable(getattr(A.team_chance, f))
