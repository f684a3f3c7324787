"""CPU checks of the restatement of Team MiniScopa over a set of deals (tests/team_chance_ref.py) against tests/team_cfr_ref.py's Ref, of the index
it builds, of algorithms.team_chance's key helpers, and of the entry points' declaration, binding and export.  The packet deals share rows at depths 0
and 1 only; the sets of tests/team_chance_sets.py (both4, reordered, hidden6) share rows at every depth, and the second half of this file pins the
restatement on them: the index, the key's partition, the sweep and the reduce, the summation order, the best response across deals."""
import os
import re

import numpy as np
import pytest

import team_cfr_ref as T
import team_chance_ref as TC
import team_chance_sets as TS
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
    """the packet deals' sharing ends at depth 1: the first card played names the deal.  Rows with several occurrences at depths 2..11 -- the reduce
    on the subtree kernel's rows, the best response's choice below depth 1 -- are covered by the sets of tests/team_chance_sets.py
    (test_index_of_the_deep_sharing_sets and what follows it)"""
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


# ---- deal sets that share rows below depth 1 (tests/team_chance_sets.py) ------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def deep(oracle):
    """name -> the set's ChanceRef, built once per process"""
    return TS.chance_ref


@pytest.mark.parametrize("name", TS.NAMES)
def test_index_of_the_deep_sharing_sets(deep, name):
    cr = deep(name)
    n = cr.n
    assert cr.G == TS.ROWS[name] and cr.occ_off[-1] == n * T.N_CHOICE
    tab = TS.occurrence_table(cr)
    print(name, tab)
    if name == "both4":
        assert tab[5] == {1: 1920, 2: 576} and tab[11] == {1: 622080, 2: 20736}
        assert all(tab[d].get(2, 0) > 0 for d in range(12))                   # both teams own shared rows at every depth
    elif name == "reordered":
        for d in range(12):                                                   # seat 0 (depths 0, 4, 8): the hand's order refines the key
            assert tab[d] == ({1: 2 * T.WIDTH[d]} if d & 3 == 0 else {2: T.WIDTH[d]}), d
        assert not np.array_equal(cr.map[0], cr.map[1])                       # the shared rows are reached through a map that permutes local rows
        shared = np.diff(cr.occ_off)[cr.map[0]] == 2
        assert np.count_nonzero(cr.map[0][shared] != cr.map[1][shared]) > 1000
    else:
        assert tab[4] == {2: 192, 3: 256, 6: 64} and tab[8] == {1: 38016, 2: 27648, 3: 9216, 6: 576} and tab[10] == {1: 290304, 2: 82944, 3: 13824}
        assert all(tab[d] == {1: n * T.WIDTH[d]} for d in range(1, 12, 2))
    # the occurrence lists: a partition of all (deal, row), ascending within every row's list, each naming its own row
    assert np.all(np.diff(cr.gkey.astype(np.uint64)) > 0)
    inner = np.ones(len(cr.occ), bool)
    inner[cr.occ_off[1:-1]] = False                                           # positions that start a new row's list
    assert np.all((np.diff(cr.occ) > 0)[inner[1:]])
    assert np.array_equal(np.sort(cr.occ), np.arange(n * T.N_CHOICE))
    assert np.array_equal(cr.map.reshape(-1)[cr.occ], np.repeat(np.arange(cr.G), np.diff(cr.occ_off)))


def random_walks(sl, perms, n_paths, seed):
    """random paths of deal 0, each replayed card by card in the other deals for as long as the card is legal there
    -> [(deal, depth, seat, infoset string of the acting team, key)] of every node met, duplicates included"""
    from scopa_amd.algorithms.team_chance import key_of
    rng = np.random.default_rng(seed)
    met = []
    for _ in range(n_paths):
        s, cards = sl.TeamState(perm=perms[0]), []
        for d in range(12):
            met.append((0, d, d & 3, s.infoset_string(s.current_player()), key_of(s)))
            cards.append(s.legal()[int(rng.integers(T.branch(d)))])
            s.step(cards[-1])
        for deal in range(1, len(perms)):
            s = sl.TeamState(perm=perms[deal])
            for d in range(12):
                met.append((deal, d, d & 3, s.infoset_string(s.current_player()), key_of(s)))
                if cards[d] not in s.legal():
                    break
                s.step(cards[d])
    return met


def test_key_partition_is_the_information_state_partition(sl, deep):
    """independently of the index code: over the nodes of random paths played in every deal of both4, the reference's information-state string of the
    acting team and the key name the same classes; the key places every node in the row the index gives it"""
    cr = deep("both4")
    met = random_walks(sl, TS.deal_set("both4"), 240, 17)
    by_string, by_key, deals_of = {}, {}, {}
    for deal, d, seat, string, key in met:
        assert by_string.setdefault(string, key) == key and by_key.setdefault(key, string) == string, (deal, d, string)
        deals_of.setdefault(key, set()).add(deal)
    assert len(by_string) == len(by_key) > 2000
    deep_shared = [k for k, ds in deals_of.items() if len(ds) > 1 and (k >> 60) >= 5]
    assert len(deep_shared) > 100                                             # the walk did meet classes of several deals far below depth 1
    where = np.searchsorted(cr.gkey, np.array(list(deals_of), np.uint64))
    assert np.array_equal(cr.gkey[where], np.array(list(deals_of), np.uint64))
    cnt = np.diff(cr.occ_off)[where]
    assert all(len(ds) <= c for ds, c in zip(deals_of.values(), cnt.tolist()))


def test_hand_order_refines_the_information_state(sl, deep):
    """reordered: seat 0 holds the same cards in both deals, so its strings coincide, and its keys do not; the other seats' strings and keys both do"""
    met = random_walks(sl, TS.deal_set("reordered"), 200, 23)
    keys_of_string = {}
    for deal, d, seat, string, key in met:
        keys_of_string.setdefault((seat, string), {})[deal] = key
    both = {k: v for k, v in keys_of_string.items() if len(v) == 2}
    assert sum(1 for (seat, _) in both if seat == 0) > 300 and sum(1 for (seat, _) in both if seat != 0) > 1000
    for (seat, string), v in both.items():
        assert (v[0] != v[1]) == (seat == 0), (seat, string)
    by_key = {}
    for deal, d, seat, string, key in met:                                   # a key never joins two strings
        assert by_key.setdefault(key, string) == string


@pytest.mark.parametrize("name", ["both4", "reordered"])
def test_sweep_and_reduce_are_the_one_deal_traversals_added_per_row(deep, name):
    """at most 2 occurrences per row: x + y is order-free, so the traverser's rows are R0 + (the one-deal increments added per global row) bit for bit"""
    cr = deep(name)
    assert np.diff(cr.occ_off).max() == 2
    R0, S0, sig0 = cr.tables()
    cr.iterate(R0, S0, sig0, 2)
    for p in (0, 1):
        R, S, sig = R0.copy(), S0.copy(), sig0.copy()
        root = cr.traverse(R, S, sig, p)
        dR, dS, roots = np.zeros((cr.G, 4)), np.zeros((cr.G, 4)), []
        for d, perm in enumerate(cr.perms):
            ref = TC.ref_of(perm)
            R1, S1, _, Q1 = ref.tables()
            roots.append(ref.traverse(R1, S1, sig0[cr.map[d]].copy(), Q1, p))
            dR[cr.map[d]] = dR[cr.map[d]] + R1                                # the map is injective within a deal
            dS[cr.map[d]] = dS[cr.map[d]] + S1
        mine = cr.team == p
        assert np.array_equal(bits(R[mine]), bits((R0 + dR)[mine])) and np.array_equal(bits(S[mine]), bits((S0 + dS)[mine]))
        assert np.array_equal(bits(sig[mine]), bits(cr.sigma(R0 + dR)[mine]))
        assert not dR[~mine].any() and not dS[~mine].any()
        for a, a0 in ((R, R0), (S, S0), (sig, sig0)):
            assert np.array_equal(bits(a[~mine]), bits(a0[~mine]))
        s = roots[0]
        for v in roots[1:]:
            s = s + v
        assert root == s / float(cr.n)
        shared_deep = mine & (np.diff(cr.occ_off) == 2) & (cr.depth >= 2)
        assert np.count_nonzero(dR[shared_deep]) > 1000                       # the check did run on shared rows below depth 1


def test_reduce_adds_in_ascending_occurrence_order(deep):
    cr = deep("hidden6")
    rows = np.nonzero(np.diff(cr.occ_off) == 6)[0]
    assert rows.size == 1 + 8 + 64 + 192 + 576
    rng = np.random.default_rng(29)
    img = rng.standard_normal((cr.n * T.N_CHOICE, 8))
    got = cr.reduce_rows(img, rows)
    differ = 0
    for k, g in enumerate(rows.tolist()):
        pairs = sorted((d, r) for d in range(cr.n) for r in np.nonzero(cr.map[d] == g)[0].tolist()) if k < 40 else None
        occ = cr.occ[cr.occ_off[g]:cr.occ_off[g + 1]]
        if pairs is not None:                                                 # the list is the row's (deal, row) pairs ascending, found without the index
            assert [d * T.N_CHOICE + r for d, r in pairs] == occ.tolist()
        fwd, bwd = img[occ[0]].copy(), img[occ[-1]].copy()
        for o in occ[1:]:
            fwd = fwd + img[o]
        for o in occ[-2::-1]:
            bwd = bwd + img[o]
        assert np.array_equal(bits(got[k]), bits(fwd))
        differ += int(not np.array_equal(bits(fwd), bits(bwd)))
    print("rows of 6 occurrences whose sum depends on the order:", differ, "of", rows.size)
    assert differ > 0                                                         # otherwise the test says nothing about order


def one_deal_exploitabilities(cr, pol):
    return np.array([TC.ref_of(perm).exploitability(cr.policy_for_deal(pol, d))[0] for d, perm in enumerate(cr.perms)])


@pytest.mark.parametrize("name", ["both4", "hidden6"])
def test_best_response_across_deals_is_below_the_per_deal_best_responses(deep, name):
    """a responder who knows the deal does at least as well as one who does not: the best response across deals is at most the mean of the one-deal
    best responses, and on these sets strictly below it (measured: (BR0 + BR1) / 2 = 3.0232 against 3.2670 on both4, 2.7188 against 3.1020 on hidden6).
    The value of the policy itself is the mean of the one-deal values, exactly"""
    cr = deep(name)
    pol = cr.average_policy(TS.ref_run(name, "cfr+")[1])
    out4, brs, per_deal = cr.exploitability(pol)
    one = one_deal_exploitabilities(cr, pol)
    mean = [cr.mean(one[:, k]) for k in range(4)]
    print(name, "across deals:", out4, "mean of the one-deal values:", mean)
    assert out4[1] <= mean[1] and out4[2] <= mean[2] and out4[0] < mean[0]
    assert out4[3] == mean[3] and np.array_equal(bits(per_deal), bits(one[:, 3]))
    assert out4[1] >= out4[3] and out4[2] >= -out4[3]
    if name == "both4":                                                       # following the returned table reproduces the best response
        for t, br in enumerate(brs):
            v, _ = cr.value_pass(br, None)
            assert cr.mean(v if t == 0 else -v) == out4[1 + t]
