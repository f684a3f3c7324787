"""CPU checks of the deal-sampled restatement (tests/chance_sampled_ref.py) that need no GPU: with every deal listed, in any order, it is
ChanceRef.run bit for bit (np.array_equal), which pins what the GPU kernels are held to (tests/test_gpu_chance_sampled.py) to code that is already
pinned to the C oracle; the skip / first-sampled / +0.0 rules on a list whose preconditions are asserted first; the ordering of exploitabilities of
an orientation run; scopa_amd.algorithms.chance.sample_deals; the entry point's presence in the header and the binding."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from chance_ref import ChanceRef
from chance_sampled_ref import SampledChanceRef


def _perm(h0, h1):
    return h0 + h1 + [c for c in range(16) if c not in h0 + h1]


# the six-deal set of tests/test_gpu_chance.py
SIX = np.array([_perm([0, 5, 10, 15], h) for h in ([1, 2, 3, 4], [1, 2, 3, 6], [1, 2, 7, 6], [9, 8, 7, 6])] +
               [_perm([0, 5, 10, 14], h) for h in ([1, 2, 3, 4], [9, 8, 7, 6])], np.uint8)
WEIGHTINGS = ("vanilla", "cfr+", "dcfr")


def _weights(name, n):
    from scopa_amd.algorithms import schedule
    return schedule(name, 0, n, 1.5, 0.0, 2.0)


@pytest.fixture(scope="module")
def six(oracle):
    trees = [oracle.Tree(perm=p) for p in SIX]
    return ChanceRef(trees), SampledChanceRef(trees)


@pytest.mark.parametrize("alternating", [False, True])
@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_every_deal_listed_is_the_full_iteration(six, weighting, alternating):
    full, ref = six
    w = _weights(weighting, 7)
    R0, S0 = full.run(*full.tables(), w, alternating)
    assert np.abs(R0).max() > 0 and np.abs(S0).max() > 0
    rng = np.random.Generator(np.random.Philox(key=[3, 1]))
    for lists in ([list(range(6))] * 7, [[5, 4, 3, 2, 1, 0]] * 7, [rng.permutation(6) for _ in range(7)]):
        R, S = ref.run_sampled(*ref.tables(), lists, w, alternating)
        assert np.array_equal(R, R0) and np.array_equal(S, S0)


def test_permuting_a_list_changes_nothing(six):
    _, ref = six
    w = _weights("dcfr", 4)
    lists = [[1, 3, 4], [0, 2, 5], [2, 3], [4]]
    shuffled = [[4, 1, 3], [5, 0, 2], [3, 2], [4]]
    for alternating in (False, True):
        Ra, Sa = ref.run_sampled(*ref.tables(), lists, w, alternating)
        Rb, Sb = ref.run_sampled(*ref.tables(), shuffled, w, alternating)
        assert np.abs(Ra).max() > 0 and np.array_equal(Ra, Rb) and np.array_equal(Sa, Sb)


def test_unsampled_occurrences_are_skipped_and_unsampled_rows_discounted(six):
    full, ref = six
    deals = [1, 3, 4]
    total, sampled, first_sampled = ref.occurrence_stats(deals)
    # preconditions, so that nothing below passes vacuously
    assert np.array_equal(total, ref.count) and total.sum() == ref.n_occ
    mixed = (sampled > 0) & (sampled < total)
    late = ~first_sampled & (sampled > 0)
    none = sampled == 0
    assert mixed.any() and late.any() and all((none & (ref.player == p)).any() for p in (0, 1))
    # a start with every cell non-zero: three full iterations, then every zero cell of a legal action set to a value of its own
    R, S = full.run(*full.tables(), _weights("vanilla", 3))
    R[ref.legal & (R == 0.0)] = -0.375
    S[ref.legal & (S == 0.0)] = 0.625
    w = np.array([0.5, 0.25, 0.5])
    R1, S1 = R.copy(), S.copy()
    ref.sweep_sampled(R1, S1, w, None, deals)
    # a row with no sampled occurrence: exactly its former value times the weight
    want_R = np.where(~(R <= 0.0), R * 0.5, R * 0.25)
    assert np.array_equal(R1[none], want_R[none]) and np.array_equal(S1[none], (S * 0.5)[none])
    assert (R1[none & (ref.nlegal == 4)] != 0.0).all() and (S1[none & (ref.nlegal == 4)] != 0.0).all()
    # every other row: the sum over its sampled occurrences alone, in deal order, from the first sampled one, by a loop over single rows
    sig = ref.sigma(R)
    delta = {d: ref.deal_delta(d, sig[ref.map[d, :ref.I[d]]], None) for d in deals}
    checked = 0
    for g in np.concatenate([np.flatnonzero(late)[:40], np.flatnonzero(mixed & ~late)[:40]]):
        dR = dS = None
        for d in sorted(deals):
            for local in np.flatnonzero(ref.map[d, :ref.I[d]] == g):
                dR = delta[d][0][local] if dR is None else dR + delta[d][0][local]
                dS = delta[d][1][local] if dS is None else dS + delta[d][1][local]
        Rn = R[g] + dR
        want = np.where(ref.legal[g], np.where(~(Rn <= 0.0), Rn * 0.5, Rn * 0.25), R[g])
        assert np.array_equal(R1[g], want) and np.array_equal(S1[g], np.where(ref.legal[g], (S[g] + dS) * 0.5, S[g]))
        checked += 1
    assert checked >= 41
    # alternating: the half-sweep of player 0 leaves player 1's rows alone, unsampled or not
    R2, S2 = R.copy(), S.copy()
    ref.sweep_sampled(R2, S2, w, 0, deals)
    p1 = ref.player == 1
    assert np.array_equal(R2[p1], R[p1]) and np.array_equal(S2[p1], S[p1])
    assert np.array_equal(R2[none & ~p1], want_R[none & ~p1]) and np.array_equal(S2[none & ~p1], (S * 0.5)[none & ~p1])


def test_orientation_run_lowers_exploitability(six):
    from scopa_amd.algorithms.chance import sample_deals
    _, ref = six
    lists, w = sample_deals(6, 3, 0, 60, seed=7), _weights("cfr+", 60)
    R, S = ref.tables()
    uniform = ref.exploitability(ref.average_policy(S))[0]
    ref.run_sampled(R, S, lists[:5], w[:5])
    after5 = ref.exploitability(ref.average_policy(S))[0]
    ref.run_sampled(R, S, lists[5:], w[5:])
    after60 = ref.exploitability(ref.average_policy(S))[0]
    print("cfr+ with 3 of 6 deals per iteration: exploitability uniform / after 5 / after 60 =", uniform, after5, after60)
    assert after60 < after5 < uniform


def test_sample_deals():
    from scopa_amd.algorithms.chance import sample_deals
    for n, m in ((6, 3), (495, 32), (7, 7), (5, 1)):
        s = sample_deals(n, m, 0, 10, seed=3)
        assert s.shape == (10, m) and s.dtype == np.int32 and s.min() >= 0 and s.max() < n
        assert (np.diff(s.astype(np.int64), axis=1) > 0).all()                                # ascending, hence distinct
        assert np.array_equal(s[4:], sample_deals(n, m, 4, 6, seed=3))                        # keyed by the absolute iteration
        want = np.sort(np.random.Generator(np.random.Philox(key=[3, 9])).choice(n, m, replace=False))
        assert np.array_equal(s[9], want)
    assert len({tuple(r) for r in sample_deals(495, 32, 0, 10)}) == 10                        # the draws differ between iterations
    assert not np.array_equal(sample_deals(495, 32, 0, 4, seed=1), sample_deals(495, 32, 0, 4, seed=2))
    assert np.array_equal(sample_deals(6, 3, 0, 4), sample_deals(6, 3, 0, 4, seed=0))
    assert sample_deals(6, 3, 5, 0).shape == (0, 3)
    for bad in ((6, 0), (6, 7)):
        with pytest.raises(ValueError):
            sample_deals(*bad, 0, 1)


def test_entry_point_is_declared_and_bound(sl):
    name = "scopa_chance_cfr_iterate_sampled"
    with open(os.path.join(ROOT, "include", "scopa.h")) as f:
        header = f.read()
    assert re.search(r"\b%s\(" % name, header) and name in sl.SYMBOLS and hasattr(sl.lib(), name)
    assert len(getattr(sl.lib(), name).argtypes) == 6
    assert sl.lib().scopa_chance_cfr_iterate_sampled(None, 1, 1, None, None, 0) == sl.SCOPA_EINVAL
    assert hasattr(sl.ChanceGame, "cfr_iterate_sampled")
