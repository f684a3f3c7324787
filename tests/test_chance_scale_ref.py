"""CPU checks behind tests/test_gpu_chance_scale.py that need no GPU: the measured figures of the deal sets of tests/chance_sets.py (set sizes,
infoset counts, multiplicities), asserted on ChanceRef so that the GPU tests on these sets cannot pass vacuously; the deal-sampled restatement with
every deal listed against ChanceRef.run bit for bit at multiplicities up to 8 and from an edge table; and the preconditions of the sampled lists the
GPU test draws on the 495 hidden-hand deals at the benchmark's sizes."""
import time

import numpy as np
import pytest

import cfr_edges as E
import chance_sets as CS


@pytest.mark.parametrize("name", ["BOTH25", "HIDDEN70", "HIDDEN495"])
def test_measured_figures(oracle, name):
    t0 = time.perf_counter()
    r = CS.ref(oracle, name)
    print(f"{name}: reference built in {time.perf_counter() - t0:.1f} s (0 if cached); G = {r.G}, occurrences = {r.n_occ}, I = {min(r.I)} .. {max(r.I)}, "
          f"largest multiplicity per seat = {CS.max_multiplicity(r)}")
    CS.check_figures(r, name)
    assert len(CS.perms(name)) == r.n and len({bytes(p) for p in CS.perms(name)}) == r.n
    if name == "BOTH25":
        assert CS.histogram(r) == CS.BOTH25_HISTOGRAM
        assert r.shared_hand_sizes(0) == [1, 2, 3, 4] and r.shared_hand_sizes(1) == [1, 2, 3, 4]
    else:
        root = np.flatnonzero(r.count == r.n)                       # seat 0's first decision: one row in every deal
        assert root.size == 1 and r.player[root[0]] == 0 and r.nlegal[root[0]] == 4 and (r.map[:, 0] == root[0]).all()


@pytest.mark.parametrize("alternating", [False, True])
def test_every_deal_listed_is_the_full_iteration_on_both25(oracle, alternating):
    r = CS.ref(oracle, "BOTH25")
    assert CS.histogram(r) == CS.BOTH25_HISTOGRAM
    R0, S0 = E.regret_table("small_large", r.nlegal), E.strategy_sum_table("subnormal_rows", r.nlegal)
    w = np.tile([1.0, 0.5, 0.75], (2, 1))
    R, S = r.run(R0.copy(), S0.copy(), w, alternating)
    assert (R != R0).any() and (S != S0).any()
    rng = np.random.Generator(np.random.Philox(key=[5, 2]))
    for lists in ([np.arange(25)] * 2, [np.arange(25)[::-1]] * 2, [rng.permutation(25) for _ in range(2)]):
        Rs, Ss = r.run_sampled(R0.copy(), S0.copy(), lists, w, alternating)
        assert E.same_bits(Rs, R) and E.same_bits(Ss, S)


@pytest.mark.parametrize("m", CS.SAMPLE_SIZES)
def test_sampled_lists_on_the_495_deals(oracle, m):
    r = CS.ref(oracle, "HIDDEN495")
    CS.check_figures(r, "HIDDEN495")
    lists = CS.sampled_lists(m)
    assert lists.shape == (CS.SAMPLE_ITERS, m) and (np.diff(lists, axis=1) > 0).all() and (lists != np.arange(m)).any()
    root = int(np.flatnonzero(r.count == 495)[0])
    unsampled_shared = 0
    for deals in lists:
        total, sampled, first_sampled = r.occurrence_stats(deals)
        assert total[root] == 495 and sampled[root] == m                                     # some but not all of its occurrences
        assert (~first_sampled & (sampled > 0)).any()                                         # an unsampled first occurrence, a sampled later one
        unsampled_shared += int(((total > 1) & (sampled == 0)).sum())
    assert unsampled_shared > 0                                                               # a shared row that an iteration leaves out
    assert CS.check_sampled_lists(r, lists)
