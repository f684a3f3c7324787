"""CPU checks of the Team MiniScopa sampling solver's yardstick: the restatement (tests/team_mccfr_ref.py) against the reference's own
MCCFRTrainer._sample run on TPIMiniScopaGame (tests/golden/team_mccfr.npz, written by tests/tools/gen_team_mccfr_golden.py); the batched definition
tied to the sequential one; the closed-form counts; and the new entry points' presence in the header, the binding and the library."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import philox_words as W
import team_cfr_ref as T
import team_mccfr_ref as M

CASES = ["s42_d4", "s7_d4", "s42_root"]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def case_stream(g, case):
    """the uniforms the reference consumed: stored whole, or regenerated from the recorded np.random.seed and pinned by their count, head and tail"""
    n, kept = int(g[case + "_n_draws"]), g[case + "_uniforms"]
    if kept.size == n:
        return kept
    u = np.random.RandomState(int(g[case + "_case"][1])).random_sample(n)
    assert same_bits(np.concatenate([u[:8], u[-8:]]), kept)
    return u


@pytest.mark.parametrize("case", CASES)
def test_replay_equals_the_reference_bit_for_bit(oracle, golden, case):
    """the reference's dict after its _sample calls: which choice and forced nodes exist, every regret_sum and strategy_sum (opponent and forced nodes
    included), and the number of np.random.choice draws"""
    g = golden.npz("team_mccfr.npz")
    seed, _, n_iters = (int(x) for x in g[case + "_case"][:3])
    path = tuple(int(x) for x in g[case + "_case"][3:])
    mc = M.MCRef(oracle.deal_py_seed(seed), path)
    u, st, upos = case_stream(g, case), mc.state(), 0
    for _ in range(n_iters):
        upos = mc.iteration(st, u, upos)
    assert upos == int(g[case + "_n_draws"]) == n_iters * sum(mc.draws) == n_iters * sum(M.closed_form_visits(p, len(path)) for p in (0, 1))
    rows, forced = g[case + "_rows"].astype(np.int64), g[case + "_forced"].astype(np.int64)
    assert np.array_equal(np.sort(rows), np.nonzero(st.seen)[0])
    assert same_bits(st.R[rows], g[case + "_regret"]) and same_bits(st.S[rows], g[case + "_strategy"])
    depth = np.searchsorted(np.array([mc.ref.off[d] for d in range(mc.d0, 12)]), rows, side="right") - 1 + mc.d0
    assert np.array_equal(T.team_of(depth), g[case + "_team"])
    arrived = np.nonzero((st.lv[0] + st.lv[1]) > 0)[0]
    assert forced.shape[0] == 4 * arrived.size == mc.n_visited(st) - rows.size
    assert np.array_equal(np.unique(forced[:, 0]), arrived) and np.array_equal(T.team_of(forced[:, 1]), g[case + "_forced_team"])
    assert not g[case + "_forced_regret"].any()
    assert same_bits([mc.forced_strategy(st, int(leaf), int(d)) for leaf, d in forced], g[case + "_forced_strategy"])
    # what the replay maintains besides: local_strategy of the updated rows is regret matching of their regrets
    upd = np.nonzero(st.S.any(1))[0]
    for d in range(mc.d0, 12):
        r = upd[(upd >= mc.ref.off[d]) & (upd < mc.ref.off[d] + mc.ref.width[d])]
        assert same_bits(st.L[r], T.Ref.sigma(st.R[r], T.branch(d)))


def test_full_tree_counts_are_the_reference_s(golden):
    g = golden.npz("team_mccfr.npz")
    assert [M.closed_form_visits(p) for p in (0, 1)] == [49381, 20583] == [M.draws_per_traversal(p) for p in (0, 1)]
    assert int(g["s42_root_n_draws"]) == 69964
    for p, (inst, mine) in enumerate([(9781, 1731), (2583, 1731)]):
        iw, ioff = M.shape(p)
        assert ioff[12] == inst and iw[12] == 3600 and sum(iw[d] for d in range(12) if T.team_of(d) == p) == mine


@pytest.mark.parametrize("table", ["zero", "onehot", "small_large"])
def test_batch_of_one_is_a_frozen_replay_of_the_same_choices(oracle, table):
    """the batched definition at batch = 1, its own Philox draws fed back as the uniform stream of the sequential form on a frozen table: the same
    increments bit for bit, the same visit counts, marks and arrivals"""
    import mccfr_edges as E
    mc = M.MCRef(oracle.deal_py_seed(42), (2, 0, 3, 1))
    n_legal = np.concatenate([np.full(mc.ref.width[d], T.branch(d)) for d in range(mc.d0, 12)])
    st = mc.state()
    if table != "zero":
        st.R[:] = E.edge_table(table, n_legal)
    seed, it, tid = 0x5C09A, 3, 17
    a, b = st.copy(), st.copy()
    dR, cnt, A = mc.delta(st.R, a, seed, it, tid, 1)
    dR2, cnt2 = np.zeros_like(dR), np.zeros_like(cnt)
    for p in (0, 1):
        U = mc.uniforms(p, [tid], seed, it)
        order = mc.stream_order(p)
        assert len(order) == mc.draws[p]
        stream = np.array([U[d][0, inst] if d >= 0 else 0.5 for d, inst in order])
        upos, d1, c1 = mc.replay(b, p, stream, 0, frozen=st.R)
        assert upos == mc.draws[p]
        dR2 += d1
        cnt2 += c1
    assert same_bits(dR, dR2) and np.array_equal(cnt, cnt2) and cnt.sum() == 2 * 69
    assert np.array_equal(a.seen, b.seen) and np.array_equal(a.lv, b.lv) and int(a.lv.sum()) == 2 * 144
    assert (A >= np.abs(dR)).all()


def test_fma_dot_against_numpy():
    """np.dot of two short float64 vectors, the reference's v (mc_cfr.py:79), is the fma chain the kernels and the restatement compute"""
    rs = np.random.RandomState(5)
    for n in (2, 3, 4):
        for _ in range(300):
            s, c = rs.random_sample(n), rs.randint(-12, 13, n) * 0.5
            s /= s.sum()
            assert M.dot_fma(s, c) == float(np.dot(s, c))


def test_vectorised_fma_is_exact():
    """the float64 emulation the batched restatement uses against rational arithmetic, on sigmas with entries down to 1e-15 and equal rewards"""
    rs = np.random.RandomState(9)
    for trial in range(6):
        k = 2 + trial % 3
        s = rs.random_sample((1500, k))
        if trial % 3 == 1:
            s[:, 0] *= 1e-15
        if trial % 3 == 2:
            s[:, 1] *= 1e-9
            s[:, 0] = 0.0
        s /= s.sum(1, keepdims=True)
        c = rs.randint(-12, 13, (1500, k)) * 0.5
        if trial >= 3:
            c[:] = c[:, :1]
        assert same_bits(M.dot_fma_vec(s, c), [M.dot_fma(a, b) for a, b in zip(s, c)])


def test_batched_counters_follow_from_the_shape(oracle):
    mc = M.MCRef(oracle.deal_py_seed(7), (0, 1, 2, 3))
    st = mc.state()
    A, cnt = mc.iterate(st, 5, 1, 0)
    assert cnt.sum() == 5 * 2 * 69 and int(st.lv.sum()) == 5 * 2 * 144           # 1 + 4 + 16 + 48 traverser instances, 144 arrivals below a depth-4 root
    assert np.array_equal(st.S.sum(1) > 0, cnt > 0) and (A.sum(1)[cnt == 0] == 0).all()
    assert np.array_equal(st.seen[cnt > 0], np.ones(int((cnt > 0).sum()), np.uint8))


# ---- the wide Philox words of tests/test_gpu_team_mccfr.py ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mc42(oracle):
    return M.MCRef(oracle.deal_py_seed(42))


@pytest.mark.parametrize("seed,iteration,b0", M.WORD_CASES + [M.ITERATE_WORDS], ids=W.case_id)
def test_uniforms_at_wide_words_are_the_oracles(oracle, mc42, seed, iteration, b0):
    """u53 of Philox (instance index, traversal id, iteration, 64 + traverser) under the 64-bit seed, bit for bit the C oracle's og_philox_uniform"""
    ids = W.ids_of(b0, M.WORD_NB)
    for p in (0, 1):
        iw, ioff = M.shape(p)
        U = mc42.uniforms(p, ids, seed, iteration)
        for d in range(12):
            for j in sorted({0, iw[d] // 2, iw[d] - 1}):
                for i, b in enumerate(ids):
                    assert U[d][i, j] == oracle.philox_uniform(seed, ioff[d] + j, b, iteration, M.PHILOX_TAG + p), (p, d, j, b)


@pytest.mark.parametrize("table", M.WORD_TABLES)
@pytest.mark.parametrize("seed,iteration,b0", M.WORD_CASES + [M.ITERATE_WORDS], ids=W.case_id)
def test_wide_word_expectations_separate(mc42, table, seed, iteration, b0):
    """a condition on the GPU tests' inputs: what they compare exactly -- the count column, seen, leaf_visits -- differs from the same quantities with
    the seed, the iteration or the traversal ids narrowed (tests/philox_words.py), so a kernel that lost a word cannot pass"""
    R0 = M.word_start(table)

    def exact(s, it, ids):
        st = mc42.state()
        _, cnt, _ = mc42.delta_ids(R0, st, s, it, ids)
        return cnt, st.seen, st.lv

    want = exact(seed, iteration, W.ids_of(b0, M.WORD_NB))
    assert want[0].sum() == M.WORD_NB * 2 * 1731 and int(want[2].sum()) == M.WORD_NB * 2 * 3600
    variants = W.narrowed(seed, iteration, b0, M.WORD_NB)
    assert variants
    for what, s, it, ids in variants:
        got = exact(s, it, ids)
        assert not np.array_equal(got[0], want[0]) and not np.array_equal(got[1], want[1]) and not np.array_equal(got[2], want[2]), what


def test_header_binding_and_library_agree():
    hdr = open(os.path.join(ROOT, "include", "scopa.h")).read()
    declared = set(re.findall(r"\b(scopa_team_mccfr_[a-z_]+)\s*\(", hdr))
    assert declared == {"scopa_team_mccfr_" + n for n in ("replay", "traverse", "apply", "iterate", "counters", "delta_get", "visits_get")}
    import scopa_amd._lib as sl
    assert declared <= set(sl.SYMBOLS)
    L = sl.lib()
    for name in declared:
        assert hasattr(L, name)
    assert sl.TEAM_MCCFR_DRAWS == (49381, 20583)
