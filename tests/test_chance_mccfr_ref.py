"""The restatement of the chance game's MCCFR iteration (tests/chance_mccfr_ref.py) against the C oracle, and the CPU-side checks of the new entry
points: declared, bound and reachable from Python, NULL handle refused (no GPU needed).

One deal: the regret table is oracle.Tree.mccfr_batched's bit for bit.  The strategy table cannot be: the oracle adds sigma once per traverser visit
(c additions per cell and iteration), the iteration under test -- like every batched MCCFR kernel here -- adds visits * sigma, one product and one
sum.  Measured on the seed-42 deal, 3 iterations at batch 48: 58 of 2 952 cells differ, by at most 9 ulp.  So the strategy table is held twice: the
oracle's bits must come out when the restatement's single product is replaced by the c-fold sum (np.array_equal), and the restatement itself must lie
within the rounding bound of those sums, (additions + 2 per iteration) * 2^-53 * S."""
import ctypes as C
import inspect
import os
import re

import numpy as np

import mccfr_edges as E
import philox_words as W
from chance_mccfr_ref import PAIR_VISITS, WORD_BATCH, WORD_LIST, ChanceMccfrRef
from conftest import ROOT


def _perm(h0, h1):
    return h0 + h1 + [c for c in range(16) if c not in h0 + h1]


def _repeated_sum(sig, visits):
    """sig added visits times from 0.0, per row (the oracle's d_strat)"""
    out = np.zeros_like(sig)
    for c in range(1, int(visits.max()) + 1):
        out = np.where((visits >= c)[:, None], out + sig, out)
    return out


def test_one_deal_is_the_oracles_batched_mccfr(oracle):
    t = oracle.Tree(seed=42)
    ref = ChanceMccfrRef([t])
    mp = ref.map[0, :t.n_infosets]
    Rg, Sg = ref.tables()
    S_rep, adds, vis = np.zeros_like(Sg), np.zeros(ref.G), [0, 0]
    for it in range(3):
        sig = E.reference_sigma(Rg, ref.nlegal)
        _, visits, touched, v = ref.iterate(Rg, Sg, 48, 321, it)
        assert touched.all() and visits.sum() == 2 * 86 * 48 and v == (463 * 48, 240 * 48)     # 1 + 5 + 20 + 60 traverser nodes per traversal
        S_rep = S_rep + _repeated_sum(sig, visits)
        adds += visits + 2
        vis = [vis[0] + v[0], vis[1] + v[1]]
    R, S, _ = t.tables()
    assert t.mccfr_batched(R, S, 321, 0, 3, 48) == vis[0] == 3 * 48 * PAIR_VISITS[0] and vis[1] == 3 * 48 * PAIR_VISITS[1]
    assert np.abs(R).max() > 0 and np.array_equal(Rg[mp], R)
    assert np.array_equal(S_rep[mp], S)
    assert (np.abs(Sg[mp] - S) <= (adds[mp] * E.EPS)[:, None] * S).all() and S.max() > 48


def test_one_deal_twice_is_one_deal_at_twice_the_ids(oracle):
    """deal 1 of [t, t] draws ids [B, 2B): together the two copies are one deal walked with ids [0, 2B) from the same frozen table"""
    B, seed, it = 40, 99, 3
    t = oracle.Tree(seed=42)
    two, one = ChanceMccfrRef([t, t]), ChanceMccfrRef([t])
    assert two.G == one.G and np.array_equal(two.map[0], two.map[1])
    R0 = E.edge_table("small_large", one.nlegal)
    S0 = np.arange(one.G * 4, dtype=np.float64).reshape(-1, 4) * one.legal
    R2, S2 = R0.copy(), S0.copy()
    A2, visits2, touched2, vis2 = two.iterate(R2, S2, B, seed, it)
    mp = one.map[0, :t.n_infosets]
    dR, dS, dA, dv, tv = t.mccfr_batched_delta_abs(R0[mp], seed, it, 0, 2 * B)
    assert vis2 == (dv, tv) == (2 * B * PAIR_VISITS[0], 2 * B * PAIR_VISITS[1])
    assert np.array_equal(visits2[mp], np.rint(dS.sum(1))) and touched2.all()
    assert np.array_equal(S2[mp], S0[mp] + np.rint(dS.sum(1))[:, None] * E.reference_sigma(R0[mp], one.nlegal[mp]))
    # the regret increments are the same terms summed as (first B) + (second B) instead of one after the other: the oracle's reorder budget
    dR2, A2b, _, _, _ = two.deltas(R0, B, seed, it)
    assert np.array_equal(A2b, A2) and np.array_equal(R2, np.where(two.legal, R0 + dR2, R0))
    assert np.abs(dR).max() > 0 and E.row_errors(dR2[mp], dR, dA).max() <= E.K_REORDER
    assert np.abs(A2[mp] - dA).max() <= 1e-12 * dA.max()
    # and the two copies do not draw the same traversals
    a = t.mccfr_batched_delta(R0[mp], seed, it, 0, B)[0]
    b = t.mccfr_batched_delta(R0[mp], seed, it, B, B)[0]
    assert not np.array_equal(a, b)


def test_a_listed_subset_leaves_the_other_rows_bits(oracle):
    six = np.array([_perm([0, 5, 10, 15], h) for h in ([1, 2, 3, 4], [1, 2, 3, 6], [1, 2, 7, 6], [9, 8, 7, 6])] +
                   [_perm([0, 5, 10, 14], h) for h in ([1, 2, 3, 4], [9, 8, 7, 6])], np.uint8)
    ref = ChanceMccfrRef([oracle.Tree(perm=p) for p in six])
    assert (ref.G, ref.ref.n_occ) == (3522, 3860)
    deals = [4, 0, 3]
    listed = ref.listed_rows(deals)
    assert listed.any() and (~listed).any() and (ref.ref.count[listed] > 1).any()
    R0 = E.edge_table("onehot", ref.nlegal)
    S0 = (1.0 + np.arange(ref.G * 4, dtype=np.float64).reshape(-1, 4)) * ref.legal
    R, S = R0.copy(), S0.copy()
    A, visits, touched, vis = ref.iterate(R, S, 37, 5, 2, deals)
    assert np.array_equal(touched, listed) and vis == (3 * 37 * PAIR_VISITS[0], 3 * 37 * PAIR_VISITS[1])
    assert np.array_equal(R[~listed].view(np.uint64), R0[~listed].view(np.uint64)) and np.array_equal(S[~listed].view(np.uint64), S0[~listed].view(np.uint64))
    assert not visits[~listed].any() and not A[~listed].any()
    assert (R[listed] != R0[listed]).any() and (S[listed] != S0[listed]).any()
    # the list's order changes nothing, and a deal's draws do not depend on who else is listed
    Rb, Sb = R0.copy(), S0.copy()
    ref.iterate(Rb, Sb, 37, 5, 2, sorted(deals))
    assert np.array_equal(Rb, R) and np.array_equal(Sb, S)
    Rc, Sc = R0.copy(), S0.copy()
    ref.iterate(Rc, Sc, 37, 5, 2, [3])
    only3 = ref.listed_rows([3]) & ~ref.listed_rows([0, 4])
    assert only3.any() and np.array_equal(Rc[only3], R[only3]) and np.array_equal(Sc[only3], S[only3])


# ---- the wide seed of tests/test_gpu_chance_mccfr.py ------------------------------------------------------------------------------------------
def test_the_oracles_uniforms_at_wide_words_are_numpy_philox(oracle):
    """this restatement draws through the C oracle: its og_philox_uniform under a 64-bit seed and 32-bit counter words against the numpy Philox of
    tests/team_mccfr_ref.py, word for word -- two implementations that share no code"""
    import team_mccfr_ref as M
    for seed in (W.WIDE_SEED, W.WIDE_SEED & W.M32, 0xC4A9CE):
        for c in ((0, 0, 0, 0), (7, 5, 1, 1), (85, 4, W.ITER_B31, 0), (3, W.M32, W.ITER_HI, 1), (W.M32, W.ITER_B31, 7, W.M32)):
            o = [int(x) for x in M.philox4x32_10(*c, seed)]
            assert oracle.philox_uniform(seed, *c) == ((o[0] >> 5) * 67108864.0 + (o[1] >> 6)) / 9007199254740992.0, (hex(seed), c)


def test_wide_seed_iterations_separate(oracle):
    """a condition on the GPU test's inputs: at each of its two iterations from reset tables, the visit counts -- which it compares exactly, through
    the strategy sums -- are not those of the seed's low 32 bits"""
    six = np.array([_perm([0, 5, 10, 15], h) for h in ([1, 2, 3, 4], [1, 2, 3, 6], [1, 2, 7, 6], [9, 8, 7, 6])] +
                   [_perm([0, 5, 10, 14], h) for h in ([1, 2, 3, 4], [9, 8, 7, 6])], np.uint8)
    ref = ChanceMccfrRef([oracle.Tree(perm=p) for p in six])
    R0, _ = ref.tables()
    for it, deals in enumerate((None, WORD_LIST)):
        want = ref.deltas(R0, WORD_BATCH, W.WIDE_SEED, it, deals)[2]
        assert want.sum() == 2 * 86 * WORD_BATCH * (6 if deals is None else len(deals))
        assert not np.array_equal(ref.deltas(R0, WORD_BATCH, W.WIDE_SEED & W.M32, it, deals)[2], want)


# ---- header and bindings ------------------------------------------------------------------------------------------------------------------
def _declared_args(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scopa.h")).read(), flags=re.S)
    m = re.search(r"int32_t\s+" + name + r"\s*\(([^;]*)\);", hdr)
    assert m is not None, name
    return [a.split()[-1].lstrip("*") for a in m.group(1).split(",")]


def test_header_declares_both_entry_points():
    assert _declared_args("scopa_chance_mccfr_iterate") == ["g", "n_iters", "batch", "seed", "m", "h_deals"]
    assert _declared_args("scopa_chance_mccfr_counters") == ["g", "decision_visits", "terminal_visits", "iteration"]


def test_library_binds_both_entry_points(sl):
    L = sl.lib()
    assert "scopa_chance_mccfr_iterate" in sl.SYMBOLS and "scopa_chance_mccfr_counters" in sl.SYMBOLS
    assert L.scopa_chance_mccfr_iterate.argtypes == [C.c_void_p, C.c_int32, C.c_uint32, C.c_uint64, C.c_int32, C.c_void_p]
    assert L.scopa_chance_mccfr_counters.argtypes == [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    assert L.scopa_chance_mccfr_iterate.restype == L.scopa_chance_mccfr_counters.restype == C.c_int32


def test_python_layer_exposes_the_solver(sl):
    from scopa_amd import algorithms
    from scopa_amd.algorithms import chance
    p = inspect.signature(sl.ChanceGame.mccfr_iterate).parameters
    assert list(p) == ["self", "batch", "n_iters", "seed", "deals"] and (p["n_iters"].default, p["seed"].default, p["deals"].default) == (1, 0, None)
    assert callable(getattr(sl.ChanceGame, "mccfr_counters", None))
    p = inspect.signature(chance.solve_mccfr).parameters
    assert list(p) == ["multi", "batch", "eps", "max_iters", "check_every", "sample", "seed"] and p["sample"].default is None and p["eps"].default == 1e-3
    assert algorithms.solve_mccfr is chance.solve_mccfr and "solve_mccfr" in algorithms.__all__


def test_null_handle_is_refused_without_a_gpu(sl):
    L = sl.lib()
    assert L.scopa_chance_mccfr_iterate(None, 1, 48, 0, 0, None) == sl.SCOPA_EINVAL
    assert L.scopa_chance_mccfr_iterate(None, 0, 0, 0, 0, None) == sl.SCOPA_EINVAL
    assert L.scopa_chance_mccfr_counters(None, None, None, None) == sl.SCOPA_EINVAL
