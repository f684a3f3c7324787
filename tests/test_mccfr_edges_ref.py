"""The batched MCCFR step on edge-case regret tables, CPU side: the oracle against the REFERENCE, and the oracle against itself.

tests/golden/mccfr_frozen_edges.npz holds what the reference's own MCCFRTrainer._sample accumulates (oracle/gen_golden.py:
gen_mccfr_frozen_edges) on the tables of oracle/mccfr_edges.py: rows with nothing positive (negatives, -0.0), one-hot rows (sigma exactly
0 and 1), 1e-9 next to 1e6, subnormals, |R| ~ 1e12, and a table on which the reference's own importance weights overflow.  The oracle
must reproduce every case bit for bit; the GPU module (tests/test_gpu_mccfr_edges.py) then holds the kernels to the oracle.

The second half measures the REORDER BUDGET the GPU module uses: how far a sum of the same increments in another order may lie from
the oracle's, per infoset row, in units of eps * (sum of |increment| into the row); and checks the DERIVED live-table bound that
tests/test_gpu_multi_mccfr.py holds k_mccfr_multi to (its walks add onto the live regret values, not onto a zeroed delta)."""
import numpy as np
import pytest

import mccfr_edges as E

N_CASES = 6


def _case(oracle, golden, n):
    t = oracle.Tree(seed=42)
    return (t,) + E.edge_case(golden.dir, t.infoset_strings, t.infoset_nlegal, n)


def test_fixture_covers_every_edge_table(golden):
    assert [c["table"] for c in E.edge_cases(golden.dir)] == list(E.EDGE_TABLES) and len(E.EDGE_TABLES) == N_CASES


def test_edge_tables_are_what_they_claim(oracle):
    """The tables hit the branches they are named after, judged by the reference's current_strategy formula in numpy."""
    t = oracle.Tree(seed=42)
    n = t.infoset_nlegal
    legal = np.arange(4)[None, :] < n[:, None]
    sg = {name: E.reference_sigma(E.edge_table(name, n), n) for name in E.EDGE_TABLES}
    uniform = np.where(legal, 1.0 / n[:, None], 0.0)
    R = E.edge_table("allneg", n)
    assert (R[legal] <= 0).all() and np.signbit(R[legal]).all() and (R[legal] == 0).any() and (R[legal] < 0).any()
    assert np.array_equal(sg["allneg"], uniform)
    assert set(np.unique(sg["onehot"])) == {0.0, 1.0} and (sg["onehot"].sum(1) == 1.0).all()
    s = sg["small_large"][legal & (n > 1)[:, None]]
    assert 0 < s.min() < 1e-14 and ((s > 1e-10) & (s < 1e-8)).any()
    # subnormal: 5e-324 / (k * 5e-324) = 1 / k exactly over the k non-zero cells; a flushed denormal would give 1 / n on every row
    R = E.edge_table("subnormal", n)
    k = (R > 0).sum(1)
    assert np.array_equal(sg["subnormal"], np.where(k[:, None] > 0, np.where(R > 0, 1.0 / np.maximum(k, 1)[:, None], 0.0), uniform))
    assert ((k < n) & (k > 0)).sum() > 100
    assert np.abs(E.edge_table("big", n)[legal]).max() > 1e12
    small = E.edge_table("small_large", n)
    nonf = E.edge_table("nonfinite", n)
    assert np.array_equal(nonf == 1e-300, legal & (small < 1.0)) and np.array_equal(nonf[nonf != 1e-300], small[nonf != 1e-300])


@pytest.mark.parametrize("case", range(N_CASES))
def test_batched_mccfr_is_the_references_sample_on_edge_tables(oracle, golden, case):
    """og_mccfr_batched_delta reproduces, BIT FOR BIT, the regret and strategy deltas and the sampled actions of the reference's own
    _sample recursion on every edge table.  `nonfinite`: the same cells are NaN / +inf / -inf as in the reference, the finite ones bit-equal."""
    t, name, R, seed, it, b0, nb, dR, dS, idx, actions = _case(oracle, golden, case)
    oR, oS, dv, tv = t.mccfr_batched_delta(R, seed, it, b0, nb)
    assert (dv, tv) == (463 * nb, 240 * nb)
    assert (name == "nonfinite") == (not np.isfinite(dR).all())
    assert E.same_bits_or_same_nonfinite(oR, dR)
    assert np.array_equal(oS.view(np.uint64), dS.view(np.uint64))
    assert set(np.flatnonzero(oS.sum(1) > 0)) <= set(idx)        # the reference's dict also holds the opponents' infosets
    tr = []
    for b in range(b0, b0 + nb):
        for p in (0, 1):
            nodes, acts = t.mccfr_batched_trace(R, seed, it, b, p)
            tr.extend(int(t.legal[n][a]) for n, a in zip(nodes, acts))
    assert np.array_equal(np.array(tr, np.int8), actions)


def test_nonfinite_case_is_small_and_independent_of_the_order_of_additions(oracle, golden):
    """What the GPU module may mask in the `nonfinite` case -- the cells that are non-finite in the REFERENCE's deltas -- is below 5 % of the
    touched cells, covers NaN, +inf and -inf, and does not depend on the order in which the increments are added: no cell's finite
    increments sum to 1e308 in absolute value, so no partial sum can overflow, and a cell is non-finite only through a non-finite increment
    (inf + -inf and NaN + x are NaN in every order)."""
    t, name, R, seed, it, b0, nb, dR, dS, idx, _ = _case(oracle, golden, E.EDGE_TABLES.index("nonfinite"))
    legal = np.arange(4)[None, :] < t.infoset_nlegal[:, None]
    touched = int((legal & (dS.sum(1) > 0)[:, None]).sum())
    bad = ~np.isfinite(dR)
    print(f"nonfinite: {int(bad.sum())} of {touched} touched cells (NaN {int(np.isnan(dR).sum())}, +inf {int(np.isposinf(dR).sum())}, -inf {int(np.isneginf(dR).sum())})")
    assert 0 < bad.sum() < 0.05 * touched
    assert np.isnan(dR).any() and np.isposinf(dR).any() and np.isneginf(dR).any()
    _, _, A, _, _ = t.mccfr_batched_delta_abs(R, seed, it, b0, nb)
    assert A.max() < 1e308


def _budget_cases():
    for deal in E.DEALS:
        for name in ("zero",) + (E.FINITE_TABLES if deal == 42 else ("onehot", "small_large")):
            yield deal, name, 3000
    for name in E.FINITE_TABLES:                                  # the largest launch of the GPU module
        yield 42, name, 17923


def test_reorder_budget(oracle):
    """The oracle against itself: every finite edge table (and the zero table) on every deal of the GPU module, 3000 pairs computed whole versus
    summed from ragged shards in a shuffled order (plainly, and through 16 partial tables); the seed-42 tables also at the GPU module's
    largest launch.  The largest error seen, in units of eps * A_row, must be what oracle/mccfr_edges.py records (REORDER_MEASURED: not above it,
    not below half of it), from which the GPU module's K_REORDER = 8 x follows.
    (Units of eps * A_row in the hundreds are expected: a row that receives thousands of like-signed increments far below its running sum
    rounds the same way every time, so the error grows with the number of additions, not with its square root.)"""
    worst, trees = {}, {}
    for deal, name, nb in _budget_cases():
        t = trees.setdefault(deal, oracle.Tree(seed=deal))
        R = np.zeros((t.n_infosets, 4)) if name == "zero" else E.edge_table(name, t.infoset_nlegal)
        worst[(deal, name, nb)] = E.reorder_error(t, R, 0xABCDEF12345, 5, 10, nb, np.random.RandomState(deal))
    for k, v in sorted(worst.items(), key=lambda kv: -kv[1])[:8]:
        print(k, f"{v:.1f}")
    top = max(worst.values())
    print(f"largest reorder error: {top:.1f} eps A_row; recorded {E.REORDER_MEASURED}; K_REORDER {E.K_REORDER}")
    assert np.isfinite(top)
    assert E.REORDER_MEASURED / 2 <= top <= E.REORDER_MEASURED
    assert E.K_REORDER == 8 * E.REORDER_MEASURED


def test_live_table_budget(oracle):
    """The oracle against itself on the live table (oracle/mccfr_edges.py:live_table_error): every finite edge table and the zero table on the
    seed-42 and seed-1282 deals at 3000 pairs and on seed 42 at 64 pairs, the shards added straight onto R0.copy().  tol_row is derived, so the
    error may nowhere exceed 1 tol_row; the largest value seen is what the module records (LIVE_MEASURED: not above it, not below half of it)."""
    worst, trees = {}, {}
    for deal, nb in ((42, 3000), (1282, 3000), (42, 64)):
        t = trees.setdefault(deal, oracle.Tree(seed=deal))
        for name in ("zero",) + E.FINITE_TABLES:
            R = np.zeros((t.n_infosets, 4)) if name == "zero" else E.edge_table(name, t.infoset_nlegal)
            worst[(deal, name, nb)] = E.live_table_error(t, R, 0xABCDEF12345, 5, 10, nb, np.random.RandomState(deal))
    for k, v in sorted(worst.items(), key=lambda kv: -kv[1])[:8]:
        print(k, f"{v:.4f}")
    top = max(worst.values())
    print(f"largest live-table error: {top:.4f} tol_row; recorded {E.LIVE_MEASURED}")
    assert np.isfinite(top) and top <= 1.0
    assert E.LIVE_MEASURED / 2 <= top <= E.LIVE_MEASURED <= 1.0


def test_reorder_of_the_nonfinite_case_keeps_its_kinds(oracle, golden):
    """The nonfinite case pair by pair in a shuffled order: the same cells NaN / +inf / -inf, the finite ones within the budget."""
    t, name, R, seed, it, b0, nb, dR, dS, idx, _ = _case(oracle, golden, E.EDGE_TABLES.index("nonfinite"))
    _, _, A, _, _ = t.mccfr_batched_delta_abs(R, seed, it, b0, nb)
    acc = np.zeros_like(dR)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in np.random.RandomState(0).permutation(nb):
            acc += t.mccfr_batched_delta(R, seed, it, b0 + int(b), 1)[0]
    assert np.array_equal(np.isnan(acc), np.isnan(dR)) and np.array_equal(np.isposinf(acc), np.isposinf(dR)) and np.array_equal(np.isneginf(acc), np.isneginf(dR))
    fin = np.isfinite(dR)
    assert E.row_errors(np.where(fin, acc, 0.0), np.where(fin, dR, 0.0), A).max() <= E.K_REORDER
