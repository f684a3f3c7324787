"""Edge-case frozen regret tables for the batched MCCFR step, and the fixture made from them.

TEST INFRASTRUCTURE: shared by oracle/gen_golden.py:gen_mccfr_frozen_edges (which runs the reference's own
MCCFRTrainer._sample on these tables and writes tests/golden/mccfr_frozen_edges.npz) and by the tests
(tests/test_mccfr_edges_ref.py, tests/test_gpu_mccfr_edges.py).  The product package never imports this module.

A table is [n_infosets][4] float64 in the tree's infoset order; slots beyond a row's legal-action count are 0.0.
Every table is a function of (name, n_legal) alone: a fixed np.random.RandomState per name, drawn for all four
slots of every row, so the legal cells of a row do not depend on the other rows' action counts.
"""
import json
import os

import numpy as np

EDGE_TABLES = ("allneg", "onehot", "small_large", "subnormal", "big", "nonfinite")
FINITE_TABLES = EDGE_TABLES[:-1]   # the tables whose deltas are finite in the reference
# np.random.RandomState seeds.  small_large and nonfinite share their draws (nonfinite IS small_large with another small value); 280 was
# picked, among 0..299, on the seed-42 deal with the oracle alone: 16 traversal pairs then already give NaN, +inf and -inf cells from
# single non-finite increments (2 % of the touched cells), while no cell's finite increments sum to more than 1e308 in absolute value --
# so which cells are NaN / +inf / -inf / finite does not depend on the order of the additions.
_RS_SEED = {"allneg": 1, "big": 2, "small_large": 280, "nonfinite": 280}


def edge_table(name, n_legal):
    """The edge table `name` for a deal whose infoset i has n_legal[i] legal actions.

    allneg       -abs(randn): nothing positive, the uniform fallback from a non-zero row.  Every 5th row has -0.0 in its even slots,
                 every 25th row is -0.0 throughout.
    onehot       -1 everywhere, +3 at slot (7 i) mod n: sigma exactly 0 and 1.
    small_large  uniform [0, 1e6) with one legal cell (slot 0; slot i mod n in every 4th row) replaced by 1e-3, 1e-6, 1e-9 in turn by row: sigma of ~1e-9 .. 1e-15
                 next to O(1) entries, importance weights of 1e9 .. 1e30 and beyond.
    subnormal    5e-324 (the smallest subnormal) in the legal cells; every 3rd row has the legal cell (i / 3) mod n at 0.0, so that a
                 flushed denormal (uniform over n) and a kept one (uniform over the n - 1 non-zero cells) differ.
    big          randn * 1e12: magnitudes as after a long run.
    nonfinite    small_large with the small cell at 1e-300: sampling probabilities underflow, weights overflow to inf and
                 inf * 0 = NaN in the reference's own arithmetic."""
    n_legal = np.asarray(n_legal, np.int64)
    I = n_legal.size
    rs = np.random.RandomState(_RS_SEED.get(name, 0))
    rows = np.arange(I)
    legal = np.arange(4)[None, :] < n_legal[:, None]
    if name == "allneg":
        R = -np.abs(rs.randn(I, 4))
        R[(rows % 5 == 0)[:, None] & (np.arange(4) % 2 == 0)[None, :]] = -0.0
        R[rows % 25 == 0] = -0.0
    elif name == "onehot":
        R = np.full((I, 4), -1.0)
        R[rows, (7 * rows) % n_legal] = 3.0
    elif name in ("small_large", "nonfinite"):
        R = rs.random_sample((I, 4)) * 1e6
        small = np.array([1e-3, 1e-6, 1e-9])[rows % 3] if name == "small_large" else np.full(I, 1e-300)
        R[rows, np.where(rows % 4 == 3, rows % n_legal, 0)] = small
    elif name == "subnormal":
        R = np.full((I, 4), 5e-324)
        third = rows % 3 == 0
        R[rows[third], ((rows // 3) % n_legal)[third]] = 0.0
    elif name == "big":
        R = rs.randn(I, 4) * 1e12
    else:
        raise KeyError(name)
    R[~legal] = 0.0
    return np.ascontiguousarray(R)


def reference_sigma(R, n_legal):
    """InfoNode.current_strategy (np.maximum, ndarray.sum, elementwise divide) row by row in numpy float64; padding slots 0."""
    sg = np.zeros_like(R)
    for i, n in enumerate(n_legal):
        pos = np.maximum(R[i, :n], 0)
        sg[i, :n] = np.ones_like(pos) / len(pos) if pos.sum() == 0 else pos / pos.sum()
    return sg


FIXTURE = "mccfr_frozen_edges.npz"


def edge_cases(golden_dir):
    g = np.load(os.path.join(golden_dir, FIXTURE), allow_pickle=False)
    return json.loads(str(g["cases"]))


def edge_case(golden_dir, t_strings, n_legal, n):
    """Case n of tests/golden/mccfr_frozen_edges.npz (the reference's own MCCFRTrainer._sample on an edge table,
    oracle/gen_golden.py:gen_mccfr_frozen_edges) re-indexed by the tree's infoset ids, like conftest.frozen_case for mccfr_frozen.npz.
    The frozen table is rebuilt by edge_table(); the rows the reference actually read are in the fixture and must be those."""
    g = np.load(os.path.join(golden_dir, FIXTURE), allow_pickle=False)
    meta = json.loads(str(g["cases"]))[n]
    I = len(t_strings)
    R = edge_table(meta["table"], n_legal)
    idx = [t_strings.index(k.split("|", 1)[1]) for k in g[f"c{n}_keys"]]
    assert np.array_equal(R[idx].view(np.uint64), g[f"c{n}_regret"].view(np.uint64)), "edge_table() is not the table the fixture was made from"
    dR, dS = np.zeros((I, 4)), np.zeros((I, 4))
    dR[idx], dS[idx] = g[f"c{n}_dregret"], g[f"c{n}_dstrategy"]
    return meta["table"], R, int(meta["seed"]), meta["iteration"], meta["b0"], meta["nb"], dR, dS, idx, g[f"c{n}_actions"]


def same_bits_or_same_nonfinite(a, b):
    """a == b bit for bit where b is finite; where b is NaN / +inf / -inf, a is the same kind (a NaN's payload and sign are not compared)."""
    a, b = np.asarray(a), np.asarray(b)
    fin = np.isfinite(b)
    return bool(np.array_equal(a[fin].view(np.uint64), b[fin].view(np.uint64)) and np.array_equal(np.isnan(a), np.isnan(b))
                and np.array_equal(np.isposinf(a), np.isposinf(b)) and np.array_equal(np.isneginf(a), np.isneginf(b)))


# ---- the reorder budget ------------------------------------------------------------------------------------------------------------
EPS = 2.0 ** -53
# deals of the GPU module (seed -> infosets -> wavefronts per traversal workgroup); tests/test_gpu_mccfr_edges.py explains the choice
DEALS = (282, 42, 40, 2244, 474, 2797, 1789, 1282)


def row_errors(got, want, A):
    """Per infoset row: max over the row's cells of |got - want|, in units of eps * A_row, A_row = the sum of |increment| over everything
    the oracle added into the row (Tree.mccfr_batched_delta_abs).  Rows with A_row = 0 received nothing: there any difference is infinite."""
    A_row = np.asarray(A).sum(1)
    err = np.abs(np.asarray(got) - np.asarray(want)).max(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err == 0.0, 0.0, err / (EPS * A_row))


def reorder_error(t, R, seed, iteration, b0, nb, rs):
    """The oracle against itself: the delta of pairs [b0, b0 + nb) computed whole versus summed from ragged shards in a shuffled order,
    once one shard after the other and once through 16 partial tables (the kernel's group tables).  Returns the largest row error in units
    of eps * A_row."""
    whole, _, A, _, _ = t.mccfr_batched_delta_abs(R, seed, iteration, b0, nb)
    cuts = np.unique(np.concatenate([[0, nb], rs.randint(1, nb, size=min(nb - 1, 96))])) if nb > 1 else np.array([0, nb])
    shards = [t.mccfr_batched_delta(R, seed, iteration, b0 + int(a), int(b - a))[0] for a, b in zip(cuts[:-1], cuts[1:])]
    order = rs.permutation(len(shards))
    seq = np.zeros_like(whole)
    groups = np.zeros((16,) + whole.shape)
    for n, i in enumerate(order):
        seq += shards[i]
        groups[n % 16] += shards[i]
    grp = np.zeros_like(whole)
    for g in groups:
        grp += g
    return max(row_errors(seq, whole, A).max(), row_errors(grp, whole, A).max())


# Measured by tests/test_mccfr_edges_ref.py::test_reorder_budget over every finite edge table and every deal of DEALS (3000 pairs): the
# largest reorder error of the oracle against itself is REORDER_MEASURED x eps x A_row.  The kernel adds in arrival order over 16 group
# tables and up to 1024 lanes, which a shard shuffle only samples: its budget is 8 x that.  Neither number comes from a kernel's output.
REORDER_MEASURED = 3237.0   # seed-42 deal, 17 923 pairs; 3000-pair launches stay below 900
K_REORDER = 8.0 * REORDER_MEASURED


# ---- the live-table budget (k_mccfr_multi) -----------------------------------------------------------------------------------------
# k_mccfr_multi's walks add every increment onto the LIVE regret value in LDS, not onto a zeroed delta table: each addition rounds at the
# magnitude of |R0| + the running sum, so on a row with large |R0| the error does not scale with A_row alone and the reorder budget above
# is the wrong measure.  One iteration from the table R0, derived, not measured:
#   * the kernel makes one addition per traverser visit into each cell of a row, c_row additions per cell (c_row = the row's visit count,
#     rint(dS.sum(1))); every partial sum is at most max|R0_row| + A_row in absolute value (A_row = the sum of |increment| into the row), so
#     each addition errs by at most eps * (max|R0_row| + A_row): c_row * eps * (max|R0_row| + A_row) in all, in any order of the additions;
#   * the oracle's own delta carries at most c_row * eps * A_row from its c_row additions onto zero, and its R0 + dR one more rounding of
#     at most eps * (max|R0_row| + A_row).
# Together (2 c_row + 1) eps (max|R0_row| + A_row) to first order; tol_row rounds that up to 2 (c_row + 1), which also covers the second-order
# terms (c_row <= 2 * pairs: c_row * eps < 1e-9).  A row nobody visited has A_row = 0 and tol_row = 2 eps max|R0_row|: it must come back as it
# was, which the callers assert bit for bit besides.  Nothing here comes from a kernel's output.
def live_table_tol(R0, dS, A):
    """tol_row [I] = 2 (c_row + 1) eps (max|R0_row| + A_row) for one iteration from R0 (dS, A: Tree.mccfr_batched_delta_abs)"""
    c = np.rint(np.asarray(dS).sum(1))
    return 2.0 * (c + 1.0) * EPS * (np.abs(np.asarray(R0)).max(1) + np.asarray(A).sum(1))


def live_row_errors(got, want, tol):
    """Per infoset row: max over the row's cells of |got - want| in units of tol_row (0 where they agree exactly)"""
    err = np.abs(np.asarray(got) - np.asarray(want)).max(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err == 0.0, 0.0, err / tol)


def live_table_error(t, R0, seed, iteration, b0, nb, rs):
    """The oracle against itself, on the live table: R0 + (the delta of pairs [b0, b0 + nb) computed whole) versus the same pairs' ragged shards
    added STRAIGHT ONTO R0.copy() -- in a shuffled order; dealt over 16 queues (the kernel's wavefronts) and taken queue after queue; and
    through 16 partial tables added onto the live table one after the other.  Returns the largest row error in units of tol_row."""
    whole, dS, A, _, _ = t.mccfr_batched_delta_abs(R0, seed, iteration, b0, nb)
    tol = live_table_tol(R0, dS, A)
    cuts = np.unique(np.concatenate([[0, nb], rs.randint(1, nb, size=min(nb - 1, 96))])) if nb > 1 else np.array([0, nb])
    shards = [t.mccfr_batched_delta(R0, seed, iteration, b0 + int(a), int(b - a))[0] for a, b in zip(cuts[:-1], cuts[1:])]
    order = rs.permutation(len(shards))
    seq, queued, parts = R0.copy(), R0.copy(), R0.copy()
    groups = np.zeros((16,) + whole.shape)
    for n, i in enumerate(order):
        seq += shards[i]
        groups[n % 16] += shards[i]
    for q in range(16):
        for i in order[q::16]:
            queued += shards[i]
    for g in groups:
        parts += g
    want = R0 + whole
    return max(live_row_errors(x, want, tol).max() for x in (seq, queued, parts))


# Measured by tests/test_mccfr_edges_ref.py::test_live_table_budget over every finite edge table and the zero table (seed-42 and seed-1282 deals at
# 3000 pairs, seed 42 at 64 pairs): the largest error of the oracle against itself is LIVE_MEASURED x tol_row.  It is recorded, not used: the
# GPU tests (tests/test_gpu_multi_mccfr.py) hold the kernel to 1 x tol_row.
LIVE_MEASURED = 0.31   # 0.3061: seed-42 deal, small_large, 64 pairs (rows visited two or three times); 3000-pair launches stay below 0.13
