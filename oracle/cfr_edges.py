"""Edge-case tables for the exact tabular solvers (vanilla CFR, synchronous CFR, exploitability), and the fixture made from them.

TEST INFRASTRUCTURE: shared by oracle/gen_golden.py:gen_cfr_edges (which seeds the reference's own CFRTrainer with these tables, runs its
_cfr_recursive and writes tests/golden/vanilla_cfr_edges.npz) and by the tests (tests/test_cfr_edges_ref.py, tests/test_gpu_cfr_edges.py).
The product package never imports this module.

A case is three [n_infosets][4] float64 tables in the tree's infoset order -- regret_sum R, strategy_sum S, local_strategy L -- and a
function of (case name, n_legal) alone.  Padding slots (beyond a row's legal-action count) are +0.0 in all three: they are written with
np.where, never by multiplying with a 0/1 mask (a negative times 0.0 is -0.0).
"""
import json
import os

import numpy as np

from mccfr_edges import FINITE_TABLES, edge_table, reference_sigma, same_bits_or_same_nonfinite  # noqa: F401  (re-exported for the tests)

# case -> (regret table, strategy_sum kind, the table local_strategy is regret-matching OF)
#   regret tables: the five finite tables of oracle/mccfr_edges.py, plus
#     inf    `big` with +inf in slot 0 of every 7th row: positive part inf, row sum inf, inf / inf = NaN and x / inf = 0 in the reference's own lines
#     nan    `big` with NaN  in slot 0 of every 7th row: np.maximum(NaN, 0) is NaN, the row sum is NaN, `NaN > 0` is False -> the uniform row
#   local_strategy: reference_sigma of the case's own regret table ("consistent": what the reference itself would hold between visits), except
#     nan_held  the NaN table with local_strategy = InfoNode.get_strategy of it (vanilla_cfr.py:23-30: `norm_sum > 0`, so a NaN row holds the
#            UNIFORM strategy), where reference_sigma -- the MCCFR node's `sum == 0` test -- gives a NaN row.  The two formulas agree on every
#            other table.  `nan` floods most of the tree with NaN through the reach products; `nan_held` keeps the NaN in the seeded cells, so
#            nearly every other cell is a finite number that depends on how a NaN regret is regret-matched.
#     stale  regrets `big`, local_strategy = regret-matching of `onehot`: legal in the reference, where local_strategy is state of its own
#            (it is what the children of a node are weighted with until the node's visit ends, vanilla_cfr.py:79-97)
CASES = {
    "allneg": ("allneg", "rand", "allneg"),
    "onehot": ("onehot", "zero_rows", "onehot"),
    "small_large": ("small_large", "subnormal_rows", "small_large"),
    "subnormal": ("subnormal", "rand", "subnormal"),
    "big": ("big", "overflow", "big"),
    "inf": ("inf", "rand", "inf"),
    "nan": ("nan", "rand", "nan"),
    "nan_held": ("nan", "rand", "nan"),
    "stale": ("big", "zero_rows", "onehot"),
}
FINITE_CASES = ("allneg", "onehot", "small_large", "subnormal", "big")          # consistent and finite: every solver takes them
NONFINITE_CASES = ("inf", "nan", "nan_held")
LANE_CASES = FINITE_CASES + ("nan_held",)      # local_strategy == InfoNode.get_strategy(regret_sum) bit for bit: what the lane-per-deal kernel's row image can hold
S_KINDS = ("rand", "zero_rows", "subnormal_rows", "overflow")


def _legal(n_legal):
    return np.arange(4)[None, :] < np.asarray(n_legal, np.int64)[:, None]


def regret_table(name, n_legal):
    if name in ("inf", "nan"):
        R = edge_table("big", n_legal)
        R[::7, 0] = np.inf if name == "inf" else np.nan      # slot 0 is legal in every row
        return R
    return edge_table(name, n_legal)


def strategy_sum_table(kind, n_legal):
    """Non-zero strategy sums, legal cells only (fixed RandomState, drawn for all four slots of every row).
    rand            uniform [0, 1e3)
    zero_rows       rand with every 3rd row all zero (the average policy's uniform fallback next to accumulated rows), and an exact 0.0 in
                    slot 0 of every 3rd row from row 1 (a probability of exactly zero)
    subnormal_rows  rand with every 3rd row at k * 5e-324, k = 1..4 by slot: subnormal sums, quotients k / sum(k)
    overflow        rand with every 3rd row at 1.2e308 * [1, 0.5, 0.25, 0.125]: a row of two or more cells sums to +inf, the average policy
                    of the row is S / inf = 0.0 throughout (one-cell rows stay finite: 1.0)"""
    n_legal = np.asarray(n_legal, np.int64)
    I = n_legal.size
    rows = np.arange(I)
    S = np.random.RandomState(11).random_sample((I, 4)) * 1e3
    third = rows % 3 == 0
    if kind == "zero_rows":
        S[third] = 0.0
        S[rows % 3 == 1, 0] = 0.0
    elif kind == "subnormal_rows":
        S[third] = 5e-324 * np.arange(1, 5)
    elif kind == "overflow":
        S[third] = 1.2e308 * np.array([1.0, 0.5, 0.25, 0.125])
    elif kind != "rand":
        raise KeyError(kind)
    return np.ascontiguousarray(np.where(_legal(n_legal), S, 0.0))


def tables(case, n_legal):
    """(R, S, L) of `case` for a deal whose infoset i has n_legal[i] legal actions."""
    r_name, s_kind, l_name = CASES[case]
    with np.errstate(invalid="ignore"):
        L = reference_sigma(regret_table(l_name, n_legal), n_legal)      # inf: inf / inf = NaN, as in the reference
    if case == "nan_held":
        nanrow = np.isnan(L).any(1)
        L[nanrow] = 1.0 / np.asarray(n_legal, np.float64)[nanrow, None]
    return regret_table(r_name, n_legal), strategy_sum_table(s_kind, n_legal), np.ascontiguousarray(np.where(_legal(n_legal), L, 0.0))


def same_bits(a, b):
    """a == b bit for bit: float64 arrays compared as uint64 (-0.0 is not +0.0, a NaN equals only the same NaN)."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))


def same(case, a, b):
    """same_bits, except in the inf / nan cases: there the finite cells bit for bit and the others by kind (a NaN's payload and sign are
    not part of what the reference defines: numpy and the device may produce different quiet NaNs from the same operation)."""
    return same_bits_or_same_nonfinite(np.asarray(a, np.float64), np.asarray(b, np.float64)) if case in NONFINITE_CASES else same_bits(a, b)


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------
FIXTURE = "vanilla_cfr_edges.npz"
N_ITERS = 3
# (case, deal seed): most on the 251-infoset deal; the seed-42 deal (738 infosets, the reference's own) for the -0.0 case and the NaN case
FIXTURE_CASES = [(c, 282) for c in CASES] + [("allneg", 42), ("nan_held", 42)]
# CFRTrainer._cfr_recursive(state, traverser, reach_p0, reach_p1) on a state below the root: (case, deal, traverser, legal-action indices, r0, r1)
TRAVERSE_FROM = [("small_large", 282, 0, (1, 2, 0), 0.0, 1.0), ("onehot", 282, 1, (3, 0, 2, 1, 1, 0), 5e-324, 1e-300)]


def fixture(golden_dir):
    g = np.load(os.path.join(golden_dir, FIXTURE), allow_pickle=False)
    return g, json.loads(str(g["cases"]))
