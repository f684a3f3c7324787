"""The exact tabular solvers on edge-case tables, CPU side: the oracle against the REFERENCE, and the oracle's exploitability against exact arithmetic.

tests/golden/vanilla_cfr_edges.npz holds what the reference's own CFRTrainer._cfr_recursive leaves (oracle/gen_golden.py:gen_cfr_edges) when its
InfoNodes are seeded with the tables of oracle/cfr_edges.py: regrets with nothing positive (negatives, -0.0), one-hot rows, 1e-9 next to 1e6,
subnormals, |R| ~ 1e12, +inf and NaN cells, a local_strategy that is NOT regret-matching of regret_sum, and non-zero strategy sums (zero rows,
subnormal rows, rows whose sum overflows).  The oracle must reproduce every case bit for bit -- compared as uint64, so -0.0 is not +0.0 -- and
the non-finite cells by kind; the GPU module (tests/test_gpu_cfr_edges.py) then holds the kernels to the fixture and to the oracle.

The NaN cases are the evidence for the regret-matching select: InfoNode.get_strategy is np.maximum(regret_sum, 0), which keeps a NaN (the row
sum is then NaN, `NaN > 0` is False, the row plays uniform); `R > 0 ? R : 0` turned the NaN into 0 and normalised the rest of the row."""
from fractions import Fraction

import numpy as np
import pytest

import cfr_edges as E

N_FIXTURE = len(E.FIXTURE_CASES) + len(E.TRAVERSE_FROM)


def _tree(oracle, deal, _cache={}):
    if deal not in _cache:
        _cache[deal] = oracle.Tree(seed=deal)
    return _cache[deal]


def test_fixture_case_list(golden):
    g, meta = E.fixture(golden.dir)
    assert [(m["case"], m["deal"]) for m in meta if m["kind"] == "iterate"] == E.FIXTURE_CASES
    assert [(m["case"], m["deal"], m["traverser"], tuple(m["path"]), float(m["r0"]), float(m["r1"])) for m in meta if m["kind"] == "from"] == E.TRAVERSE_FROM
    assert all(m["iters"] == E.N_ITERS for m in meta if m["kind"] == "iterate") and len(meta) == N_FIXTURE
    assert {m["case"] for m in meta} >= set(E.CASES)


def test_edge_tables_are_what_they_claim(oracle):
    t = _tree(oracle, 282)
    n = t.infoset_nlegal.astype(int)
    legal = np.arange(4)[None, :] < n[:, None]
    assert t.n_infosets == 251 and _tree(oracle, 42).n_infosets == 738
    for case in E.CASES:
        R, S, L = E.tables(case, n)
        for a in (R, S, L):      # padding is +0.0, bit for bit
            assert not a[~legal].view(np.uint64).any(), case
        assert (S[legal] >= 0).all() and S.any()
    R, _, L = E.tables("inf", n)
    assert np.isposinf(R).sum() == len(range(0, 251, 7)) and np.isnan(L[::7, 0]).all() and np.isfinite(L[1::7]).all()
    R, _, L = E.tables("nan", n)
    assert np.isnan(R).sum() == len(range(0, 251, 7)) and np.isnan(L[::7][legal[::7]]).all()
    Rh, _, Lh = E.tables("nan_held", n)
    assert E.same_bits(Rh, R) and np.isfinite(Lh).all() and np.array_equal(Lh[::7], np.where(legal[::7], 1.0 / n[::7, None], 0.0))
    R, _, L = E.tables("stale", n)
    assert not E.same_bits(L, E.reference_sigma(R, n)) and set(np.unique(L)) == {0.0, 1.0}
    for case in E.FINITE_CASES:      # "consistent": the MCCFR node's formula and InfoNode.get_strategy agree
        R, _, L = E.tables(case, n)
        assert E.same_bits(L, E.reference_sigma(R, n))
    S = E.strategy_sum_table("zero_rows", n)
    assert (S[::3] == 0).all() and (S[1::3, 0] == 0).all() and (S[2::3][legal[2::3]] > 0).all()
    S = E.strategy_sum_table("subnormal_rows", n)
    assert (S[::3][legal[::3]] < 2.3e-308).all() and (S[::3][legal[::3]] > 0).all()
    S = E.strategy_sum_table("overflow", n)
    with np.errstate(over="ignore"):
        assert np.isposinf(S[::3].sum(1)[n[::3] > 1]).all() and np.isfinite(S).all()


def test_rebuilt_inputs_are_the_fixtures_inputs(oracle, golden):
    """oracle/cfr_edges.py rebuilds, bit for bit, the tables the reference was seeded with (they are in the fixture, once per deal and table)."""
    g, meta = E.fixture(golden.dir)
    seen = 0
    for m in meta:
        t = _tree(oracle, m["deal"])
        assert np.array_equal(g[f"in{m['deal']}_nlegal"], t.infoset_nlegal)
        R, S, L = E.tables(m["case"], t.infoset_nlegal)
        r_name, s_kind, l_name = E.CASES[m["case"]]
        for tag, a in ((f"R_{r_name}", R), (f"S_{s_kind}", S), (f"L_{m['case'] if m['case'] == 'nan_held' else l_name}", L)):
            assert E.same(m["case"], a, g[f"in{m['deal']}_{tag}"]), (m, tag)
            seen += 1
    assert seen == 3 * N_FIXTURE


@pytest.mark.parametrize("n", range(len(E.FIXTURE_CASES)))
def test_oracle_reproduces_the_reference_from_edge_tables(oracle, golden, n):
    """og_cfr_exact from the seeded tables: regret_sum, strategy_sum, local_strategy and the root value of every traversal, bit for bit
    (uint64 views); in the inf / nan cases the finite cells bit for bit and the same cells NaN / +inf / -inf."""
    g, meta = E.fixture(golden.dir)
    m = meta[n]
    case = m["case"]
    t = _tree(oracle, m["deal"])
    R, S, L = E.tables(case, t.infoset_nlegal)
    rv = t.cfr_exact(R, S, L, m["iters"])
    nonfinite = int((~np.isfinite(g[f"c{n}_regret"])).sum())
    print(case, m["deal"], "non-finite regret cells in the reference:", nonfinite, "; -0.0 regret cells:", int((np.signbit(g[f"c{n}_regret"]) & (g[f"c{n}_regret"] == 0)).sum()))
    assert (case in E.NONFINITE_CASES) == (nonfinite > 0)
    assert E.same(case, rv, g[f"c{n}_root"])
    assert E.same(case, R, g[f"c{n}_regret"])
    assert E.same(case, S, g[f"c{n}_strategy"])
    assert E.same(case, L, g[f"c{n}_local"])


def test_fixture_has_negative_zero_regrets_and_finite_cells_beside_the_nans(golden):
    """What makes the bit comparison matter: the reference leaves -0.0 regret cells from the `allneg` table on the seed-42 deal, and the nan_held
    cases keep most cells finite (so the comparison is of numbers, not of NaN floods)."""
    g, meta = E.fixture(golden.dir)
    n = [(m["case"], m["deal"]) for m in meta].index(("allneg", 42))
    R = g[f"c{n}_regret"]
    assert (np.signbit(R) & (R == 0)).sum() == 6
    for deal in (282, 42):
        n = [(m["case"], m["deal"]) for m in meta].index(("nan_held", deal))
        R, L = g[f"c{n}_regret"], g[f"c{n}_local"]
        assert 0 < np.isnan(R).sum() < 0.06 * R.size and np.isfinite(L).all() and np.isfinite(g[f"c{n}_root"]).all()


@pytest.mark.parametrize("n", range(len(E.FIXTURE_CASES), N_FIXTURE))
def test_oracle_traverse_from_with_tiny_reaches(oracle, golden, n):
    """_cfr_recursive on a state three / six plies down with reach arguments (0.0, 1.0) and (5e-324, 1e-300)."""
    g, meta = E.fixture(golden.dir)
    m = meta[n]
    t = _tree(oracle, m["deal"])
    R, S, L = E.tables(m["case"], t.infoset_nlegal)
    R0, S0, L0 = R.copy(), S.copy(), L.copy()
    v = t.cfr_exact_from(R, S, L, m["path"], m["traverser"], float(m["r0"]), float(m["r1"]))
    assert E.same_bits(np.array([v]), g[f"c{n}_value"])
    assert E.same_bits(R, g[f"c{n}_regret"]) and E.same_bits(S, g[f"c{n}_strategy"]) and E.same_bits(L, g[f"c{n}_local"])
    assert not E.same_bits(R, R0) or not E.same_bits(S, S0) or not E.same_bits(L, L0)     # the call did something (six plies down the rows have one action: only strategy_sum can move)


# ---- exploitability and policy value against exact rational arithmetic ---------------------------------------------------------------
def exact_best_response(t, P):
    """Best responses and the on-policy value of policy P [n_infosets][4] on tree t in fractions.Fraction (every float64 is a rational; no
    rounding anywhere).  The definition of scopa_eval.hip / og_exploitability: the best responder picks, per infoset, the first action
    maximising sum over the infoset's nodes of (reach of everyone else) * value(child); exploitability = (BR_0 + BR_1) / 2.
    -> (br0, br1, value_p0, gaps): gaps = for every best-responder infoset with a node of non-zero reach, max q - q[a] for every action a but the chosen one."""
    F = [[Fraction(float(x)) for x in row] for row in P]
    order = sorted(range(t.n_nodes), key=lambda k: t.depth[k])
    out, gaps = [], []
    for br in (0, 1, 2):
        reach = [None] * t.n_nodes
        reach[0] = Fraction(1)
        for k in order:
            if t.term[k]:
                continue
            for a in range(t.nlegal[k]):
                reach[t.child[k][a]] = reach[k] if t.player[k] == br else reach[k] * F[t.infoset[k]][a]
        val = [None] * t.n_nodes
        by_depth = {}
        for k in order:
            by_depth.setdefault(int(t.depth[k]), []).append(k)
        for d in sorted(by_depth, reverse=True):
            members = {}
            for k in by_depth[d]:
                if t.term[k]:
                    val[k] = Fraction(int(t.r2[k][1 if br == 1 else 0]), 2)
                elif t.player[k] == br:
                    members.setdefault(int(t.infoset[k]), []).append(k)
                else:
                    val[k] = sum((F[t.infoset[k]][a] * val[t.child[k][a]] for a in range(t.nlegal[k])), Fraction(0))
            for I, nodes in members.items():
                n = t.nlegal[nodes[0]]
                q = [sum((reach[k] * val[t.child[k][a]] for k in nodes), Fraction(0)) for a in range(n)]
                best = max(range(n), key=lambda a: (q[a], -a))      # the first maximum
                if any(reach[k] != 0 for k in nodes):
                    gaps.extend(q[best] - q[a] for a in range(n) if a != best)
                for k in nodes:
                    val[k] = val[t.child[k][best]]
        out.append(val[0])
    return out[0], out[1], out[2], gaps


def _edge_policies(t):
    n = t.infoset_nlegal.astype(int)
    legal = np.arange(4)[None, :] < n[:, None]
    pol = {"uniform": np.where(legal, 1.0 / n[:, None], 0.0),
           "onehot": E.reference_sigma(E.edge_table("onehot", n), n)}                       # rows of exactly 0 and 1
    # The average policy of a strategy_sum with zero rows, subnormal rows and rows whose sum overflows.  Not E.strategy_sum_table: a row of random
    # float64 quotients sums to 1 +- 1e-16, not to 1, and two actions whose subtrees tie in real arithmetic then differ by ~1e-17 -- neither a tie
    # nor a gap.  Here every accumulated row holds small integers that sum to a power of two (times 5e-324 on the subnormal rows), so its
    # quotients are exact and sum to exactly 1; exact zeros included.
    rs = np.random.RandomState(3)
    pat = {1: [(1,)], 2: [(1, 3), (1, 1), (0, 4)], 3: [(1, 1, 2), (5, 2, 1), (0, 3, 1)], 4: [(1, 2, 2, 3), (1, 1, 1, 5), (0, 1, 3, 4), (2, 2, 2, 2)]}
    S = np.zeros((n.size, 4))
    for i, m in enumerate(n):
        S[i, :m] = rs.permutation(pat[m][rs.randint(len(pat[m]))])
    for kind, fill in (("zero_rows", lambda row: 0.0 * row), ("subnormal_rows", lambda row: 5e-324 * row), ("overflow", lambda row: np.where(row > 0, 1.2e308, 0.0))):
        Sk = S.copy()
        first = 1 if kind == "overflow" else 0        # (an all-zero policy row at the root, infoset 0, would make every value 0)
        Sk[first::3] = fill(S[first::3])
        pol["avg_" + kind] = t.average_policy(Sk)
    return pol


def test_average_policy_of_edge_strategy_sums(oracle):
    """og_average_policy is InfoNode.policy (vanilla_cfr.py:32-39) row by row in numpy: uniform where nothing was accumulated, k / sum(k) on the
    subnormal rows, S / inf = 0.0 where the row sum overflows."""
    t = _tree(oracle, 282)
    n = t.infoset_nlegal.astype(int)
    for kind in E.S_KINDS:
        S = E.strategy_sum_table(kind, n)
        want = np.zeros_like(S)
        with np.errstate(over="ignore"):
            for i, m in enumerate(n):
                s = np.sum(S[i, :m])
                want[i, :m] = S[i, :m] / s if s > 0 else np.ones(m) / m
        assert E.same_bits(t.average_policy(S), want), kind
    P = t.average_policy(E.strategy_sum_table("overflow", n))
    assert (P[::3][n[::3] > 1] == 0).all()
    P = t.average_policy(E.strategy_sum_table("subnormal_rows", n))
    assert np.array_equal(P[0, :n[0]], np.arange(1, n[0] + 1) / np.arange(1, n[0] + 1).sum())


@pytest.mark.parametrize("name", ["uniform", "onehot", "avg_zero_rows", "avg_subnormal_rows", "avg_overflow"])
def test_exploitability_and_policy_value_against_exact_best_response(oracle, name):
    """og_exploitability / og_policy_value on edge policies of the 251-infoset deal against a best response in exact rational arithmetic, at the
    project's own 1e-12 (test_exploitability_kernel_agrees_with_the_independent_best_response).  Ties are a condition, checked with the exact values
    at EVERY best-responder infoset that has a node of non-zero reach: the gap between the best action and any other is either exactly 0 (both
    sides then take the first of them) or above 1e-9, far beyond what float64 rounding of sums of <= 576 terms of magnitude <= 4 can move."""
    t = _tree(oracle, 282)
    P = _edge_policies(t)[name]
    b0, b1, v0, gaps = exact_best_response(t, P)
    near = [g for g in gaps if 0 < g <= Fraction(1, 10 ** 9)]
    print(name, "infoset-action gaps checked:", len(gaps), "exact ties:", sum(1 for g in gaps if g == 0), "smallest non-zero gap:", float(min((g for g in gaps if g > 0), default=0)))
    assert len(gaps) > 0 and not near
    e, br = t.exploitability(P)
    print(name, "exploitability", e, "exact", float((b0 + b1) / 2), "br", br, "value", t.policy_value(P))
    assert abs(Fraction(float(br[0])) - b0) <= Fraction(1, 10 ** 12) and abs(Fraction(float(br[1])) - b1) <= Fraction(1, 10 ** 12)
    assert abs(Fraction(float(e)) - (b0 + b1) / 2) <= Fraction(1, 10 ** 12)
    assert abs(Fraction(float(t.policy_value(P))) - v0) <= Fraction(1, 10 ** 12)
