"""The restatement of the exact weighted CFR iteration across decks (tests/full_chance_cfr_ref.py) held to independent code:

  (a) a depth-first recursive weighted CFR per deck with rows shared by pair, sweep by sweep from the same tables.  It adds in another order (math.fsum
      for a node's value, the decks' partial sums joined last deck first), so the comparison is within a reorder budget, derived below;
  (b) the exploitability restatement's value pass: the first sweep's value IS solve(..., which=1)["out4"][3], on bits;
  (c) cfr_variants_ref's weighting rule, on planted cells: R exactly 0.0, -0.0, negative regrets, weights 0 and 1;
  (d) with one round to go, on 3 decks, the average policy's (BR0 + BR1) / 2: there the game has perfect recall and the response is THE best response;
  (e) the tables, deck sets and conditions of tests/test_gpu_full_chance_cfr_edges.py: (a) again from every finite edge table, from `huge_finite` and on
      300 decks; the segment lengths, deck spans, subnormal and NaN counts that module relies on; `huge` as a fixed function of the pair list;
  (f) the restatement run with the kernel mutations that module names, where they concern mc_sigma and the weighting rule.

THE REORDER BUDGET of (a), derived as tests/full_chance_ref.py's users derive theirs: the number of terms times eps times the sum of magnitudes.
Both codes compute, in float64, the same real number for every cell.  A regret cell is the sum over the m nodes g that hold the pair of
w_opp[g] (x[child] - x[g]); every such term is itself built from at most 36^R leaf values under g and at most 6 R reach factors above it, each
joined by one rounded operation, so at most m (36^R + 6 R + 4) rounded operations feed the cell (the 4: the subtraction, the product, the add
into the row and the weighting).  Each operation's rounding is at most eps = 2^-52 of a partial result, and no partial result exceeds the same
expression evaluated on magnitudes: A = sum over g of w_opp[g] (|x|[child] + |x|[g]) + |R before|, with |x| the value pass run on |leaf|.  Hence
|difference| <= 2 m (36^R + 6 R + 4) eps A; the 2 covers both codes' errors, and a sum within that distance of zero taking the other branch of the
weighting (both branches scale by at most 1).  Strategy cells: the same with A = sum of w_own[g] prob[g][a] + |S before|.  A sweep's value: the n
root values of at most 36^R + 6 R operations each and the n adds of the mean: (36^R + 6 R + n) eps mean of |x|[root]."""
import math
import types

import numpy as np
import pytest

import cfr_variants_ref as CV
import full_chance_cfr_ref as CFR
import full_chance_exploit_ref as X
import full_chance_ref as W
import full_mccfr_ref as F
import mccfr_edges as ME
import test_gpu_full_chance_cfr as G            # (fixture builders are plain CPU code; only the module's tests carry the gpu mark)
import test_gpu_full_chance_cfr_edges as GE

SEED = 0x5C09A
EPS = 2.0 ** -52
DCFR = dict(alpha=1.5, beta=0.0, gamma=2.0)
SETS = [(5, 3, None), (5, 5, 0), (4, 3, 0), (4, 5, 0)]     # (round of the root, decks, fixed seat); the first and last are the GPU tests' R = 1, 2 sets


def trained(root, decks, iters=3, batch=4):
    rows, counter = W.Rows(), 0
    for _ in range(iters):
        counter = W.iterate(root, decks, batch, SEED, rows, counter)
    return rows.R, rows.S


def dfs_sweep(root, decks, R, S, w, update):
    """an independent sweep: a recursion per deck, rows shared by pair -> (value, R', S', budget_R, budget_S, value budget)"""
    rounds = 6 - int(root.s.round_number)
    ops = 36 ** rounds + 6 * rounds + 4
    per_deck, values, mags = [], [], []

    def rec(st, r0, r1, acc):
        if st.s.terminal:
            v = st.s.r2[0] / 2.0
            return v, abs(v)
        p = st.s.step & 1
        h = sorted(F.hand(st, p))
        n = len(h)
        if n == 1:
            return rec(F.child(st, h[0]), r0, r1, acc)
        key = W.wide_key(st, p)
        sg = F.sigma_of(R.get(key, [0.0] * 3), n)
        kids = [rec(F.child(st, c), r0 * sg[a] if p == 0 else r0, r1 * sg[a] if p == 1 else r1, acc) for a, c in enumerate(h)]
        v = math.fsum(sg[a] * kids[a][0] for a in range(n))
        m = math.fsum(sg[a] * kids[a][1] for a in range(n))
        if update is None or update == p:
            opp, own, sgn = (r1, r0, 1.0) if p == 0 else (r0, r1, -1.0)
            row = acc.setdefault(key, [[0.0] * 3, [0.0] * 3, [0.0] * 3, [0.0] * 3, 0])
            for a in range(n):
                row[0][a] += opp * (sgn * (kids[a][0] - v))
                row[1][a] += own * sg[a]
                row[2][a] += opp * (kids[a][1] + m)
                row[3][a] += own * sg[a]
            row[4] += 1
        return v, m

    for deck in decks:
        acc = {}
        v, m = rec(W.root_on(root, deck), 1.0, 1.0, acc)
        per_deck.append(acc)
        values.append(v)
        mags.append(m)
    R2, S2 = {k: list(v) for k, v in R.items()}, {k: list(v) for k, v in S.items()}
    bR, bS = {}, {}
    total = {}
    for acc in reversed(per_deck):               # the decks' partial sums joined last deck first
        for k, row in acc.items():
            t = total.setdefault(k, [[0.0] * 3, [0.0] * 3, [0.0] * 3, [0.0] * 3, 0])
            for a in range(3):
                for c in range(4):
                    t[c][a] += row[c][a]
            t[4] += row[4]
    for k, (dR, dS, aR, aS, m) in total.items():
        n = W.key_actions(k)
        old_R, old_S = R.get(k, [0.0] * 3), S.get(k, [0.0] * 3)
        R2[k] = [CFR.weigh(old_R[a] + dR[a], w[0], w[1]) if a < n else 0.0 for a in range(3)]
        S2[k] = [(old_S[a] + dS[a]) * w[2] if a < n else 0.0 for a in range(3)]
        bR[k] = [2.0 * m * ops * EPS * (aR[a] + abs(old_R[a])) for a in range(3)]
        bS[k] = [2.0 * m * ops * EPS * (aS[a] + abs(old_S[a])) for a in range(3)]
    n = len(decks)
    return math.fsum(values) / n, R2, S2, bR, bS, (ops + n) * EPS * (math.fsum(mags) / n)


# ---- (a) the depth-first recursion per deck, sweep by sweep ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", ["empty", "trained"])
@pytest.mark.parametrize("r0,n,fix_seat", SETS)
def test_sweeps_by_depth_first_recursion(oracle, r0, n, fix_seat, start):
    decks, _, root = G.packet(oracle, r0, n, fix_seat)
    tree = G.tree_of(root, decks, 6 - r0)
    R, S = ({}, {}) if start == "empty" else trained(root, decks)
    hold_sweeps_to_recursion(root, decks, tree, R, S)
    assert any(max(r) > 0.0 for r in R.values())


def hold_sweeps_to_recursion(root, decks, tree, R, S):
    """four weighted sweeps from R, S (changed in place), each against dfs_sweep from the same tables within the reorder budget"""
    CFR.claim(tree, R, S)
    worst = 0.0
    for w, update in (((1.0, 1.0, 1.0), None), ((0.75, 0.0, 0.5), 0), ((0.75, 0.5, 0.25), 1), ((1.0, 0.0, 1.0), None)):
        v2, R2, S2, bR, bS, bv = dfs_sweep(root, decks, R, S, w, update)
        v = CFR.sweep(tree, R, S, w, update)                       # in place: the next sweep starts from the restatement's tables in both codes
        assert abs(v - v2) <= bv, (v, v2, bv)
        assert set(R2) == set(R) and set(S2) == set(S)
        touched = 0
        for k in R:
            for a in range(3):
                eR, eS = abs(R[k][a] - R2[k][a]), abs(S[k][a] - S2[k][a])
                assert eR <= bR.get(k, [0.0] * 3)[a] and eS <= bS.get(k, [0.0] * 3)[a], (k, a, R[k], R2[k], S[k], S2[k])
                if eR:
                    worst = max(worst, eR / bR[k][a])
            touched += k in bR
            assert a < W.key_actions(k) or (R[k][2] == 0.0 and S[k][2] == 0.0)
        players = {(k[0] >> 62) & 1 for k in bR}
        assert players == ({0, 1} if update is None else {update}) and touched > 0
    print("largest regret difference / budget:", worst)


# ---- (b) the first sweep's value is the exploitability restatement's value pass ----------------------------------------------------------------------
@pytest.mark.parametrize("alternating", [True, False])
@pytest.mark.parametrize("r0,n,fix_seat", SETS)
def test_first_sweep_value_is_the_value_pass(oracle, r0, n, fix_seat, alternating):
    decks, _, root = G.packet(oracle, r0, n, fix_seat)
    tree = G.tree_of(root, decks, 6 - r0)
    for R, S in (({}, {}), trained(root, decks)):
        _, _, values = CFR.iterate(tree, R, S, [[1.0, 0.5, 0.25]] * 2, alternating)
        want = X.solve(tree, R, S, which=1)["out4"][3]
        assert G.same_bits(values[0, 0], want)
        assert alternating or G.same_bits(values[:, 0], values[:, 1])
    assert not alternating or r0 == 5 or values[0, 0] != values[0, 1]              # sweep 1 of an iteration meets player 0's new rows


def test_claim_and_copies(oracle):
    decks, _, root = G.packet(oracle, 4, 5, 0)
    tree = G.tree_of(root, decks, 2)
    R, S = trained(root, decks)
    before = ({k: list(v) for k, v in R.items()}, {k: list(v) for k, v in S.items()})
    R0, S0, v0 = CFR.iterate(tree, R, S, np.zeros((0, 3)))
    assert (R, S) == before and (R0, S0) == before and v0.shape == (0, 2)          # no iteration claims nothing
    R1, S1, _ = CFR.iterate(tree, R, S, [[1.0, 1.0, 1.0]])
    assert (R, S) == before and set(R1) == set(S1) == set(R) | set(G.level_pairs(tree))
    outside = set(R) - set(G.level_pairs(tree))
    assert all(R1[k] == R[k] and S1[k] == S[k] for k in outside)


# ---- (c) the weighting rule ---------------------------------------------------------------------------------------------------------------------------
def chain_tree(value_x2):
    """an 8-ply game of one action a ply in cfr_variants_ref's tree arrays: every infoset's increment is +-0.0 and its strategy increment 1.0, so its
    sweep is the weighting rule alone"""
    t = types.SimpleNamespace(n_nodes=9, n_infosets=8)
    t.depth, t.term = np.arange(9), np.array([0] * 8 + [1])
    t.r2 = np.zeros((9, 2), np.int64)
    t.r2[8, 0] = value_x2
    t.nlegal, t.player = np.array([1] * 8 + [0]), np.array([0, 1] * 4 + [0])
    t.infoset, t.infoset_player, t.infoset_nlegal = np.array(list(range(8)) + [0]), np.array([0, 1] * 4), np.ones(8, np.int64)
    t.child = np.zeros((9, 4), np.int64)
    t.child[:8, 0] = np.arange(1, 9)
    return t


CELLS = [0.0, -0.0, -1.5, 2.0, -1e-300, 1e-300, 3.25, -7.0]


@pytest.mark.parametrize("w", [(1.0, 0.0, 1.0), (0.0, 1.0, 0.0), (1.0, 1.0, 1.0), (0.0, 0.0, 0.5), (0.5, 0.25, 0.75), (1.0, 0.5, 1.0)])
def test_weighting_rule_is_cfr_variants_refs(w):
    ref = CV.Ref(chain_tree(3))
    for shift in range(2):                                         # every cell at a player-0 and at a player-1 infoset
        cells = CELLS[shift:] + CELLS[:shift]
        R, S = np.zeros((8, 4)), np.zeros((8, 4))
        R[:, 0], S[:, 0] = cells, np.arange(8) / 4.0
        ref.sweep(R, S, w, None)
        for i, r in enumerate(cells):
            d = 0.0                                                # dR = 0.0 + opp * (sgn * (v - v)): +0.0 for either player
            assert G.same_bits(R[i, 0], CFR.weigh(r + d, w[0], w[1])), (i, r, w)
            assert G.same_bits(S[i, 0], (i / 4.0 + 1.0) * w[2])
    assert G.same_bits(CFR.weigh(-0.0, 1.0, 1.0), -0.0) and G.same_bits(CFR.weigh(-0.0, 1.0, 0.0), -0.0) and G.same_bits(CFR.weigh(0.0, 0.0, 1.0), 0.0)
    assert math.isnan(CFR.weigh(float("nan"), 1.0, 0.0))           # !(NaN <= 0): the positive branch


@pytest.mark.parametrize("w", [(1.0, 0.0, 1.0), (0.0, 1.0, 0.0), (0.5, 0.25, 0.75)])
@pytest.mark.parametrize("alternating", [True, False])
def test_weighting_rule_on_planted_cells_of_a_forest(oracle, w, alternating):
    """a weighted sweep is the unweighted sweep (weights 1: exact) followed by cfr_variants_ref's rule per cell, on tables that hold the edge cells"""
    decks, _, root = G.packet(oracle, 4, 5, 0)
    tree = G.tree_of(root, decks, 2)
    R, S = G.planted_tables(tree)
    assert {0.0, -1.5} <= {x for r in R.values() for x in r} and any(math.copysign(1.0, x) < 0 and x == 0.0 for r in R.values() for x in r)
    CFR.claim(tree, R, S)
    for update in ((0, 1) if alternating else (None,)):
        Rv, Sv = {k: list(v) for k, v in R.items()}, {k: list(v) for k, v in S.items()}
        assert G.same_bits(CFR.sweep(tree, Rv, Sv, (1.0, 1.0, 1.0), update), CFR.sweep(tree, R, S, w, update))
        keys = sorted(R)
        a, s = np.array([Rv[k] for k in keys]), np.array([Sv[k] for k in keys])
        mine = np.array([update is None or ((k[0] >> 62) & 1) == update for k in keys])[:, None] & (np.arange(3)[None, :] < np.array([W.key_actions(k) for k in keys])[:, None])
        want_R = np.where(mine, np.where(~(a <= 0.0), a * w[0], a * w[1]), a)           # cfr_variants_ref.Ref.sweep's two lines
        want_S = np.where(mine, s * w[2], s)
        assert G.same_bits(np.array([R[k] for k in keys]), want_R) and G.same_bits(np.array([S[k] for k in keys]), want_S)
        assert (a[mine] <= 0.0).any() and (a[mine] > 0.0).any()


# ---- (d) one round to go: the average policy's exploitability falls ---------------------------------------------------------------------------------
def test_exploitability_falls_with_one_round_to_go(oracle):
    from scopa_amd.algorithms import schedule
    decks, _, root = G.shape(oracle, 1)
    tree = G.tree_of(root, decks, 1)
    figures, R, S, t = [X.solve(tree, {}, {}, 0)["out4"][0]], {}, {}, 0
    for n in (10, 190):
        R, S, _ = CFR.iterate(tree, R, S, schedule("dcfr", t, n, **DCFR), True)
        t += n
        figures.append(X.solve(tree, R, S, 0)["out4"][0])
    print("R = 1, 3 decks, (BR0 + BR1) / 2 of the average policy: empty store %.6g, after 10 alternating DCFR(1.5, 0, 2) iterations %.6g, after 200 %.6g" % tuple(figures))
    assert all(f >= -1e-12 for f in figures)
    assert figures[2] < figures[1] < figures[0]


# ---- (e) what tests/test_gpu_full_chance_cfr_edges.py plants and sweeps, held without a GPU ----------------------------------------------------------
FINITE = tuple(t for t in GE.TABLES if t not in GE.LOOSE)


@pytest.mark.parametrize("name", FINITE)
def test_edge_tables_by_depth_first_recursion(oracle, name):
    decks, _, root = G.shape(oracle, 2)
    tree = G.tree_of(root, decks, 2)
    R, S = GE.edge_tables(G.level_pairs(tree), name)
    hold_sweeps_to_recursion(root, decks, tree, R, S)


def test_300_decks_by_depth_first_recursion(oracle):
    decks, _, root = G.packet(oracle, 5, 300, None)
    hold_sweeps_to_recursion(root, decks, G.tree_of(root, decks, 1), {}, {})


@pytest.mark.parametrize("name", GE.TABLES)
def test_edge_table_conditions(oracle, name):
    """the conditions the GPU module asserts of each table on the R = 2 forest hold in the restatement, which raises nothing on any of them"""
    decks, _, root = G.shape(oracle, 2)
    tree = G.tree_of(root, decks, 2)
    pairs = G.level_pairs(tree)
    R0, S0 = GE.edge_tables(pairs, name)
    assert sorted(R0) == sorted(S0) == pairs and 3 * len(pairs) == 2043
    R1, S1, values = CFR.iterate(tree, R0, S0, GE.EDGE_W, True)
    R2, S2, v2 = CFR.iterate(tree, R1, S1, np.ones((1, 3)), False)
    GE.edge_conditions(name, R0, S0, R1, S1, values, R2, S2)
    keys = sorted(R1)
    print(name, "regret words changed by the first call: %d of %d; subnormal regret cells after it: %d; NaN cells: %d regret, %d strategy" % (
        GE.changed_words(R0, R1) + (GE.subnormal_cells(R1), int(np.isnan(GE.words(R1, keys)).sum()), int(np.isnan(GE.words(S1, keys)).sum()))))
    finite = all(np.isfinite(GE.words(t, keys)).all() for t in (R1, S1, R2, S2)) and np.isfinite(values).all() and np.isfinite(v2).all()
    assert finite == (name != "huge")           # `nonfinite` makes no non-finite number in this arithmetic: its comparison by kind is one on bits


def test_wide_deck_sets_are_what_the_gpu_tests_need(oracle):
    decks, _, root = G.packet(oracle, 5, 300, None)
    tree = G.tree_of(root, decks, 1)
    assert len({d.tobytes() for d in decks}) == 300 and [len(ks) for _, n, ks in tree[0] if n > 1] == [300, 900, 2700, 5400]
    longest, span = GE.segments_and_spans(tree)
    print("300 decks, R = 1: longest segment", longest, "widest pair", span, "decks,", len(G.level_pairs(tree)), "pairs")
    assert longest >= 64 and span >= 32
    decks, _, root = G.packet(oracle, 4, 70, 0)
    tree = G.tree_of(root, decks, 2)
    longest, span = GE.segments_and_spans(tree)
    print("70 decks, R = 2: longest segment", longest, "widest pair", span, "decks,", len(G.level_pairs(tree)), "pairs")
    assert longest >= 128 and span == 70
    decks, _, root = G.shape(oracle, 3)
    assert GE.segments_and_spans(G.tree_of(root, decks, 3))[0] > 64


def test_huge_is_a_fixed_function_of_the_pair_list(oracle):
    decks, _, root = G.shape(oracle, 2)
    pairs = G.level_pairs(G.tree_of(root, decks, 2))
    a, b = CFR.huge_rows(pairs), CFR.huge_rows(list(reversed(pairs)))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    keys, n_act, R, S = a
    legal = np.arange(3)[None, :] < n_act[:, None]
    assert keys.tolist() == [list(k) for k in pairs] and not R[~legal].any() and not S[~legal].any()
    assert np.isposinf(R).sum() > 20 and np.isneginf(R).sum() > 20 and np.isnan(R).sum() > 20 and np.isposinf(S).sum() > 20
    assert (np.isfinite(R) | legal).all() and (~np.isfinite(R)).sum(1).max() == 1 and (S[legal] >= 0.0).all() and not np.isnan(S).any()
    assert np.abs(R[np.isfinite(R)]).max() > 1.6e308 and (R[np.isfinite(R)] < 0.0).any()
    _, _, Rf, Sf = CFR.huge_rows(pairs, finite=True)
    assert np.isfinite(Rf).all() and np.isfinite(Sf).all()
    same = np.isfinite(R) & np.isfinite(S)
    assert G.same_bits(Rf[same], R[same]) and G.same_bits(Sf[same], S[same]) and (Rf[~np.isfinite(R)] == 1e308).all()


def test_deck_order_moves_the_bits(oracle):
    """what test_deck_order_defines_the_bits compares on the device: the same decks in another order give the restatement other bits"""
    decks, _, root = G.shape(oracle, 2)
    w = G.weights_of("dcfr", 0, 3)
    a = CFR.iterate(G.tree_of(root, decks, 2), {}, {}, w, True)
    b = CFR.iterate(G.tree_of(root, np.ascontiguousarray(decks[[3, 0, 4, 2, 1]]), 2), {}, {}, w, True)
    keys = sorted(a[0])
    assert sorted(b[0]) == keys
    print("deck order: regret bits", "equal" if G.same_bits(GE.words(a[0], keys), GE.words(b[0], keys)) else "differ", "; values", "equal" if G.same_bits(a[2], b[2]) else "differ")
    assert np.allclose(GE.words(a[0], keys), GE.words(b[0], keys), rtol=0, atol=1e-9)


# ---- (f) the restatement under the kernel mutations the GPU module names ---------------------------------------------------------------------------
def mutant_run(oracle, monkeypatch, name, weigh=None, sigma_of=None):
    decks, _, root = G.shape(oracle, 2)
    tree = G.tree_of(root, decks, 2)
    R0, S0 = GE.edge_tables(G.level_pairs(tree), name)
    want = CFR.iterate(tree, R0, S0, GE.EDGE_W, True)
    if weigh:
        monkeypatch.setattr(CFR, "weigh", weigh)
    if sigma_of:
        monkeypatch.setattr(F, "sigma_of", sigma_of)
    got = CFR.iterate(tree, R0, S0, GE.EDGE_W, True)
    keys = sorted(want[0])
    return all(ME.same_bits_or_same_nonfinite(x, y) for x, y in ((GE.words(got[0], keys), GE.words(want[0], keys)), (GE.words(got[1], keys), GE.words(want[1], keys)), (got[2], want[2])))


def sigma_mutant(positive, uniform_if):
    def sigma_of(R, n):
        pos = [R[i] if positive(R[i]) else 0.0 for i in range(n)]
        s = pos[0]
        for i in range(1, n):
            s += pos[i]
        return [1.0 / n] * n if uniform_if(s) else [x / s for x in pos]
    return sigma_of


def test_restatement_separates_the_subnormal_mutation(oracle, monkeypatch):
    assert not mutant_run(oracle, monkeypatch, "subnormal", sigma_of=sigma_mutant(lambda r: r > 2.3e-308, lambda s: s == 0.0))


def test_nan_rule_mutations_are_equivalent_by_kind(oracle, monkeypatch):
    """`r > 0` for `!(r <= 0)` in the weighting and `!(s > 0)` for `s == 0` in the regret matching differ only where r or s is NaN.  s is a sum of
    cells that are 0.0 or positive, so it is never NaN; a NaN r times either weight is NaN.  Under the comparison by kind no table separates them"""
    for name in ("huge", "nonfinite", "allneg"):
        assert mutant_run(oracle, monkeypatch, name, weigh=lambda r, p, n: r * p if r > 0.0 else r * n)
        monkeypatch.undo()
        assert mutant_run(oracle, monkeypatch, name, sigma_of=sigma_mutant(lambda r: r > 0.0, lambda s: not s > 0.0))
        monkeypatch.undo()
