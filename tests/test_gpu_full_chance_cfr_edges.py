"""GPU checks of the exact weighted CFR iteration of FullScopa across a set of decks (scopa_amd/csrc/scopa_full_chance_cfr.hip:
scopa_full_chance_cfr_iterate) where tests/test_gpu_full_chance_cfr.py does not reach: the project's edge tables and a table of cells near DBL_MAX on
every pair of a forest, deck sets wider than a wavefront and a workgroup of roots, one deck, a permuted deck list, 150 iterations in one call, a scratch
that grows by forest and by n_iters, and the cap (89 decks at R = 3) and R = 4.

The standard is that file's: the reference is tests/full_chance_cfr_ref.py's iterate on full_chance_exploit_ref's forest, fed with tables_get taken
before the call; the pair set, every regret and strategy word and every sweep value are compared on bits.  Where a planted table makes non-finite
numbers (`nonfinite`, `huge`) the comparison is mccfr_edges.same_bits_or_same_nonfinite: finite words on bits, a NaN, +inf or -inf the same kind (the
host and the device produce other NaN signs and payloads).  No tolerance appears anywhere.  The cap and R = 4 are too large for the restatement (a
forest of 4.2 million leaves: minutes for the tree alone); there the iteration is held to the project's independent exploitability sweep, device
against device.  tests/test_full_chance_cfr_ref.py holds the tables, shapes and conditions used here to its guards without a GPU.

A mutation of scopa_full_chance_cfr.hip / scopa_mccfr_sigma.h / scopa_full_chance_forest.h and the test that fails under it.  Each changes arithmetic
only, no address and no bound; each variant was built apart from the tree and run once against this module on an MI355X:
  `!(r <= 0.0)` to `r > 0.0` in k_full_chance_cfr_update      none: 32 passed.  The two differ only where r is NaN, and NaN times either weight is NaN: under
                                                              the comparison by kind no input separates them (G test_nan_rule_mutations_are_equivalent_by_kind)
  mc_sigma's `> 0.0` to `> 2.3e-308`                          test_edge_tables_on_every_pair[subnormal, subnormal+S] at R = 2 and 1, [2-huge], [2-huge_finite]
                                                              (weighted cells fall below DBL_MIN) and test_edge_tables_at_r3[subnormal];
                                                              G test_restatement_separates_the_subnormal_mutation
  `s == 0.0` to `!(s > 0.0)` in mc_sigma                      none: 32 passed.  s adds cells that are 0.0 or positive (a NaN cell fails `> 0.0`), so s lies in
                                                              [0, +inf] and is never NaN: the two are the same function of every row (G as the first)
  k_full_chance_eval_mean's loop in descending deck order     test_300_decks_with_one_round_to_go, test_70_decks_with_two_rounds_to_go and 17 more (5 and 3 decks
                                                              move a last bit too); test_one_deck passes, as it must
  `wt = d_wt + 3 * (t & 63)`                                  test_150_iterations_in_one_call, both cases, and nothing else
  `val = d_val + 2 * (t & 63)`                                test_150_iterations_in_one_call, both cases, and nothing else
  k_full_chance_cfr_update's serial sums from hi - 1 down     test_70_decks_with_two_rounds_to_go, test_edge_tables_at_r3[subnormal, big, mixed] and 16 more
  to j
  k_full_chance_cfr_store skipping rows of uniform sigma      test_edge_tables_on_every_pair[allneg] at R = 2 and 1 and 22 more (every table read-back that holds
                                                              a row with no positive regret); the cap tests were not run under the mutations

Measured once on an MI355X (wall time of the calls of a test, `-s` prints them again) and on the CPU (the restatement's time in the same test):
  every test's device calls take under 0.03 s in all (the 150-iteration calls 0.008 s, the five growth calls with their exploitability calls
  0.011 s); no test takes more than a few seconds, and where one takes more than 0.5 s it is the restatement's tree, built once per process:
  test_70_decks_with_two_rounds_to_go 3.1 s (tree 2.6 s, restatement 1.06 s), the first R = 3 case 2.0 s (tree 1.9 s), the R = 3 cases 0.17 - 0.36 s
  of restatement each, test_150_iterations_in_one_call 0.40 / 0.22 s, the growth test 0.26 s, 300 decks 0.11 s, an R = 2 edge table 0.06 s.
  The cap, 89 decks at R = 3: P = 131 693 pairs, capacity_log2 = 20; exploitability 0.003 s, cfr_iterate(1) 0.004 s a call.
  R = 4, 2 decks: P = 20 634 pairs, capacity_log2 = 17; exploitability 0.003 s, cfr_iterate(1) 0.005 s a call."""
import time

import numpy as np
import pytest

import full_chance_cfr_ref as CFR
import full_chance_exploit_ref as X
import full_chance_ref as W
import full_mccfr_ref as F
import mccfr_edges as E
from test_gpu_full_chance_cfr import (SEED, assert_tables as assert_tables_bits, level_pairs, out4_of, packet, plant, planted_tables, same_bits, shape,
                                      state_of, tables_of, tree_of, weights_of)

pytestmark = pytest.mark.gpu

EDGE_W = np.array([[1.0, 0.0, 0.5], [0.75, 0.5, 1.0], [1.0, 0.0, 0.0]])         # a negative-regret weight of 0, a strategy weight of 0, inf * 0
TABLES = E.EDGE_TABLES + ("subnormal+S", "small_large+S", "huge", "huge_finite")  # +S: the table as regret AND as strategy rows
LOOSE = ("nonfinite", "huge")                                                     # compared by kind where not finite
R3_TABLES = ("subnormal", "big", "huge", "mixed")
SUBNORMAL_MAX = 2.2250738585072014e-308                                           # DBL_MIN: below it a non-zero cell is subnormal
CLOCK = {"device": 0.0, "cpu": 0.0}


# ---- helpers ------------------------------------------------------------------------------------------------------------------------------------------
def same(a, b, loose=False):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and (E.same_bits_or_same_nonfinite(a, b) if loose else same_bits(a, b))


def edge_tables(pairs, name, tree=None):
    """the regret and strategy tables `name` over `pairs` as {(A, B): [3]}"""
    if name == "mixed":
        return planted_tables(tree, "mixed")
    if name.startswith("huge"):
        keys, _, R, S = CFR.huge_rows(pairs, finite=name == "huge_finite")
    else:
        keys, _, R, S = W.edge_rows(np.array(pairs, np.uint64), name.split("+")[0])
        S = R.copy() if name.endswith("+S") else S
    return X.table_of(keys, R), X.table_of(keys, S)


def words(table, keys):
    return np.array([table[k] for k in keys], np.float64).reshape(-1, 3)


def changed_words(R0, R1):
    """the regret words of R0's pairs whose bits differ in R1 -> (changed, all)"""
    keys = sorted(R0)
    a, b = words(R0, keys), words(R1, keys)
    return int((a.view(np.uint64) != b.view(np.uint64)).sum()), a.size


def subnormal_cells(R):
    a = np.abs(words(R, sorted(R)))
    return int(((a > 0.0) & (a < SUBNORMAL_MAX)).sum())


def edge_conditions(name, R0, S0, R1, S1, values, R2, S2):
    """what the R = 2 case of table `name` must show, on the restatement's own numbers: R0, S0 planted, R1, S1 after the 3 alternating iterations of
    EDGE_W with their `values`, R2, S2 after the simultaneous one.  Measured on the CPU alone (tests/test_full_chance_cfr_ref.py runs it there)"""
    keys = sorted(R1)
    changed, total = changed_words(R0, R1)
    assert set(R0) == set(R1) and 4 * changed >= total, (name, changed, total)          # every table moves at least a quarter of the regret words
    if name.startswith("subnormal"):
        assert subnormal_cells(R1) > 0 and subnormal_cells(R2) > 0
    if name == "huge":
        assert np.isnan(values[0]).all() and np.isfinite(values[1:]).all(), values
        assert np.isnan(words(R1, keys)).any() and np.isnan(words(S1, keys)).any()
    if name == "huge_finite":
        assert np.isfinite(values).all() and all(np.isfinite(words(t, keys)).all() for t in (R0, S0, R1, S1, R2, S2))
    if name == "allneg":
        assert any(max(R0[k]) <= 0.0 and max(R1[k]) <= 0.0 and R1[k] != R0[k] for k in keys)


def assert_tables(h, R_ref, S_ref, what, loose=False):
    if not loose:
        return assert_tables_bits(h, R_ref, S_ref, what)
    keys, n_act, R, S = h.tables_get()
    k_ref = sorted(R_ref)
    assert sorted(S_ref) == k_ref and keys.tolist() == [list(k) for k in k_ref], f"{what}: pair sets differ ({keys.shape[0]} rows against {len(k_ref)})"
    assert n_act.tolist() == [W.key_actions(k) for k in k_ref]
    assert same(R, words(R_ref, k_ref), True), f"{what}: regret rows differ"
    assert same(S, words(S_ref, k_ref), True), f"{what}: strategy rows differ"


def step(h, tree, n_iters, weights, alternating, what, loose=False, root=None):
    """one cfr_iterate call checked against the restatement fed with tables_get taken just before it -> (values, R_ref, S_ref)"""
    tR, tS = tables_of(h)
    t0 = time.perf_counter()
    values = h.cfr_iterate(n_iters, weights, alternating, root)
    t1 = time.perf_counter()
    R_ref, S_ref, v_ref = CFR.iterate(tree, tR, tS, np.ones((n_iters, 3)) if weights is None else weights, alternating)
    CLOCK["device"] += t1 - t0
    CLOCK["cpu"] += time.perf_counter() - t1
    assert same(values, v_ref, loose), f"{what}: sweep values {values} against {v_ref}"
    assert_tables(h, R_ref, S_ref, what, loose)
    return values, R_ref, S_ref


def assert_exploitability(h, tree, what, root=None):
    tR, tS = tables_of(h)
    for which in (0, 1):
        t0 = time.perf_counter()
        got = out4_of(h.exploitability(root, which))
        t1 = time.perf_counter()
        want = X.solve(tree, tR, tS, which)["out4"]
        CLOCK["device"] += t1 - t0
        CLOCK["cpu"] += time.perf_counter() - t1
        assert same_bits(got, want), f"{what}, which {which}: {got} against {want}"


def handle(ctx, sl, decks, acts, capacity_log2):
    ctx.mccfr_seed(SEED)
    return sl.FullChanceMCCFR(ctx, decks, state_of(sl, decks[0], acts), capacity_log2)


def segments_and_spans(tree):
    """(the most nodes any pair holds in one level, the most decks any pair's nodes lie on) of a forest"""
    longest, spans = 0, {}
    for d, (_, n, ks) in enumerate(tree[0]):
        counts = {}
        for g, k in enumerate(ks or ()):
            counts[k] = counts.get(k, 0) + 1
            spans.setdefault(k, set()).add(X.deck_of(tree, d, g))
        longest = max([longest] + list(counts.values()))
    return longest, max(len(v) for v in spans.values())


@pytest.fixture(autouse=True)
def clock(request):
    CLOCK["device"] = CLOCK["cpu"] = 0.0
    yield
    print(f"\n{request.node.name}: device calls {CLOCK['device']:.3f} s, restatement {CLOCK['cpu']:.3f} s")


# ---- 1. edge tables on every pair ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TABLES)
@pytest.mark.parametrize("R", [2, 1])
def test_edge_tables_on_every_pair(ctx, sl, oracle, R, name):
    decks, acts, st = shape(oracle, R)
    tree = tree_of(st, decks, R)
    pairs = level_pairs(tree)
    h = handle(ctx, sl, decks, acts, 14)
    R0, S0 = edge_tables(pairs, name)
    plant(h, R0, S0)
    assert h.counters()["rows"] == len(pairs) == len(R0)
    loose, exact = name in LOOSE, name not in LOOSE
    if exact:
        assert_exploitability(h, tree, f"{name} planted, R {R}")
    values, R1, S1 = step(h, tree, 3, EDGE_W, 1, f"{name}, R {R}, alternating", loose)
    _, R2, S2 = step(h, tree, 1, np.ones((1, 3)), 0, f"{name}, R {R}, simultaneous", loose)
    assert h.counters()["rows"] == len(pairs) and h.counters()["dropped"] == 0
    if exact:
        assert_exploitability(h, tree, f"{name} after the iterations, R {R}")
    if R == 2:
        edge_conditions(name, R0, S0, R1, S1, values, R2, S2)
    else:
        assert changed_words(R0, R1)[0] > 0


@pytest.mark.parametrize("name", R3_TABLES)
def test_edge_tables_at_r3(ctx, sl, oracle, name):
    """planted rows at R = 3: segments longer than a wavefront whose nodes carry differing sigma and reach"""
    decks, acts, st = shape(oracle, 3)
    tree = tree_of(st, decks, 3)
    h = handle(ctx, sl, decks, acts, 18)
    R0, S0 = edge_tables(level_pairs(tree), name, tree)
    plant(h, R0, S0)
    values, R1, _ = step(h, tree, 2, weights_of("dcfr", 0, 2), 0, f"{name}, R 3", name in LOOSE)
    assert changed_words(R0, R1)[0] > 0 and segments_and_spans(tree)[0] > 64
    if name == "mixed":
        assert len(R0) < len(level_pairs(tree)) and len({tuple(F.sigma_of(r, W.key_actions(k))) for k, r in R0.items()}) > 3
        assert_exploitability(h, tree, "mixed after the iterations, R 3")


# ---- 2. wide and degenerate deck sets -----------------------------------------------------------------------------------------------------------------
def test_300_decks_with_one_round_to_go(ctx, sl, oracle):
    """a root level of 300 lanes across two workgroups (levels of 300, 900, 2700 and 5400 nodes), a mean over 300 roots"""
    decks, acts, st = packet(oracle, 5, 300, None)
    tree = tree_of(st, decks, 1)
    assert [len(ks) for _, n, ks in tree[0] if n > 1] == [300, 900, 2700, 5400]
    longest, span = segments_and_spans(tree)
    assert longest >= 64 and span >= 32, (longest, span)
    a, b = handle(ctx, sl, decks, acts, 15), handle(ctx, sl, decks, acts, 15)
    step(a, tree, 3, weights_of("dcfr", 0, 3), 1, "300 decks, alternating")
    step(b, tree, 3, weights_of("dcfr", 0, 3), 0, "300 decks, simultaneous")
    assert a.counters()["rows"] == len(level_pairs(tree))
    plant(b, *planted_tables(tree, "mixed"))
    step(b, tree, 2, weights_of("dcfr", 3, 2), 1, "300 decks, mixed rows planted")
    assert_exploitability(b, tree, "300 decks")


def test_70_decks_with_two_rounds_to_go(ctx, sl, oracle):
    """more roots than a wavefront and than the benchmark's 64; pairs that every deck holds"""
    decks, acts, st = packet(oracle, 4, 70, 0)
    tree = tree_of(st, decks, 2)
    longest, span = segments_and_spans(tree)
    assert span == 70 and longest >= 128, (longest, span)
    h = handle(ctx, sl, decks, acts, 16)
    step(h, tree, 2, weights_of("dcfr", 0, 2), 1, "70 decks, alternating")
    assert_exploitability(h, tree, "70 decks after 2 iterations")
    h.reset()
    plant(h, *planted_tables(tree, "mixed"))
    step(h, tree, 1, weights_of("dcfr", 2, 1), 0, "70 decks, mixed rows planted")
    assert_exploitability(h, tree, "70 decks, mixed rows planted")


@pytest.mark.parametrize("R", [1, 2])
def test_one_deck(ctx, sl, oracle, R):
    """the chance move is degenerate: the mean of one root"""
    decks, acts, st = shape(oracle, R)
    tree = tree_of(st, decks[:1], R)
    h = handle(ctx, sl, decks[:1], acts, 12)
    step(h, tree, 3, weights_of("dcfr", 0, 3), 1, f"one deck, R {R}")
    assert h.counters()["rows"] == len(level_pairs(tree))
    step(h, tree, 2, weights_of("cfr+", 3, 2), 0, f"one deck, R {R}, simultaneous")
    assert_exploitability(h, tree, f"one deck, R {R}")


def test_deck_order_defines_the_bits(ctx, sl, oracle):
    """two handles over the same 5 decks in another order: each equals the restatement for its own order, and where the two restatements differ the
    devices differ in the same words"""
    decks, acts, st = shape(oracle, 2)
    order = [3, 0, 4, 2, 1]
    other = np.ascontiguousarray(decks[order])
    w = weights_of("dcfr", 0, 3)
    out = []
    for d in (decks, other):
        tree = tree_of(st, d, 2)
        h = handle(ctx, sl, d, acts, 14)                                            # (a packet's decks share every card played before the root)
        values, R1, S1 = step(h, tree, 3, w, 1, "a deck order")
        out.append((values, h.tables_get(), R1))
    (va, ta, Ra), (vb, tb, Rb) = out
    keys = sorted(Ra)
    assert sorted(Rb) == keys and np.array_equal(ta[0], tb[0])
    cpu_same = same_bits(words(Ra, keys), words(Rb, keys))
    assert same_bits(ta[2], tb[2]) == cpu_same and same_bits(va, vb) == same_bits(*[CFR.iterate(tree_of(st, d, 2), {}, {}, w, 1)[2] for d in (decks, other)])
    print("the two deck orders give", "the same" if cpu_same else "different", "regret bits on the CPU, and so on the device")


# ---- 3. long runs and scratch growth -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,alternating", [("dcfr", 1), ("cfr+", 0)])
def test_150_iterations_in_one_call(ctx, sl, oracle, variant, alternating):
    """the offsets into the weights (3 t) and values (2 t) and the schedule far from t = 0; 1 + 149 on a second handle gives the same bits"""
    decks, acts, st = packet(oracle, 5, 300, None)
    decks = decks[:40]
    tree = tree_of(st, decks, 1)
    w = weights_of(variant, 0, 150)
    assert len({tuple(x) for x in w.tolist()}) == 150
    a, b = handle(ctx, sl, decks, acts, 13), handle(ctx, sl, decks, acts, 13)
    values, _, _ = step(a, tree, 150, w, alternating, f"150 iterations, {variant}")
    assert values.shape == (150, 2) and not same_bits(values[0], values[64]) and not same_bits(values[0], values[128])   # (slot t & 63 would show)
    t0 = time.perf_counter()
    vb = np.concatenate([b.cfr_iterate(1, w[:1], alternating), b.cfr_iterate(149, w[1:], alternating)])
    CLOCK["device"] += time.perf_counter() - t0
    assert same_bits(values, vb) and all(x.tobytes() == y.tobytes() for x, y in zip(a.tables_get(), b.tables_get()))
    assert a.counters() == b.counters() and a.counters()["iterations"] == 300


def test_scratch_grows_by_forest_and_by_iterations(ctx, sl, oracle):
    """one handle: a small forest first, then a larger one (the scratch is freed, allocated anew and every pointer laid out again), then more iterations
    (the weights and values parts grow), then small layouts inside the large buffer; the exploitability sweep's own scratch grows the same way"""
    decks, acts5, st5 = packet(oracle, 5, 6, None)
    train = decks[:3]
    st4 = F.root_of(decks[0], acts5[:24])
    tree2, tree1 = tree_of(st4, train, 2), tree_of(st5, train, 1)
    root5 = state_of(sl, decks[0], acts5)
    h = handle(ctx, sl, train, acts5[:24], 14)
    w = weights_of("dcfr", 0, 71)

    def both_roots(what):
        assert_exploitability(h, tree1, f"{what}, the round-5 root", root=root5)
        assert_exploitability(h, tree2, f"{what}, the handle's root")

    step(h, tree1, 1, w[:1], 1, "call 1: R = 1, 1 iteration", root=root5)
    both_roots("after call 1")
    step(h, tree2, 1, w[1:2], 1, "call 2: R = 2, the forest grows")
    step(h, tree2, 64, w[2:66], 0, "call 3: 64 iterations, the weights and values grow")
    both_roots("after call 3")
    step(h, tree1, 2, w[66:68], 1, "call 4: R = 1 inside the large buffer", root=root5)
    both_roots("after call 4")
    step(h, tree2, 3, w[68:71], 1, "call 5: R = 2, 3 iterations")
    assert h.counters()["iterations"] == 2 * 71 and h.counters()["dropped"] == 0


# ---- 4. the cap and R = 4, device against device --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r0,n", [(3, (1 << 22) // 36 ** 3), (2, 2)])
def test_cap_and_r4_against_the_exploitability_sweep(ctx, sl, oracle, r0, n):
    """89 decks at R = 3 (the cap: levels of up to 2 million nodes, the sorts' large-size path) and 2 decks at R = 4.  The restatement is too slow here
    (minutes for the tree alone), so the iteration is held to the project's INDEPENDENT exploitability sweep on the same device: the first sweep's
    value is the value pass of the store's sigma before the call, the rows claimed are the pairs the response reduce counts, and the rows the first
    call stored, read back through the store by the exploitability kernels, give the value the second call's compact rows give"""
    assert n == (89 if r0 == 3 else 2)
    decks, acts, _ = packet(oracle, r0, n, 0)
    times = {}

    def timed(what, fn, *args):
        t0 = time.perf_counter()
        out = fn(*args)
        times[what] = time.perf_counter() - t0
        CLOCK["device"] += times[what]
        return out

    probe = handle(ctx, sl, decks, acts, 4)
    before = timed("exploitability, empty store", probe.exploitability)
    P = probe.response_get(0)[0].shape[0] + probe.response_get(1)[0].shape[0]
    del probe
    c = next(c for c in range(4, 31) if 4 * P <= 1 << c)
    runs = []
    for i in range(2):
        h = handle(ctx, sl, decks, acts, c)
        before1 = h.exploitability(None, 1)["value"]
        v = timed("cfr_iterate 1", h.cfr_iterate, 1, weights_of("dcfr", 0, 1), 1)
        rows = h.counters()
        assert same_bits(v[0, 0], before1) and same_bits(before1, before["value"])
        assert rows["rows"] == P and rows["dropped"] == 0, (rows, P)
        e = timed("exploitability, which 1", h.exploitability, None, 1)
        v2 = timed("cfr_iterate 2", h.cfr_iterate, 1, weights_of("dcfr", 1, 1), 1)
        assert same_bits(v2[0, 0], e["value"]), (v2, e)
        four = np.concatenate([v.ravel(), v2.ravel()])
        assert np.isfinite(four).all() and (np.abs(four) <= 22.0).all(), four
        assert not same_bits(v[0, 0], v[0, 1]) and not same_bits(v2[0, 0], v[0, 1]) and h.counters()["rows"] == P
        runs.append((v, v2, h.counters()))
        del h
    assert same_bits(runs[0][0], runs[1][0]) and same_bits(runs[0][1], runs[1][1]) and runs[0][2] == runs[1][2]
    print(f"\nround-{r0} root, {n} decks: P = {P} pairs, capacity_log2 = {c}; " + ", ".join(f"{k} {t:.3f} s" for k, t in times.items()))
