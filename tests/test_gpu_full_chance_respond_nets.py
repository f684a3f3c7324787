"""GPU checks of the sampled best response to the Deep CFR nets on FullScopa over decks (k_frn_claim, k_frn_expand, k_frn_step, k_frn_up in
scopa_amd/csrc/scopa_full_chance_sdcfr.hip; scopa_full_chance_respond_nets_traverse / _iterate of include/scopa.h; FullChanceDeepCFR.sampled_response
and .sampled_lower_bound) against the store route (respond_traverse on policy_store(), where a store of the nets' policy fits), the depth-first
restatement tests/full_chance_respond_ref.py and the level-by-level restatement tests/full_chance_respond_nets_ref.py, which
tests/test_full_chance_respond_nets_ref.py holds to the depth-first one on bits.

The standard is tests/test_gpu_full_chance_respond.py's (assert_response_delta): pair set, visit counts and counters exact, d_strategy all zero, no
pair of the opponent claimed, a d_regret row met once bit-identical, the rest within the reorder budget (in_budget, K_REORDER of
oracle/mccfr_edges.py).  The restatement is fed the DEVICE's own average rows (average_at), so no draw is ambiguous.  Shapes are the frontier suite's:
R = 1 on 3 decks, R = 2 on 5, R = 3 on 2, nb 1 and 5, snapshot counts 0, 1 and 3."""
import numpy as np
import pytest
import torch

import full_chance_ref as X
import full_chance_respond_nets_ref as N
import full_chance_respond_ref as Q
import full_mccfr_ref as F
import mccfr_edges as E

from test_gpu_full_chance_net_match import Snaps, XAVIER3, average_at, beyond, deep_on, handle
from test_gpu_full_chance_respond import assert_response_delta, rows_of
from test_gpu_full_chance_sdcfr import SEED, SHAPES, packet, raises, state_of
from test_gpu_full_mccfr import in_budget, same_bits

pytestmark = pytest.mark.gpu

NO_SNAPSHOTS = ([], [0] * 6, 0, 0)
PER_PATH, PER_ROW = 2 * 64 + 16 + 24 + 2 * 8, 24 + 4        # bytes of scratch a path and a responder row take (include/scopa.h, respond_nets, 5)
_REF = {}


def per_traversal(R):
    return 6 ** R * PER_PATH + 4 * (6 ** R - 1) // 5 * PER_ROW


def device_fn(ctx, sets):
    """probs_at of the restatement from the device's own rows: sets[player] is a Snaps"""
    return lambda keys2, player: average_at(ctx, sets[player], keys2, player)


def ref_of(name, build):
    """a restatement computed once and left unchanged"""
    if name not in _REF:
        _REF[name] = build()
    return _REF[name]


def visits(h):
    c = h.counters()
    return c["choice_visits"], c["terminal_visits"]


def fresh(sl, ctx, decks, root, capacity_log2=14):
    ctx.mccfr_seed(SEED)
    return sl.FullChanceMCCFR(ctx, decks, root, capacity_log2)


# ---- 1. the same walk as the store route ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 2])
def test_same_walk_as_the_store_route(sl, oracle, R):
    """where a store of the nets' policy fits, respond_nets_traverse and respond_traverse(policy_store(), which 0, cut 0) are held, both, to both
    restatements: the depth-first one reading the store's rows, the level-by-level one fed average_at"""
    r0, n, fix = SHAPES[R]
    decks, acts, st = packet(oracle, r0, n, fix)
    d, t, c = deep_on(sl, decks, acts, 3)
    store = d.policy_store()
    root = state_of(sl, decks[0], acts)
    nets_h, store_h = fresh(sl, c, decks, root), fresh(sl, c, decks, root)
    store_h.cut(0)
    sets = [d._snapshot_set(p) for p in range(2)]
    try:
        opp_rows = rows_of(store.solver)
        for resp in (0, 1):
            for nb in (1, 5):
                refs = [X.Rows(), X.Rows()]
                Q.traverse(st, decks, resp, 2, 0, nb, SEED, refs[0], opp_rows, 0)
                N.traverse(st, decks, resp, 2, 0, nb, SEED, refs[1], d.average_policy_at)
                assert (refs[0].choice, refs[0].terminal) == (refs[1].choice, refs[1].terminal) == (n * nb * F.shape_counts(r0)[resp], n * nb * 6 ** R)
                for h, route in ((nets_h, "nets"), (store_h, "store")):
                    before = visits(h)
                    h.reset()
                    if route == "nets":
                        h.respond_nets_traverse(resp, sets[1 - resp][0], 2, 0, nb)
                    else:
                        h.respond_traverse(store.solver, 0, resp, 2, 0, nb)
                    for ref, against in zip(refs, ("the depth-first restatement", "the level restatement")):
                        keys, counts = assert_response_delta(h, ref, resp, f"R {R}, responder {resp}, nb {nb}, {route} route against {against}")
                    after = h.counters()
                    assert (after["choice_visits"] - before[0], after["terminal_visits"] - before[1]) == (refs[0].choice, refs[0].terminal)
                    assert (after["rows"], after["dropped"], after["iterations"]) == (counts.size, 0, 0)
                    got = h.tables_get()
                    assert not got[2].any() and not got[3].any()           # increments only
    finally:
        del sets
        for x in (nets_h, store_h, store, d, t, c):
            x.close()


# ---- 2. no snapshots is uniform play ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 2])
def test_no_snapshots_is_uniform_play(ctx, sl, oracle, R):
    r0, n, fix = SHAPES[R]
    h, decks, acts, st = handle(ctx, sl, oracle, r0, n, fix, capacity_log2=14)
    u = fresh(sl, ctx, decks, state_of(sl, decks[0], acts))
    u.cut(0)
    for resp in (0, 1):
        for nb in (1, 5):
            rows = X.Rows()
            Q.traverse(st, decks, resp, 1, 3, nb, SEED, rows)
            h.reset()
            u.reset()
            h.respond_nets_traverse(resp, NO_SNAPSHOTS, 1, 3, nb)
            u.respond_traverse(None, 0, resp, 1, 3, nb)
            assert_response_delta(h, rows, resp, f"R {R}, responder {resp}, nb {nb}: no snapshots")
            assert_response_delta(u, rows, resp, f"R {R}, responder {resp}, nb {nb}: uniform play")
            a, b = h.delta_get(), u.delta_get()
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and same_bits(a[2][a[1] <= 2], b[2][b[1] <= 2])   # (two adds commute)
    assert visits(h) == visits(u)


# ---- 3. chunk seams and lists --------------------------------------------------------------------------------------------------------------------------------
def test_chunk_seams_and_lists(ctx, sl, oracle):
    R, resp, nb = 2, 1, 2
    r0, n, fix = SHAPES[R]
    h, decks, acts, st = handle(ctx, sl, oracle, r0, n, fix, capacity_log2=14)
    sets = [Snaps(XAVIER3(40)), Snaps(XAVIER3(50))]
    fn = device_fn(ctx, sets)
    opp = sets[1 - resp].args

    def ref(listed):
        rows = X.Rows()
        N.traverse(st, decks, resp, 4, 7, nb, SEED, rows, fn, listed)
        return rows

    full = ref(None)
    got = []
    try:
        for budget in (0, per_traversal(R), 3 * per_traversal(R) + 5):     # one chunk; 10 chunks of 1; chunks of 3, 3, 3, 1
            h.debug_sdcfr_scratch(budget)
            h.reset()
            h.respond_nets_traverse(resp, opp, 4, 7, nb)
            assert_response_delta(h, full, resp, f"budget {budget}")
            got.append(h.delta_get())
        h.debug_sdcfr_scratch(per_traversal(R) - 1)
        raises(sl, sl.SCOPA_EINVAL, h.respond_nets_traverse, resp, opp, 4, 7, nb)   # a budget below one traversal
        h.debug_sdcfr_scratch(3 * per_traversal(R))
        part = ref((0, 2, 3))
        assert set(part.count) < set(full.count)
        for listed in ([0, 2, 3], [3, 0, 2]):                              # a permuted list, m < n, across chunk seams: no draw of a listed deck changes
            h.reset()
            h.respond_nets_traverse(resp, opp, 4, 7, nb, listed)
            assert_response_delta(h, part, resp, f"list {listed}")
            got.append(h.delta_get())
        h.debug_sdcfr_scratch(0)
        alone = ref((4,))                                                  # the deck INDEX reaches the tag: deck 4 listed alone draws what it draws in the full set
        h.reset()
        h.respond_nets_traverse(resp, opp, 4, 7, nb, [4])
        assert_response_delta(h, alone, resp, "deck 4 alone")
        wrong = X.Rows()
        N.traverse(st, decks[4:], resp, 4, 7, nb, SEED, wrong, fn)          # (the guard: the same deck at index 0 draws otherwise)
        assert wrong.arrays("count")[1].tolist() != alone.arrays("count")[1].tolist() or wrong.arrays("count")[0].tolist() != alone.arrays("count")[0].tolist()
        before = h.delta_get()
        h.respond_nets_traverse(resp, opp, 4, 7, nb, [])                   # an empty list is a no-op
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before, h.delta_get()))
    finally:
        h.debug_sdcfr_scratch(0)
    for g in got[1:3]:
        assert np.array_equal(got[0][0], g[0]) and np.array_equal(got[0][1], g[1])
    assert np.array_equal(got[3][0], got[4][0]) and np.array_equal(got[3][1], got[4][1])


# ---- 4. beyond the sweeps --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resp", [0, 1])
@pytest.mark.parametrize("r0,nb", [(1, 2), (0, 1)])
def test_beyond_the_sweeps(ctx, sl, oracle, r0, nb, resp):
    """R = 5 on 2 decks at nb = 2 and the deal on 2 decks at nb = 1, 3 Xavier snapshots: against the level restatement fed by the device's rows"""
    small, decks3, st = beyond(ctx, sl, oracle, r0)
    decks = decks3[:2]
    h = fresh(sl, ctx, decks, small.root, 19)
    sets = [Snaps(XAVIER3(40)), Snaps(XAVIER3(50))]

    def build():
        rows = X.Rows()
        N.traverse(st, decks, resp, 1, 0, nb, SEED, rows, device_fn(ctx, sets))
        return rows

    rows = ref_of(("beyond", r0, nb, resp), build)
    R = 6 - r0
    assert (rows.choice, rows.terminal) == (2 * nb * F.shape_counts(r0)[resp], 2 * nb * 6 ** R)
    h.respond_nets_traverse(resp, sets[1 - resp].args, 1, 0, nb)
    keys, counts = assert_response_delta(h, rows, resp, f"round {r0}, responder {resp}, nb {nb}")
    c = h.counters()
    assert (c["choice_visits"], c["terminal_visits"], c["dropped"], c["rows"]) == (rows.choice, rows.terminal, 0, keys.shape[0])
    assert counts.sum() == 2 * nb * 4 * (6 ** R - 1) // 5                   # every responder node of every traversal updated its row
    h.close()


# ---- 5. iterate ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_iterate_is_the_call_sequence(ctx, sl, oracle):
    R = 2
    r0, n, fix = SHAPES[R]
    h1, decks, acts, st = handle(ctx, sl, oracle, r0, n, fix, capacity_log2=14)
    h2 = fresh(sl, ctx, decks, state_of(sl, decks[0], acts))
    sets = [Snaps(XAVIER3(40)), Snaps([XAVIER3(50)[0]])]                    # 3 snapshots and 1
    args = [s.args for s in sets]
    fn = device_fn(ctx, sets)
    lists = [[1, 3], [0, 2], [2, 1]]
    h1.respond_nets_iterate(args, 2, 3, lists=lists)
    ref, A, counter = X.Rows(), {}, 0
    for t, lst in enumerate(lists):
        for r in range(2):
            h2.respond_nets_traverse(r, args[1 - r], 2 * t + r, 0, 2, lst)
            h2.apply()
            N.traverse(st, decks, r, counter, 0, 2, SEED, ref, fn, lst)
            for k, a in ref.A.items():
                A[k] = [x + y for x, y in zip(A.get(k, [0.0] * 3), a)]
            ref.apply()
            counter += 1
    assert h1.counters() == h2.counters() and h1.counters()["iterations"] == 6 and h1.counters()["dropped"] == 0
    assert h1.counters()["choice_visits"] == 3 * 2 * 2 * sum(F.shape_counts(r0)[:2])
    t1, t2 = h1.tables_get(), h2.tables_get()
    k_ref, R_ref = ref.arrays("R")
    assert np.array_equal(t1[0], t2[0]) and np.array_equal(t1[0], k_ref) and not t1[3].any() and not t2[3].any()
    assert not h1.delta_get()[1].any() and not h1.delta_get()[2].any()
    # six launches deep a later sigma reads regrets that carry an earlier launch's reorder error, so the bound is the suite's for a run of launches
    # (tests/ctx_lifecycle.py): 100 x the launch budget over the |increment| sums of all launches + 100 x launches x eps |R|
    A_rows = np.array([A[tuple(k)] for k in k_ref.tolist()]).reshape(-1, 3)
    bound = 100 * E.K_REORDER * E.EPS * A_rows.sum(1)[:, None] + 100 * 6 * E.EPS * np.abs(R_ref)
    for name, tab in (("iterate", t1), ("the call sequence", t2)):
        err = np.abs(tab[2] - R_ref)
        print(name, "largest regret error / bound:", float(np.where(err == 0.0, 0.0, err / np.where(bound > 0, bound, 1.0)).max()))
        assert (err <= bound).all(), name
    # two identical runs from reset, nb = 1 on one listed deck, one iteration: the tree walked does not depend on the responder's rows, so the
    # restatement's visit counts per launch are the device's, and a row met at most twice in its launch carries the same bits (two adds commute)
    once = {}
    for r in range(2):
        rows = X.Rows()
        N.traverse(st, decks, r, r, 0, 1, SEED, rows, fn, [2])
        once.update({k: v <= 2 for k, v in rows.count.items()})
    runs = []
    for _ in range(2):                                                     # (fresh handles: the iteration counter is a Philox word)
        h = fresh(sl, ctx, decks, state_of(sl, decks[0], acts))
        h.respond_nets_iterate(args, 1, 1, lists=[[2]])
        runs.append(h.tables_get())
        assert h.counters()["iterations"] == 2
        h.close()
    assert np.array_equal(runs[0][0], runs[1][0]) and sorted(once) == [tuple(k) for k in runs[0][0].tolist()]
    pick = np.array([once[tuple(k)] for k in runs[0][0].tolist()])
    assert pick.sum() > 10 and same_bits(runs[0][2][pick], runs[1][2][pick]) and runs[0][2][pick].any()


# ---- 6. the bound at one round to go --------------------------------------------------------------------------------------------------------------------------------
def row_gaps(keys, R):
    """best minus second regret over every row's legal slots"""
    out = np.zeros(len(keys))
    for i, (k, r) in enumerate(zip(keys.tolist(), R)):
        top = sorted(r[:X.key_actions(k)], reverse=True)
        out[i] = top[0] - top[1]
    return out


def test_the_bound_at_one_round_to_go(sl, oracle):
    """Round-5 root, 3 decks (SHAPES[1]), deep_on's nets of 3 snapshots; the nets route and the store route (respond_iterate on policy_store()) step
    side by side, one iteration at batch 48 at a time, hardened after each.
    (a) what either hardened responder wins, exactly (cross_play), is at most BR_p of policy_store().exploitability() + 1e-9: at R = 1 the sweep's
        response IS the best response.
    (b) the two routes' hardened rows are equal except at rows whose best-minus-second regret on the store route's table lies within the row's
        reorder budget (K_REORDER eps A_row + 2 eps |R|, A_row the |increment| sums of the level restatement run beside them).  Such rows are of two
        kinds.  Rows whose two best regrets are EQUAL in the restatement (Q.regret_gap's ties: two cards of one rank that score alike, the last
        two-card choice): 27 to 29 of the 72 rows here, a property of the game that no seed removes, and a flip there changes no value
        (tests/test_full_chance_respond_ref.py::test_bound_case_is_what_the_gpu_test_needs).  And rows whose POSITIVE gap is that small by
        coincidence: the restatement fed full_chance_sdcfr_ref's float64 average policy has none with deep_on's seeds at any of 16 iterations
        (smallest positive gap 0.25), so the seeds stay; on the device they may make up at most 1 % of the rows.  Both counts are printed.
    (c) at every iteration at which the store route attains BR_p to 1e-9 the nets route does: the float64 restatement attains both at iteration 3
        (and not again before iteration 15), so the store route is asserted to attain them at one of the 8 iterations at least."""
    from scopa_amd.algorithms.full_chance import cross_play
    r0, n, fix = SHAPES[1]
    decks, acts, st = packet(oracle, r0, n, fix)
    d, t, c = deep_on(sl, decks, acts, 3)
    store = d.policy_store()
    from scopa_amd.algorithms import FullChanceMCCFRTrainer
    routes = [FullChanceMCCFRTrainer(decks=decks, root_actions=acts, capacity_log2=12, batch=48, ctx=c) for _ in range(2)]
    sets = [d._snapshot_set(p) for p in range(2)]
    try:
        e = store.exploitability()
        ref, A, counter, attained = X.Rows(), {}, 0, []
        for it in range(1, 9):
            routes[0].solver.respond_nets_iterate([s[0] for s in sets], 48, 1)
            routes[1].solver.respond_iterate(store.solver, 0, 48, 1)
            for resp in range(2):
                N.traverse(st, decks, resp, counter, 0, 48, SEED, ref, d.average_policy_at)
                for k, a in ref.A.items():
                    A[k] = [x + y for x, y in zip(A.get(k, [0.0] * 3), a)]
                ref.apply()
                counter += 1
            won = []
            for r in routes:
                r.solver.harden()
                v0 = cross_play([r, store])[0][1][0]
                v1 = -cross_play([store, r])[0][1][0]
                assert v0 <= e["br0"] + 1e-9 and v1 <= e["br1"] + 1e-9, it                                   # (a)
                won.append((v0, v1))
            print(f"iteration {it}: nets route wins {won[0]}, store route {won[1]} of ({e['br0']}, {e['br1']})")
            tabs = [r.solver.tables_get() for r in routes]
            assert np.array_equal(tabs[0][0], tabs[1][0]) and np.array_equal(tabs[0][0], ref.arrays("R")[0])
            keys, R_store = tabs[1][0], tabs[1][2]
            A_rows = np.array([A[tuple(k)] for k in keys.tolist()]).reshape(-1, 3)
            budget = E.K_REORDER * E.EPS * A_rows.sum(1) + 2.0 * E.EPS * np.abs(R_store).max(1)
            close = row_gaps(keys, R_store) <= budget
            tied = {k for k, _, _ in Q.regret_gap(ref)[1]}
            is_tied = np.array([tuple(k) in tied for k in keys.tolist()])
            differ = (tabs[0][3] != tabs[1][3]).any(1)
            print(f"iteration {it}: {len(keys)} rows, {int((close & is_tied).sum())} tied in the restatement, {int((close & ~is_tied).sum())} within the "
                  f"budget by coincidence, {int(differ.sum())} hardened rows differ between the routes")
            assert not (differ & ~close).any(), it                                                            # (b)
            assert (close & ~is_tied).sum() <= 0.01 * len(keys), it
            assert ((tabs[0][3] == 0.0) | (tabs[0][3] == 1.0)).all() and (tabs[0][3].sum(1) == 1.0).all()
            if abs(won[1][0] - e["br0"]) <= 1e-9 and abs(won[1][1] - e["br1"]) <= 1e-9:                       # (c)
                attained.append(it)
                assert abs(won[0][0] - e["br0"]) <= 1e-9 and abs(won[0][1] - e["br1"]) <= 1e-9, it
        print("the store route attains both values at iterations", attained)
        assert attained
    finally:
        del sets
        for x in routes + [store, d, t, c]:
            x.close()


# ---- 7. the Python interface ------------------------------------------------------------------------------------------------------------------------------------------
def nets_bytes(d):
    out = []
    for buf in d.strategy_buffers:
        out += [list(buf._slots), list(buf.weights)] + ([] if buf._store is None else [t.cpu().numpy().tobytes() for t in buf._store])
    return out


def with_snapshots(d, n_snap=3):
    from full_chance_sdcfr_ref import xavier_net
    with torch.cuda.stream(d._stream):
        for player in (0, 1):
            for it in range(n_snap):
                d.strategy_buffers[player].add_strategy(None, it + 1, params=[torch.tensor(a, device="cuda") for a in xavier_net(21 + it + 10 * player, head_bias=0.05 * it)])
    d._stream.synchronize()
    return d


def test_python_from_the_deal(sl, oracle):
    from scopa_amd.algorithms import packet_decks
    from scopa_amd.algorithms.deep_cfr import FullChanceDeepCFR
    decks = packet_decks(oracle.full_deal_py_seed(42), 0, 3, 5)
    d = with_snapshots(FullChanceDeepCFR(decks[:2], root_actions=(), traversal="frontier", batch=1, decks_per_iteration=1, seed=SEED))
    r = None
    try:
        before = nets_bytes(d)
        r = d.sampled_response(1, batch=1, capacity_log2=19)
        S = r.solver.tables_get()[3]
        assert r.counters()["iterations"] == 2 and r.counters()["dropped"] == 0 and len(S) > 10000
        assert (S.sum(1) == 1.0).all() and ((S == 0.0) | (S == 1.0)).all()
        assert r.solver.capacity_log2 == 19 and r.decks.shape == (2, 40) and np.array_equal(r.decks, decks[:2]) and r.root_actions == () and r.batch == 1
        r.solver.respond_nets_iterate([d._snapshot_set(p)[0] for p in range(2)], 1)                              # training goes on
        r.solver.harden()
        assert r.counters()["iterations"] == 4
        rep = d.sampled_lower_bound(1, 64, batch=1, capacity_log2=19)
        assert rep["lower_bound"] is True and rep["episodes"] == 64 and rep["exact_reward"] is None and rep["exact_by_seat"] is None
        assert rep["exact_std_error"] is None and all(s["exact_reward"] is None and s["episodes"] == 32 for s in rep["by_seat"]) and abs(rep["reward"]) <= 21
        held = d.sampled_lower_bound(1, 16, batch=1, capacity_log2=18, sample=1, decks=decks[2:])                 # a held-out deck
        assert held["lower_bound"] is True and abs(held["reward"]) <= 21
        with pytest.raises(ValueError, match="even"):
            d.sampled_lower_bound(1, 63, batch=1, capacity_log2=19)
        assert before == nets_bytes(d)
    finally:
        if r is not None:
            r.close()
        d.close()


def test_python_inside_the_sweeps(sl, oracle):
    r0, n, fix = SHAPES[1]
    decks, acts, st = packet(oracle, r0, n, fix)
    d, t, c = deep_on(sl, decks, acts, 3)
    try:
        before = nets_bytes(d)
        episodes = 3 << 13                                                  # n / 2 is a multiple of the 3 decks: the match's law is the exact target's
        rep = d.sampled_lower_bound(8, episodes, batch=48, capacity_log2=12)
        e = d.exploitability()
        print("sampled", rep["reward"], "+-", rep["std_error"], "exact value of the response", rep["exact_reward"], "+-", rep["exact_std_error"], "by seat",
              [s["reward"] for s in rep["by_seat"]], rep["exact_by_seat"], "exploitability", e)
        assert rep["lower_bound"] is True and rep["episodes"] == episodes
        for seat, s in enumerate(rep["by_seat"]):
            assert abs(s["reward"] - s["exact_reward"]) <= 5.0 * s["exact_std_error"], seat
            assert s["exact_reward"] <= e[f"br{seat}"] + 1e-9                # the responder's seat p value is at most BR_p
        assert abs(rep["reward"] - rep["exact_reward"]) <= 5.0 * rep["exact_std_error"]
        assert before == nets_bytes(d)
        with pytest.raises(ValueError, match="even"):
            d.sampled_lower_bound(1, 7)
    finally:
        for x in (d, t, c):
            x.close()


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(ctx, sl, oracle):
    R = 2
    r0, n, fix = SHAPES[R]
    h, decks, acts, st = handle(ctx, sl, oracle, r0, n, fix, capacity_log2=14)
    sets = [Snaps(XAVIER3(40)), Snaps(XAVIER3(50))]
    good = sets[1].args
    h.respond_nets_traverse(0, good, 0, 0, 2)                              # increments left standing
    before = (h.delta_get(), h.counters(), [t.cpu().numpy().tobytes() for s in sets for t in s.store])
    assert before[0][2].any()
    slots, ptrs, max_size, coef = good
    other = packet(oracle, r0, n, fix, deck_seed=7)
    mid = state_of(sl, decks[0], acts[:-1])                                # no round boundary
    bad_sets = [(slots, ptrs[:2] + [0] + ptrs[3:], max_size, coef), (slots, ptrs, max_size, 0), (slots, ptrs, 2, coef), ([1, 4, max_size], ptrs, max_size, coef),
                (list(range(max_size + 1)), ptrs, max_size, coef)]
    bad = [lambda: h.respond_nets_traverse(2, good, 0, 0, 1), lambda: h.respond_nets_traverse(-1, good, 0, 0, 1),     # responder outside {0, 1}
           lambda: h.respond_nets_traverse(0, good, 0, 0, 0), lambda: h.respond_nets_traverse(0, good, 0, 0, (1 << 24) + 1),   # nb
           lambda: h.respond_nets_traverse(0, good, 0, (1 << 32) - 1, 2),                                           # traversal ids beyond 2^32
           lambda: h.respond_nets_traverse(0, good, 0, 0, 1, [0, 2, 2]), lambda: h.respond_nets_traverse(0, good, 0, 0, 1, [0, 5]),
           lambda: h.respond_nets_traverse(0, good, 0, 0, 1, [-1]), lambda: h.respond_nets_traverse(0, good, 0, 0, 1, [0, 1, 2, 3, 4, 0]),
           lambda: h.respond_nets_traverse(0, good, 0, 0, 1, root=mid),
           lambda: h.respond_nets_traverse(0, good, 0, 0, 1, root=state_of(sl, other[0][0], other[1])),             # the handle's decks do not fit it
           lambda: h.respond_nets_iterate([good, good], 0), lambda: h.respond_nets_iterate([good, good], 1, 2, lists=[[0, 1], [2, 2]]),
           lambda: h.respond_nets_iterate([good, good], 1, (1 << 20) + 1)]
    bad += [lambda s=s: h.respond_nets_traverse(0, s, 0, 0, 1) for s in bad_sets]
    bad += [lambda s=s: h.respond_nets_iterate([good, s], 1) for s in bad_sets] + [lambda: h.respond_nets_iterate([bad_sets[0], good], 1)]
    for i, call in enumerate(bad):
        with pytest.raises(sl.ScopaError) as e:
            call()
        assert e.value.status == sl.SCOPA_EINVAL, i
    with pytest.raises(ValueError):
        h.respond_nets_iterate([good], 1)
    L = sl.lib()
    assert L.scopa_full_chance_respond_nets_traverse(None, None, 0, 1, None, 0, None, 0, 0) == sl.SCOPA_EINVAL
    assert L.scopa_full_chance_respond_nets_iterate(None, None, 1, 1, None, 0) == sl.SCOPA_EINVAL
    assert L.scopa_full_chance_respond_nets_traverse(h._h, None, 0, 1, None, 0, None, 0, 0) == sl.SCOPA_EINVAL      # a NULL set
    assert L.scopa_full_chance_respond_nets_iterate(h._h, None, 1, 1, None, 0) == sl.SCOPA_EINVAL
    try:
        h.debug_sdcfr_scratch(per_traversal(R) - 1)
        raises(sl, sl.SCOPA_EINVAL, h.respond_nets_iterate, [good, good], 1)
    finally:
        h.debug_sdcfr_scratch(0)
    after = (h.delta_get(), h.counters(), [t.cpu().numpy().tobytes() for s in sets for t in s.store])
    assert before[1] == after[1] and before[2] == after[2]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before[0], after[0]))
    # a too-small response store: rows are dropped and counted, nothing faults, the rows kept are right
    rows = X.Rows()
    N.traverse(st, decks, 0, 0, 0, 5, SEED, rows, device_fn(ctx, sets))
    want = dict(zip([tuple(k) for k in rows.arrays("count")[0].tolist()], rows.arrays("count")[1].tolist()))
    assert len(want) > (1 << 7)
    small = fresh(sl, ctx, decks, state_of(sl, decks[0], acts), 7)
    raises(sl, sl.SCOPA_ENOMEM, small.respond_nets_traverse, 0, good, 0, 0, 5)
    c = small.counters()                                                  # the process goes on
    assert c["dropped"] > 0 and c["rows"] <= (1 << 7) and (c["choice_visits"], c["terminal_visits"]) == (rows.choice, rows.terminal)
    keys, counts, _, dS = small.delta_get()
    assert keys.shape[0] == c["rows"] and not dS.any()
    for k, m in zip(keys.tolist(), counts.tolist()):
        assert m <= want[tuple(k)]                                        # (a pair the restatement never met is a KeyError)
    assert counts.sum() + c["dropped"] == sum(want.values())              # every visit of a responder's node either updated its row or was dropped
    small.harden()
    assert small.counters()["rows"] == c["rows"]
