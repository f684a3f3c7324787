"""Cached state of a long-lived scopa_ctx across table writers, deal changes and mode toggles.

A context keeps device-side caches behind host flags: the sigma | threshold rows of the batched MCCFR step (sigcdf_valid), the first-visit marks and
mccfr_all_seen, captured (traverse, apply) x k graphs, a caller-bound delta buffer, the exact-CFR schedule, the SDCFR node bits and policy table, the
evaluator's thresholds.  Each is right only if every entry point that moves the data it was derived from also drops it.  Every case here has one shape:
on ONE context run a mutator, then a consumer, and compare the consumer's output with the reference computed from scratch for the state the context
should be in -- oracle.Tree, tests/cfr_variants_ref.py, tests/xplay_ref.py -- and, where one can be built, with a second, fresh context brought to
the same state directly.  Comparisons are ctx_lifecycle.py's: bit equality for the deterministic kernels, the reorder budget of
tests/test_gpu_mccfr_edges.py for the batched MCCFR step, exact equality for counters and visit counts.

What the cases pin (include/scopa.h):
  * scopa_tables_set moves table contents, not visits: the first-visit marks (scopa_visited_get: "since the last reset") and with them
    mccfr_all_seen survive it; scopa_tables_reset clears both.
  * scopa_set_deal unbinds a caller-bound delta buffer BEFORE it resets the tables, so the reset never writes the new deal's row count into a buffer
    promised for the old one.
  * after scopa_set_deal and before a new launch the getters answer with the new deal's zero state (iteration 0, no marks, route -1) or refuse
    (scopa_sdcfr_policy_get, scopa_eval_tabular_match: SCOPA_ESTATE); scopa_counters counts since creation, so differences are taken.
conftest.py hands every test a context of its own, so no state can reach another test through it; each test still restores the modes it touched
(ctx_lifecycle.restore, in a finally), so that a wider fixture scope later would not turn these cases into a source of order dependence."""
import numpy as np
import pytest

import mccfr_edges as E
from cfr_edges import same_bits
from ctx_lifecycle import DEALS, DEFAULT_SEED, PAIR, check_iterations, counted, deal, oracle_iterations, restore, tree

pytestmark = pytest.mark.gpu

SEED = 77
BATCHES = (48, 1000)                    # one workgroup, and more than one
GRAPH_ITERS = (3, 70)                   # a chunk below 64, and a chunk boundary
N_DECISION, N_TERMINAL = 1653, 576


def _tables_bits(ctx, want, what):
    for name, a, b in zip(("regret", "strategy", "local"), ctx.tables_get(), want):
        assert same_bits(a, b), (what, name, np.argwhere(a.view(np.uint64) != np.asarray(b).view(np.uint64))[:4])


def _legal(t):
    return np.arange(4)[None, :] < t.infoset_nlegal[:, None]


# ---- 1. sigma rows after every regret writer ------------------------------------------------------------------------------------------------------
def _dcfr_weights():
    from scopa_amd.algorithms import schedule
    return schedule("dcfr", 0, 2, 1.5, 0.0, 2.0)


def _write(ctx, t, writer, R, S, L):
    """run `writer` on the context and on copies of (R, S, L); -> the tables the context must now hold, and whether the writer resets the iteration"""
    R, S, L = R.copy(), S.copy(), L.copy()
    if writer.startswith("set_"):
        R = E.edge_table(writer[4:], t.infoset_nlegal)
        ctx.tables_set(regret=R)
    elif writer == "reset":
        ctx.tables_reset()
        R, S, L = t.tables()
    elif writer == "exact_iterate":
        assert same_bits(ctx.cfr_exact_iterate(1), t.cfr_exact(R, S, L, 1))
    elif writer == "exact_traverse":
        assert ctx.cfr_exact_traverse(1) == t.cfr_exact_from(R, S, L, np.zeros(0, np.int32), 1, 1.0, 1.0)
    elif writer == "exact_traverse_from":
        assert ctx.cfr_exact_traverse_from(0, (1, 2, 0), 0.5, 0.25) == t.cfr_exact_from(R, S, L, (1, 2, 0), 0, 0.5, 0.25)
    elif writer == "sync":
        ctx.cfr_sync_iterate(1)
        t.cfr_sync(R, S, 1)
    elif writer == "sync_weighted":
        from cfr_variants_ref import Ref
        ctx.cfr_sync_iterate_weighted(_dcfr_weights(), alternating=True)
        Ref(t).run(R, S, _dcfr_weights(), alternating=True)
    elif writer == "replay":
        u = np.random.RandomState(0).random_sample(PAIR[0] * 3)      # the golden fixture's uniform stream (tests/golden/mccfr.npz, seed 0)
        assert ctx.mccfr_replay(3, u) == t.mccfr_replay(R, S, 3, u) == PAIR[0] * 3
    else:
        raise KeyError(writer)
    return R, S, L, writer == "reset"


WRITERS = ("set_onehot", "set_allneg", "set_small_large", "reset", "exact_iterate", "exact_traverse", "exact_traverse_from", "sync", "sync_weighted",
           "replay")
CONSUMERS = ("eager", "graph", "split", "apply_only", "sharded")


@pytest.mark.parametrize("consumer", CONSUMERS)
@pytest.mark.parametrize("writer", WRITERS)
def test_sigma_rows_after_every_regret_writer(ctx, sl, oracle, writer, consumer):
    """One batched iteration at batch 48 leaves valid sigma rows; then the writer; then each consumer of the rows, at batches 48 and 1000, against the
    oracle started from the written tables.  The graph consumer runs the same (batch, 3) on both sides of the writer: the second call replays a graph
    captured before the write.  The deterministic writers' tables are compared bit for bit first (the base state is read back from the device).
    One (writer, consumer) pair per case: two batches, at most six oracle iterations of 1000 pairs."""
    try:
        t = deal(ctx, sl, oracle, 42)
        ctx.mccfr_seed(SEED)
        for batch in BATCHES:
            what = (writer, consumer, batch)
            ctx.tables_reset()
            ctx.mccfr_delta_set(np.zeros((t.n_infosets, 5)))
            ctx.mccfr_iterate(48, 1)
            warm = 1
            if consumer == "graph":
                ctx.mccfr_graph_mode(True)
                ctx.mccfr_iterate(batch, 3)
                warm += 3
            assert ctx.mccfr_iteration() == warm, what
            R1, S1, L1 = ctx.tables_get()
            R2, S2, L2, zeroed = _write(ctx, t, writer, R1, S1, L1)
            _tables_bits(ctx, (R2, S2, L2), what)
            it = 0 if zeroed else warm
            assert ctx.mccfr_iteration() == it, what
            c0 = ctx.counters()
            if consumer in ("eager", "graph"):
                n = 2 if consumer == "eager" else 3
                ctx.mccfr_iterate(batch, n)
            elif consumer == "split":
                n = 1
                ctx.mccfr_traverse(it, 0, batch)
                ctx.mccfr_apply()
            elif consumer == "sharded":
                n = 1
                h = ctx.p2p_create(0, 1)
                ctx.p2p_connect(h.reshape(1, 64))
                ctx.mccfr_iterate_sharded(0, batch, 1)
                assert ctx.p2p_status()[0] == 0
                ctx.p2p_destroy()
            else:                                       # mccfr_apply alone on a hand-set delta: the !sigcdf_valid branch of the apply
                rng = np.random.RandomState(batch)
                D = np.zeros((t.n_infosets, 5))
                D[:, :4] = np.where(_legal(t), rng.standard_normal((t.n_infosets, 4)) * 3.0, 0.0)
                D[:, 4] = rng.randint(0, 5, t.n_infosets)
                ctx.mccfr_delta_set(D)
                ctx.mccfr_apply()
                Rg, Sg, Lg = ctx.tables_get()
                assert same_bits(Rg, R2 + D[:, :4]), what
                assert same_bits(Sg, S2 + D[:, 4:5] * E.reference_sigma(R2, t.infoset_nlegal)), what
                assert same_bits(Lg, L2) and not ctx.mccfr_delta_get().any() and ctx.mccfr_iteration() == it + 1, what
                assert ctx.counters() == c0, what
                continue
            ctx.mccfr_graph_mode(False)
            assert ctx.mccfr_iteration() == it + n, what
            counted(ctx, c0, batch * n, what)
            Rg, Sg, Lg = ctx.tables_get()
            assert same_bits(Lg, L2), what              # the batched step does not touch local_strategy
            check_iterations((Rg, Sg), t, R2, S2, SEED, it, n, batch, what, exact_strategy=consumer == "split")
    finally:
        restore(ctx, sl)


# ---- 2. first-visit tracking and the graph key ----------------------------------------------------------------------------------------------------
B2 = 256


def _until_all_seen(c, batch, k, limit):
    """graph-mode calls of (batch, k) until every infoset is marked and one more call has run with tracking off; -> calls made"""
    for call in range(1, limit + 1):
        c.mccfr_iterate(batch, k)
        if (c.visited_get() != 0).all():
            c.mccfr_iterate(batch, k)                       # the host counts the marks before this call's first chunk: tracking is off in it
            return call + 1
    raise AssertionError("the marks never completed")


@pytest.mark.parametrize("mutator", ["tables_reset", "tables_set"])
@pytest.mark.parametrize("k", GRAPH_ITERS)
def test_first_visit_tracking_and_the_graph_key(ctx, sl, oracle, mutator, k):
    """Graph-mode iterations until mccfr_all_seen flips (the track flag is a launch argument of the captured traversals and part of the graph key),
    then the mutator, then the same (batch, k) again.  Deal 42, batch 256 and the default seed: the run of
    test_mccfr_first_visit_tracking_switches_off_once_every_infoset_is_marked, whose 240 iterations mark all 738 infosets (on the oracle the
    251-infoset deal keeps one infoset unmarked through 4000 iterations of 48 pairs: no small run completes its marks).
    tables_reset clears the marks: tracking is on again, and marks, iteration number and counters equal a fresh context's after the same calls.
    The batched step adds its float64 increments in arrival order (memory-side atomics), so two runs of it are not bit-reproducible: the two
    contexts' tables are compared with each other within twice the budget each is held to against the oracle, not bit for bit.
    tables_set moves table contents, not visits (scopa_visited_get: 'since the last reset'): the marks stay complete and unchanged, and the tables
    equal the oracle's from the set tables."""
    fresh = None
    try:
        t = deal(ctx, sl, oracle, 42)
        ctx.mccfr_seed(DEFAULT_SEED)
        ctx.mccfr_graph_mode(True)
        calls = _until_all_seen(ctx, B2, k, limit=-(-240 // k) + 8)
        marks = ctx.visited_get().copy()
        assert (marks != 0).all() and ctx.mccfr_iteration() == calls * k
        if mutator == "tables_reset":
            ctx.tables_reset()
            assert not ctx.visited_get().any() and ctx.mccfr_iteration() == 0
            R0, S0, _ = t.tables()
        else:
            R0 = E.edge_table("small_large", t.infoset_nlegal)
            S0 = ctx.tables_get()[1]
            ctx.tables_set(regret=R0)
            assert np.array_equal(ctx.visited_get(), marks) and ctx.mccfr_iteration() == calls * k
        it = ctx.mccfr_iteration()
        c0 = ctx.counters()
        ctx.mccfr_iterate(B2, k)
        counted(ctx, c0, B2 * k, (mutator, k))
        assert ctx.mccfr_iteration() == it + k
        Rg, Sg, _ = ctx.tables_get()
        check_iterations((Rg, Sg), t, R0, S0, DEFAULT_SEED, it, k, B2, (mutator, k))
        if mutator == "tables_set":
            assert np.array_equal(ctx.visited_get(), marks)
        else:
            fresh = sl.Context(0)
            fresh.set_deal(sl.deal_py_seed(42))
            fresh.mccfr_seed(DEFAULT_SEED)
            fresh.mccfr_graph_mode(True)
            f0 = fresh.counters()
            fresh.mccfr_iterate(B2, k)
            assert np.array_equal(ctx.visited_get(), fresh.visited_get())       # 0x40000000 + id marks: a function of which infosets were seen
            assert 0 < int((ctx.visited_get() != 0).sum())
            counted(fresh, f0, B2 * k, "fresh context")
            Rf, Sf, _ = fresh.tables_get()
            tol = check_iterations((Rf, Sf), t, R0, S0, DEFAULT_SEED, 0, k, B2, "fresh context")
            assert (np.abs(Rg - Rf) <= 2 * tol).all()
            np.testing.assert_allclose(Sg, Sf, rtol=1e-10, atol=1e-10)
            assert fresh.mccfr_iteration() == ctx.mccfr_iteration() == k
    finally:
        if fresh is not None:
            fresh.close()
        restore(ctx, sl)


# ---- 3. set_deal with everything warm -------------------------------------------------------------------------------------------------------------
SENTINEL = -7.25


def _uniform_policy(t):
    return np.where(_legal(t), 1.0 / t.infoset_nlegal[:, None].astype(np.float64), 0.0)


def _packed_image(ctx, nets):
    """both nets (the oracle's flat layout) as scopa_sdcfr_pack_weights lays them out, packed on the context's stream and waited for"""
    import torch
    from sdcfr_policy_ref import net_params
    img = torch.zeros((2, ctx._L.scopa_sdcfr_image_floats()), dtype=torch.float32, device="cuda:0")
    for p in range(2):
        ps = [torch.from_numpy(np.ascontiguousarray(w, np.float32)).to("cuda:0") for w in net_params(nets[p])]
        torch.cuda.synchronize()
        ctx.sdcfr_pack_weights(p, *(x.data_ptr() for x in ps), img.data_ptr())
        ctx.synchronize()                                   # the parameter tensors die with this iteration
    return img


def _sdcfr_walk(ctx, golden, batch, trav, iteration):
    """one default-mode scopa_sdcfr_traverse_fused launch under the fixture's nets -> (feat, regret, values)"""
    import torch
    from conftest import sdcfr_nets
    nets = sdcfr_nets(golden.npz("sdcfr.npz"))
    img = _packed_image(ctx, nets)
    feat = torch.zeros((41 * batch, 34), dtype=torch.float32, device="cuda:0")
    reg = torch.zeros((41 * batch, 16), dtype=torch.float32, device="cuda:0")
    vals = torch.zeros(batch, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    ctx.sdcfr_traverse_fused(trav, batch, img.data_ptr(), feat.data_ptr(), reg.data_ptr(), 0, 41 * batch, 0, vals.data_ptr(), 0, iteration, 0)
    ctx.synchronize()
    return feat.cpu().numpy(), reg.cpu().numpy(), vals.cpu().numpy(), nets


def _check_walk(ctx, golden, deal_seed, batch, trav, iteration, seed, what):
    """the walk's rows and root values against sdcfr_policy_ref.traverse_batch for the deal in force, within that module's own tolerances"""
    import sdcfr_policy_ref as R
    f, r, v, nets = _sdcfr_walk(ctx, golden, batch, trav, iteration)
    nt = R.NodeTable(deal_seed, nets)
    ref = R.traverse_batch(nt, trav, range(batch), seed, iteration)
    for b, x in enumerate(ref):
        rows = slice(41 * b, 41 * b + 41)
        assert np.array_equal(f[rows], x.feat), (what, b)
        assert (np.abs(r[rows] - x.regret) <= x.tol_regret).all(), (what, b)
        assert abs(float(v[b]) - x.value) <= x.tol_value, (what, b)
    return nt


def _warm_everything(ctx, sl, golden, t, bound):
    import torch
    ctx.cfr_exact_iterate(1)                                # the schedule
    assert ctx.cfr_exact_last_route() == 0
    ctx.mccfr_graph_mode(True)
    for batch in BATCHES:                                   # captured graphs at two batches
        ctx.mccfr_iterate(batch, 3)
    pol = torch.from_numpy(_uniform_policy(t)).to("cuda:0")
    torch.cuda.synchronize()
    ctx.eval_tabular_prepare(pol.data_ptr())                # evaluator thresholds
    ctx.eval_tabular_match(64, 32, 1)
    _sdcfr_walk(ctx, golden, 13, 0, 40)                     # node bits and the policy table
    ctx.sdcfr_policy_get()
    ctx.mccfr_bind_delta(bound.data_ptr(), t.n_infosets * 5 * 8)
    assert ctx.mccfr_delta_buffer() == (bound.data_ptr(), t.n_infosets * 5 * 8)


def _consume_everything(ctx, sl, oracle, golden, seed_deal, own_delta, what):
    """every consumer on the deal just set, each against the oracle from zero tables"""
    import torch
    from xplay_ref import Ref
    t = tree(oracle, seed_deal)
    # the getters, before any new launch: the new deal's zero state or a refusal
    assert ctx.mccfr_iteration() == 0 and ctx.cfr_exact_last_route() == -1 and not ctx.visited_get().any(), what
    _tables_bits(ctx, t.tables(), what)
    for refused in (ctx.sdcfr_policy_get, lambda: ctx.eval_tabular_match(64, 32, 1)):
        with pytest.raises(sl.ScopaError) as e:
            refused()
        assert e.value.status == sl.SCOPA_ESTATE, what
    assert ctx.mccfr_delta_buffer() == (own_delta, t.n_infosets * 5 * 8), what
    assert not ctx.mccfr_delta_get().any(), what
    c0 = ctx.counters()
    # exact CFR: the schedule is rebuilt for this deal
    R, S, L = t.tables()
    assert same_bits(ctx.cfr_exact_iterate(2), t.cfr_exact(R, S, L, 2)), what
    _tables_bits(ctx, (R, S, L), what)
    assert ctx.cfr_exact_last_route() == 0 and np.array_equal(ctx.visited_get(), np.arange(1, t.n_infosets + 1)), what
    c1 = ctx.counters()
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (4 * N_DECISION, 4 * N_TERMINAL), what
    # graph-mode MCCFR at both batches (graph mode is still on: the old deal's graphs must be gone), then the split path
    Z = np.zeros((t.n_infosets, 4))
    for batch in BATCHES:
        ctx.tables_reset()
        c1 = ctx.counters()
        ctx.mccfr_iterate(batch, 3)
        counted(ctx, c1, 3 * batch, what)
        Rg, Sg, _ = ctx.tables_get()
        check_iterations((Rg, Sg), t, Z, Z, DEFAULT_SEED, 0, 3, batch, what + (batch, "graph"))
    ctx.tables_reset()
    ctx.mccfr_traverse(0, 0, 48)
    d = ctx.mccfr_delta_get()
    dR, dS, A, _, _ = t.mccfr_batched_delta_abs(Z, DEFAULT_SEED, 0, 0, 48)
    assert np.array_equal(d[:, 4], np.rint(dS.sum(1))), what
    assert (E.row_errors(d[:, :4], dR, A) <= E.K_REORDER).all(), what
    ctx.mccfr_apply()
    Rg, Sg, _ = ctx.tables_get()
    check_iterations((Rg, Sg), t, Z, Z, DEFAULT_SEED, 0, 1, 48, what + ("split",))
    # the evaluator: prepared again for this deal, episode for episode against the restatement
    ref = Ref(t)
    P = t.average_policy(Sg)
    pol = torch.from_numpy(P).to("cuda:0")
    idx = torch.full((257,), -1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    ctx.eval_tabular_prepare(pol.data_ptr())
    st = ctx.eval_tabular_match(257, 129, 5, 0, idx.data_ptr())
    _check_match(oracle, ref, st, idx.cpu().numpy().astype(np.int64), P, 257, 129, 5, DEFAULT_SEED, what)
    # the SDCFR walk: node bits and policy table of this deal
    nt = _check_walk(ctx, golden, seed_deal, 13, 0, 40, DEFAULT_SEED, what)
    pol32, _ = ctx.sdcfr_policy_get()
    Pn, Tn, _, _ = nt.by_level()
    assert (np.abs(pol32.astype(np.float64) - Pn) <= Tn).all(), what


def _check_match(oracle, ref, st, idx, P, n, n_seat0, sid, seed, what):
    """scopa_eval_tabular_match's episodes and sums against xplay_ref: the policy's seat by its thresholds, the other seat by the uniform table's"""
    thr, uni = ref.thresholds(P), ref.thresholds(np.where(np.arange(4)[None, :] < ref.nlegal[:, None], 1.0 / ref.nlegal[:, None], 0.0))
    first, second = np.arange(n_seat0), np.arange(n_seat0, n)
    want0 = ref.episodes(oracle, thr, uni, first, sid, seed)
    want1 = ref.episodes(oracle, uni, thr, second, sid, seed)
    assert np.array_equal(idx[:n_seat0], want0) and np.array_equal(idx[n_seat0:n], want1), what
    assert st[0].tolist() == ref.match_stats(want0, 0) and st[1].tolist() == ref.match_stats(want1, 1), what


def test_set_deal_with_everything_warm(ctx, sl, oracle, golden):
    """Deal 282 (251 infosets) with every cache warm -> set_deal(129) (1144 infosets) -> every consumer -> set_deal(282) -> every consumer again.
    The bound delta buffer is the first 251 * 5 doubles of a tensor of 1144 * 5 + 64 sentinels: a reset that ran before the unbind would write 1144
    rows into it, inside the test's own allocation, and the slack would show it."""
    import torch
    try:
        ctx.mccfr_seed(DEFAULT_SEED)
        t = deal(ctx, sl, oracle, 282)
        own = ctx.mccfr_delta_buffer()[0]
        buf = torch.full((DEALS[129] * 5 + 64,), SENTINEL, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        _warm_everything(ctx, sl, golden, t, buf)
        ctx.synchronize()
        assert not buf[:DEALS[282] * 5].cpu().numpy().any() and (buf[DEALS[282] * 5:].cpu().numpy() == SENTINEL).all()    # bind zeroes what it was promised
        for seed_deal in (129, 282):
            deal(ctx, sl, oracle, seed_deal)
            ctx.synchronize()
            assert (buf[DEALS[282] * 5:].cpu().numpy() == SENTINEL).all(), seed_deal
            _consume_everything(ctx, sl, oracle, golden, seed_deal, own, (seed_deal,))
            assert (buf[DEALS[282] * 5:].cpu().numpy() == SENTINEL).all() and not buf[:DEALS[282] * 5].cpu().numpy().any(), seed_deal
            if seed_deal == 129:                            # warm again on the large deal, so that the way back shrinks every size
                ctx.cfr_exact_iterate(1)
                ctx.mccfr_iterate(48, 3)
    finally:
        restore(ctx, sl)


# ---- 4. seed, LDS limit and graph mode toggles ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", GRAPH_ITERS)
def test_seed_lds_limit_and_graph_mode_toggles(ctx, sl, oracle, k):
    """After graphs are captured for (48, k): a new seed, an LDS limit that narrows the traversal workgroups (98 KB: 4 wavefronts at 738 infosets)
    and its restoration, graph_mode(0) then (1), and profiling on (the eager fallback inside a graph-mode context).  After each, the same (48, k)
    call from reset tables against the oracle under the seed then in force; iteration ids continue without a gap across the fallback."""
    try:
        t = deal(ctx, sl, oracle, 42)
        Z = np.zeros((t.n_infosets, 4))
        ctx.mccfr_graph_mode(True)
        seed = SEED

        def run(what, reset=True):
            if reset:
                ctx.tables_reset()
            it = ctx.mccfr_iteration()
            R0, S0, _ = ctx.tables_get()
            c0 = ctx.counters()
            ctx.mccfr_iterate(48, k)
            counted(ctx, c0, 48 * k, what)
            assert ctx.mccfr_iteration() == it + k, what
            Rg, Sg, _ = ctx.tables_get()
            check_iterations((Rg, Sg), t, R0, S0, seed, it, k, 48, (what, k))

        ctx.mccfr_seed(seed)
        run("captured")
        seed = 0xABCDEF12345
        ctx.mccfr_seed(seed)
        run("new seed")
        ctx.debug_lds_limit(98 * 1024)
        run("narrow workgroups")
        ctx.debug_lds_limit(0)
        run("limit restored")
        ctx.mccfr_graph_mode(False)
        ctx.mccfr_graph_mode(True)
        run("graph mode off and on")
        ctx.prof_enable(1)                                  # launches that carry events cannot be captured: the eager loop runs
        run("profiled: eager fallback", reset=False)
        assert ctx.prof_read()[0] > 0                       # only eager launches carry events: the fallback ran
        ctx.prof_enable(0)
        run("graphs again after the fallback", reset=False)
        assert ctx.mccfr_iteration() == 3 * k
    finally:
        restore(ctx, sl)


# ---- 6. evaluator thresholds ----------------------------------------------------------------------------------------------------------------------
def test_evaluator_thresholds_follow_prepare_and_the_deal(ctx, sl, oracle):
    """prepare(A), match, prepare(B), match, a pair match (thresholds of its own), a match that must still use B, set_deal, a match that must refuse
    (the thresholds are indexed by the old deal's infoset ids), prepare on the new deal, match.  n = 257 episodes, episode for episode."""
    import torch
    from xplay_ref import Ref, policy_set
    try:
        ctx.mccfr_seed(SEED)
        t = deal(ctx, sl, oracle, 42)
        ref, pols = Ref(t), policy_set(t)
        A, B = pols["dirichlet"], pols["zeros"]
        dA, dB, dC = (torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0") for x in (A, B, pols["onehot_a"]))
        idx = torch.full((257,), -1, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()

        def match(P, r, tr, what):
            idx.fill_(-1)
            torch.cuda.synchronize()
            st = ctx.eval_tabular_match(257, 129, 9, 0, idx.data_ptr())
            _check_match(oracle, r, st, idx.cpu().numpy().astype(np.int64), P, 257, 129, 9, SEED, what)

        ctx.eval_tabular_prepare(dA.data_ptr())
        match(A, ref, t, "A")
        ctx.eval_tabular_prepare(dB.data_ptr())
        match(B, ref, t, "B after A")
        st = ctx.eval_pair_match(dA.data_ptr(), dC.data_ptr(), 257, 129, 9, idx.data_ptr())
        thrA, thrC = ref.thresholds(A), ref.thresholds(pols["onehot_a"])
        w0 = ref.episodes(oracle, thrA, thrC, np.arange(129), 9, SEED)
        w1 = ref.episodes(oracle, thrC, thrA, np.arange(129, 257), 9, SEED)
        got = idx.cpu().numpy().astype(np.int64)
        assert np.array_equal(got[:129], w0) and np.array_equal(got[129:], w1)
        assert st[0].tolist() == ref.match_stats(w0, 0) and st[1].tolist() == ref.match_stats(w1, 1)
        match(B, ref, t, "B after the pair match")
        t2 = deal(ctx, sl, oracle, 129)
        with pytest.raises(sl.ScopaError) as e:
            ctx.eval_tabular_match(257, 129, 9, 0, idx.data_ptr())
        assert e.value.status == sl.SCOPA_ESTATE
        ref2 = Ref(t2)
        P2 = policy_set(t2)["dirichlet"]
        d2 = torch.from_numpy(np.ascontiguousarray(P2)).to("cuda:0")
        torch.cuda.synchronize()
        ctx.eval_tabular_prepare(d2.data_ptr())
        match(P2, ref2, t2, "the new deal")
    finally:
        restore(ctx, sl)


# ---- 7. MultiDeal: packed rows, mixed solvers, a second build --------------------------------------------------------------------------------------
def _multi_seeds(n):
    return ([42, 129, 282, 7, 474, 1789] + list(range(100, 100 + n)))[:n]       # 65: one full wavefront of lanes plus one


def _multi_trees(oracle, seeds, _cache={}):
    for s in seeds:
        if s not in _cache:
            _cache[s] = oracle.Tree(seed=s)
    return [_cache[s] for s in seeds]


@pytest.mark.parametrize("n", [6, 65])
def test_multi_deal_rows_solvers_and_a_second_build(ctx, sl, oracle, n):
    """One MultiDeal of n deals.  (a) cfr_exact_iterate_lanes, tables_set on the LAST deal (lane 0 of the second wavefront at 65) with a consistent
    edge table, lanes again: the lane-packed rows must be re-read -- every deal bit for bit against Tree.cfr_exact.  (b) mccfr_iterate, a masked
    alternating DCFR sweep, mccfr_iterate: the sweep bit for bit against cfr_variants_ref from the device's own tables (masked-out deals keep their
    bits), the MCCFR legs at rtol = atol = 1e-10 as tests/test_gpu_multi.py, iteration ids 0, 1 then 2, 3.  (c) set_perms and build a second time:
    tables, counters and the MCCFR iteration number are a fresh handle's."""
    import cfr_edges as CE
    from cfr_variants_ref import Ref
    m = None
    try:
        seeds = _multi_seeds(n)
        trees = _multi_trees(oracle, seeds)
        m = sl.MultiDeal(ctx, n)
        m.set_perms(np.stack([sl.deal_py_seed(s) for s in seeds]))
        assert m.build().tolist() == [t.n_infosets for t in trees]
        # (a)
        want = [t.tables() for t in trees]
        m.cfr_exact_iterate_lanes(1)
        for t, w in zip(trees, want):
            t.cfr_exact(*w, 1)
        want[n - 1] = CE.tables("onehot", trees[n - 1].infoset_nlegal)
        m.tables_set(n - 1, *want[n - 1])
        m.cfr_exact_iterate_lanes(1)
        for d, (t, w) in enumerate(zip(trees, want)):
            t.cfr_exact(*w, 1)
            got = m.tables_get(d)
            assert all(same_bits(a, b) for a, b in zip(got[:3], w)), ("lanes after tables_set", n, d)
        assert m.counters() == (2 * 2 * N_DECISION * n, 2 * 2 * N_TERMINAL * n)
        # (b) from fresh tables: a second build on the same deals
        m.build()
        assert m.counters() == (0, 0)
        mask = np.arange(n) % 2 == 0
        cur = []
        m.mccfr_iterate(48, 2, SEED)
        for d, t in enumerate(trees):
            Z = np.zeros((t.n_infosets, 4))
            Ro, So, _ = oracle_iterations(t, Z, Z, SEED, 0, 2, 48)
            Rg, Sg, Lg, _ = m.tables_get(d)
            np.testing.assert_allclose(Rg, Ro, rtol=1e-10, atol=1e-10)
            np.testing.assert_allclose(Sg, So, rtol=1e-10, atol=1e-10)
            cur.append((Rg, Sg, Lg))
        m.cfr_sync_iterate_weighted(_dcfr_weights(), alternating=True, active=mask)
        for d, t in enumerate(trees):
            R, S, L = (x.copy() for x in cur[d])
            if mask[d]:
                Ref(t).run(R, S, _dcfr_weights(), alternating=True)
            got = m.tables_get(d)
            assert all(same_bits(a, b) for a, b in zip(got[:3], (R, S, L))), ("masked sweep", n, d, bool(mask[d]))
            cur[d] = (R, S, L)
        c0 = m.counters()
        m.mccfr_iterate(48, 2, SEED)
        c1 = m.counters()
        assert (c1[0] - c0[0], c1[1] - c0[1]) == (PAIR[0] * 48 * 2 * n, PAIR[1] * 48 * 2 * n)
        for d, t in enumerate(trees):
            Ro, So, _ = oracle_iterations(t, cur[d][0], cur[d][1], SEED, 2, 2, 48)
            Rg, Sg, Lg, _ = m.tables_get(d)
            np.testing.assert_allclose(Rg, Ro, rtol=1e-10, atol=1e-10)
            np.testing.assert_allclose(Sg, So, rtol=1e-10, atol=1e-10)
            assert same_bits(Lg, cur[d][2])
        # (c) other deals on the same object
        seeds2 = seeds[::-1][:-1] + [2244]
        trees2 = _multi_trees(oracle, seeds2)
        m.set_perms(np.stack([sl.deal_py_seed(s) for s in seeds2]))
        assert m.build().tolist() == [t.n_infosets for t in trees2]
        assert m.counters() == (0, 0)
        for d, t in enumerate(trees2):
            got = m.tables_get(d)
            assert all(same_bits(a, b) for a, b in zip(got[:3], t.tables())), ("second build", n, d)
            assert [sl.key_to_string(k) for k in got[3]] == t.infoset_strings
        m.mccfr_iterate(48, 1, SEED)
        assert m.counters() == (PAIR[0] * 48 * n, PAIR[1] * 48 * n)
        for d, t in enumerate(trees2):
            Z = np.zeros((t.n_infosets, 4))
            Ro, So, _ = oracle_iterations(t, Z, Z, SEED, 0, 1, 48)           # iteration 0 again
            Rg, Sg, _, _ = m.tables_get(d)
            np.testing.assert_allclose(Rg, Ro, rtol=1e-10, atol=1e-10)
            np.testing.assert_allclose(Sg, So, rtol=1e-10, atol=1e-10)
    finally:
        if m is not None:
            m.close()
        restore(ctx, sl)


# ---- 5. Deep CFR on a long-lived solver ----------------------------------------------------------------------------------------------------------
def _solver_nets(d):
    """the solver's own parameters read back, as sdcfr_policy_ref takes them"""
    return [{k: v.detach().clone() for k, v in d.advantage_nets[p].net.state_dict().items()} for p in range(2)]


def _load_nets(d, nets):
    import torch
    import sdcfr_policy_ref as R
    for p in range(2):
        params = R.net_params(nets[p])
        d.advantage_nets[p].net.load_state_dict({k: torch.from_numpy(w.astype(np.float32)).to("cuda:0") for k, w in zip(R.SD_KEYS, params)})


def _solver_rows(d, trav, B, mode):
    import torch
    d._engine.ctx.sdcfr_mode(mode)
    try:
        mem = d.advantage_nets[trav].buffer
        mem.total = 0
        vals = d._traverse_batch(trav, B, fused=True)
    finally:
        d._engine.ctx.sdcfr_mode(0)
    f, r, m = (x.cpu().numpy() for x in mem.rows(torch.arange(41 * B, device="cuda:0")))
    return f, r, m, vals.cpu().numpy()


def _check_solver(d, deal_seed, nets, B, what):
    """walk and per-visit rows of both traversers: bit for bit the same, and sdcfr_policy_ref.traverse_batch's for `nets` on `deal_seed` within
    tol_regret / tol_value, features and masks exact; then the walk's policy table against the same nets"""
    import sdcfr_policy_ref as R
    nt = R.NodeTable(deal_seed, nets)
    # the rule of test_gpu_sdcfr_policy_ref.py's cases: the first iteration, from the current one on, at which the REFERENCE can decide every draw
    # of the sampled ids for both traversers (it raises AmbiguousDraw where a draw lies within its own tolerance of a cdf boundary)
    for it in range(d._iteration, d._iteration + 16):
        try:
            refs = [R.traverse_batch(nt, trav, range(B), DEFAULT_SEED, it) for trav in (0, 1)]
            break
        except R.AmbiguousDraw:
            continue
    else:
        raise AssertionError((what, "sixteen iterations in a row with an ambiguous draw"))
    d._iteration = it
    for trav in (0, 1):
        walk = _solver_rows(d, trav, B, 0)
        visit = _solver_rows(d, trav, B, 1)
        assert all(np.array_equal(a, b) for a, b in zip(walk, visit)), (what, trav, "walk vs per-visit")
        f, r, m, v = walk
        for b, x in enumerate(refs[trav]):
            rows = slice(41 * b, 41 * b + 41)
            assert np.array_equal(f[rows], x.feat) and np.array_equal(m[rows], x.mask), (what, trav, b)
            assert (np.abs(r[rows] - x.regret) <= x.tol_regret).all(), (what, trav, b)
            assert abs(float(v[b]) - x.value) <= x.tol_value, (what, trav, b)
    _solver_rows(d, 0, B, 0)                                # the table of the last WALK launch
    pol, _ = d._engine.ctx.sdcfr_policy_get()
    P, T, _, _ = nt.by_level()
    assert (np.abs(pol.astype(np.float64) - P) <= T).all(), (what, "policy table")


@pytest.mark.parametrize("B", [13, 96])
def test_deep_cfr_on_a_long_lived_solver(ctx, sl, golden, B):
    """One DeepCFR: walk; load_state_dict of perturbed nets; walk; one train step by each backend (PyTorch eager, graph-replayed, the hand-written
    step), a walk after each; per-visit mode and back (inside every check); the engine's set_deal(7); walk.  After each step the rows are those of
    the nets and deal then in force -- after train the solver's own parameters read back -- so a stale packed image (weights_epoch), policy table or
    node-bit table fails here.  Batch 13 is ragged against the twelve wavefronts; 96 fills them.  Iterations 40 (fixture nets) and 41 (from the
    perturbed nets on): those at which test_gpu_sdcfr_policy_ref.py's cases have no ambiguous draw."""
    import torch
    from conftest import sdcfr_nets
    from scopa_amd.algorithms.deep_cfr import DeepCFR
    from scopa_amd.envs.openspiel_mini_scopa import MiniScopaGame
    base = sdcfr_nets(golden.npz("sdcfr.npz"))
    rng = np.random.default_rng(11)
    perturbed = [np.asarray(base[p], np.float32) + (0.05 * rng.standard_normal(base[p].size)).astype(np.float32) for p in range(2)]
    torch.manual_seed(0)
    d = DeepCFR(MiniScopaGame(seed=42), num_players=2, device="cuda:0", batch=B, memory_size=41 * B, graph_training=True)
    try:
        d._iteration = 40
        _load_nets(d, base)
        _check_solver(d, 42, base, B, "fixture nets")
        d._iteration = 41
        _load_nets(d, perturbed)
        _check_solver(d, 42, perturbed, B, "after load_state_dict")
        for backend in ("torch", "graph", "hip"):
            for a in d.advantage_nets:
                a.use_graph, a.train_backend = backend == "graph", "hip" if backend == "hip" else "torch"
                before = [p.detach().clone() for p in a.param_list()]
                a.train(batch_size=128, epochs=1)
                torch.cuda.synchronize()
                assert any(not torch.equal(x, y) for x, y in zip(before, a.param_list())), (backend, "the step moved nothing")
            _check_solver(d, 42, _solver_nets(d), B, f"after train ({backend})")
        trained = _solver_nets(d)
        d._engine.ctx.set_deal(sl.deal_py_seed(7))
        _check_solver(d, 7, trained, B, "after set_deal(7)")
    finally:
        d._engine.close()


# ---- 7b. ChanceGame: stamps and increment rows of unlisted deals, traversal tables across a reset ------------------------------------------------
def _chance_perms(n):
    from chance_sets import HIDDEN70
    from test_gpu_chance_mccfr import SIX
    return SIX if n == 6 else HIDDEN70[:65]


def _chance_ref(oracle, n, _cache={}):
    from chance_mccfr_ref import ChanceMccfrRef
    from chance_sampled_ref import SampledChanceRef
    if n not in _cache:
        cr = SampledChanceRef([oracle.Tree(perm=p) for p in _chance_perms(n)])
        assert int((cr.count > 1).sum()) > 0                # rows shared between deals: what the reduce is about
        _cache[n] = (cr, ChanceMccfrRef(cr))
    return _cache[n]


def _chance_lists(n):
    """(two MCCFR lists, two sampled-CFR lists over other deals, a last and shorter MCCFR list): every deal of the last list sat in another slot, or
    in none, in the calls before it"""
    ids = np.arange(n)
    first = [ids[::2].tolist(), ids[1::2].tolist()[:len(ids[::2])]]
    first[1] = (first[1] + ids[::2].tolist())[:len(first[0])]            # both rows of one call have the same length
    sampled = [ids[::3].tolist(), (ids[::3] + 1)[: len(ids[::3])].clip(0, n - 1).tolist()]
    sampled[1] = sorted(set(sampled[1]))
    sampled[1] = (sampled[1] + [i for i in ids.tolist() if i not in sampled[1]])[:len(sampled[0])]
    last = [ids[::-1][: max(2, n // 4)].tolist()]
    return first, sampled, last


@pytest.mark.parametrize("n", [6, 65])
def test_chance_game_lists_tables_and_reduce(ctx, sl, oracle, n):
    """mccfr_iterate over listed deals (two iterations, two lists), cfr_iterate_sampled over other lists (alternating DCFR weights), tables_set of an
    edge table, mccfr_iterate over a shorter list.  The sampled sweeps are held bit for bit to chance_sampled_ref from the device's own tables; the
    MCCFR legs to chance_mccfr_ref (two iterations: rtol = atol = 1e-10; the last one from given tables: strategy sums and visit counts exact,
    regrets in the reorder budget) and rows without a listed occurrence keep their bits -- so an increment row or stamp left by an earlier call
    for a deal that is not listed now would show."""
    from chance_sets import multi, weights
    g = None
    try:
        cr, mr = _chance_ref(oracle, n)
        g = sl.ChanceGame(multi(ctx, sl, _chance_perms(n)))
        assert (g.n, g.G, g.n_occurrences) == (cr.n, cr.G, cr.n_occ)
        first, sampled, last = _chance_lists(n)
        R, S = cr.tables()
        g.mccfr_iterate(48, 2, SEED, deals=first)
        mr.run(R, S, 48, SEED, 0, 2, first)
        Rg, Sg = g.tables_get()
        np.testing.assert_allclose(Rg, R, rtol=1e-10, atol=1e-10)
        np.testing.assert_allclose(Sg, S, rtol=1e-10, atol=1e-10)
        pairs = 48 * sum(len(x) for x in first)
        assert g.mccfr_counters() == (PAIR[0] * pairs, PAIR[1] * pairs, 2)
        w = weights("dcfr", 2)
        g.cfr_iterate_sampled(sampled, w, alternating=True)
        cr.run_sampled(Rg, Sg, sampled, w, alternating=True)                # from the device's own tables, in place
        got = g.tables_get()
        assert np.array_equal(got[0], Rg) and np.array_equal(got[1], Sg), "sampled sweeps after MCCFR"
        R0 = E.edge_table("small_large", cr.nlegal)
        S0 = Sg.copy()
        g.tables_set(R0, S0)
        R, S = R0.copy(), S0.copy()
        A, visits, touched, vis = mr.iterate(R, S, 48, SEED, 2, last[0])
        assert 0 < touched.sum() < cr.G
        g.mccfr_iterate(48, 1, SEED, deals=last)
        Rg, Sg = g.tables_get()
        want_S = np.where(cr.legal, S0 + visits.astype(np.float64)[:, None] * E.reference_sigma(R0, cr.nlegal), S0)
        assert np.array_equal(S, want_S) and np.array_equal(Sg, want_S)
        bound = (E.K_REORDER * E.EPS * A.sum(1))[:, None] + 2.0 * E.EPS * np.abs(R)
        assert (np.abs(Rg - R) <= bound).all()
        assert same_bits(Rg[~touched], R0[~touched]) and same_bits(Sg[~touched], S0[~touched])
        assert g.mccfr_counters() == (PAIR[0] * pairs + vis[0], PAIR[1] * pairs + vis[1], 3)
    finally:
        if g is not None:
            g.close()
            g.multi.close()
        restore(ctx, sl)


@pytest.mark.parametrize("n,batch", [(6, 13), (6, 96), (65, 13)])
def test_chance_game_sdcfr_traverse_across_a_reset(ctx, sl, oracle, golden, n, batch):
    """sdcfr_traverse over a list, an MCCFR iteration over another list and tables_reset, sdcfr_traverse over a third list: each call's rows and
    root values equal, bit for bit (the contract of tests/test_gpu_chance_sdcfr.py), those of scopa_sdcfr_traverse_fused on a second context that is
    moved from listed deal to listed deal by set_deal -- which also walks that context's node-bit table through every deal change."""
    import torch
    from chance_sets import multi
    from conftest import sdcfr_nets
    g, other = None, None
    try:
        perms = _chance_perms(n)
        ctx.mccfr_seed(DEFAULT_SEED)
        g = sl.ChanceGame(multi(ctx, sl, perms))
        other = sl.Context(0)
        other.mccfr_seed(DEFAULT_SEED)
        img = _packed_image(ctx, sdcfr_nets(golden.npz("sdcfr.npz")))
        v0 = g.sdcfr_visits()

        def both(trav, deals, iteration):
            m, rows = len(deals), 41 * len(deals) * batch
            out = []
            for chance in (True, False):
                f = torch.full((rows, 34), SENTINEL, dtype=torch.float32, device="cuda:0")
                r = torch.full((rows, 16), SENTINEL, dtype=torch.float32, device="cuda:0")
                v = torch.full((m * batch,), SENTINEL, dtype=torch.float32, device="cuda:0")
                torch.cuda.synchronize()
                if chance:
                    g.sdcfr_traverse(trav, batch, img.data_ptr(), f.data_ptr(), r.data_ptr(), 0, rows, 0, v.data_ptr(), iteration, 1000, deals)
                    ctx.synchronize()
                else:
                    for s, dl in enumerate(deals):
                        other.set_deal(np.ascontiguousarray(perms[dl]))
                        other.sdcfr_traverse_fused(trav, batch, img.data_ptr(), f.data_ptr(), r.data_ptr(), 0, rows, 41 * s * batch,
                                                   v.data_ptr() + 4 * s * batch, 0, iteration, 1000 + dl * batch)
                        other.synchronize()
                out.append((f.cpu().numpy(), r.cpu().numpy(), v.cpu().numpy()))
            assert (out[1][1] != SENTINEL).any(1).all() and (out[1][2] != SENTINEL).all()
            assert all(np.array_equal(a, b) for a, b in zip(*out)), (trav, deals)

        a, b, c = [n - 1, 0, 2], [1, n - 2], [2, n - 1, 1, 3]
        both(0, a, 3)
        g.mccfr_iterate(48, 1, SEED, deals=[b])
        g.tables_reset()
        assert not g.tables_get()[0].any()
        both(1, c, 4)
        both(0, a, 3)
        assert g.sdcfr_visits() - v0 == batch * (105 * 2 * len(a) + 82 * len(c))
    finally:
        if other is not None:
            other.close()
        if g is not None:
            g.close()
            g.multi.close()
        restore(ctx, sl)
