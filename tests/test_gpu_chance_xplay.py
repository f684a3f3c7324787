"""scopa_chance_cross_play, scopa_chance_best_response and scopa_chance_match (scopa_amd/csrc/scopa_chance_xplay.hip) and the Python layer on them, on
the GPU.

The exact kernels are held BIT FOR BIT to tests/chance_xplay_ref.py (which tests/test_chance_xplay_ref.py anchors to ChanceRef.exploitability), to
scopa_cross_play / scopa_best_response on contexts holding one deal each, and to scopa_chance_exploitability; the match episode for episode to the
reference's deal draws and to scopa_eval_pair_match on a context holding the drawn deal.  Sets: the six deals of tests/test_gpu_chance.py (four
policies: uniform, solved by 20 DCFR iterations, Dirichlet, one-hot), BOTH25 and HIDDEN70 of tests/chance_sets.py (rows shared by up to 8 and 70
deals)."""
import numpy as np
import pytest

import chance_sets
import chance_xplay_ref as X
from cfr_edges import same_bits
from xplay_ref import TWO53

pytestmark = pytest.mark.gpu

KB64 = 64 * 1024
N_DECISION, N_NODES = 1653, 2229


def _multi(ctx, sl, perms):
    perms = np.asarray(perms, np.uint8).reshape(-1, 16)
    m = sl.MultiDeal(ctx, len(perms))
    m.set_perms(perms)
    m.build()
    return m


def _game(ctx, sl, perms):
    return sl.ChanceGame(_multi(ctx, sl, perms))


def _dev(a, dtype=None):
    import torch
    return torch.as_tensor(np.array(a, dtype=dtype, order="C"), device="cuda:0")          # a copy: the cached tables are read-only


def _cross(g, stack, per_deal=True):
    """raw scopa_chance_cross_play of a [K][G][4] device tensor -> (per_deal [n][K][K][4] or None, out [K][K][4])"""
    import torch
    k = stack.shape[0]
    out = torch.full((k, k, 4), -9.0, dtype=torch.float64, device="cuda:0")
    per = torch.full((g.n, k, k, 4), -9.0, dtype=torch.float64, device="cuda:0") if per_deal else None
    torch.cuda.synchronize()
    g.cross_play(k, stack.data_ptr(), out.data_ptr(), per.data_ptr() if per_deal else 0)
    g.ctx.synchronize()
    return (per.cpu().numpy() if per_deal else None), out.cpu().numpy()


def _best(g, stack, tables=True):
    import torch
    k = stack.shape[0]
    out4 = torch.full((k, 4), -9.0, dtype=torch.float64, device="cuda:0")
    br = torch.full((k, 2, g.G, 4), -9.0, dtype=torch.float64, device="cuda:0") if tables else None
    torch.cuda.synchronize()
    g.best_response(k, stack.data_ptr(), br.data_ptr() if tables else 0, out4.data_ptr())
    g.ctx.synchronize()
    return out4.cpu().numpy(), br


def _match(g, a, b, n, n_seat0, stream_id, want=True):
    import torch
    deal = torch.full((max(n, 1),), -1, dtype=torch.int32, device="cuda:0") if want else None
    idx = torch.full((max(n, 1),), -1, dtype=torch.int32, device="cuda:0") if want else None
    torch.cuda.synchronize()
    st = g.match(a.data_ptr(), b.data_ptr(), n, n_seat0, stream_id, deal.data_ptr() if want else 0, idx.data_ptr() if want else 0)
    if not want:
        return st, None, None
    return st, deal.cpu().numpy()[:n].astype(np.int64), idx.cpu().numpy()[:n].astype(np.int64)


def _single_cross(ctx, local_stack):
    """scopa_cross_play on the deal ctx holds"""
    import torch
    k = local_stack.shape[0]
    out = torch.full((k, k, 4), -9.0, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    ctx.cross_play(k, local_stack.data_ptr(), out.data_ptr())
    ctx.synchronize()
    return out.cpu().numpy()


def _single_pair(ctx, a, b, n, n_seat0, stream_id):
    import torch
    idx = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    st = ctx.eval_pair_match(a.data_ptr(), b.data_ptr(), n, n_seat0, stream_id, idx.data_ptr())
    return st, idx.cpu().numpy().astype(np.int64)


# ---- cross-play -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sel", [(0, 1, 2, 3), (2,)], ids=["K4", "K1"])
def test_cross_play_six_deals(ctx, sl, oracle, sel):
    """d_per_deal and d_out bit for bit against the restatement and against scopa_cross_play on a context holding each deal for the policy_for_deal
    tables; the diagonal is ChanceGame.exploitability's value; a repeat and the run without a per-deal image give the same bits."""
    s = X.six(oracle)
    ref_per, ref_out = X.six_cross(oracle)
    sel = list(sel)
    pols = s["pols"][sel]
    g = _game(ctx, sl, X.SIX)
    assert (g.n, g.G) == (6, 3522) and np.array_equal(g.index()[1], s["cref"].map)
    stack = _dev(pols)
    per, out = _cross(g, stack)
    assert same_bits(per, ref_per[np.ix_(range(6), sel, sel)]) and same_bits(out, ref_out[np.ix_(sel, sel)])
    assert same_bits(_cross(g, stack, per_deal=False)[1], out)                            # the handle's own image
    per2, out2 = _cross(g, stack)
    assert same_bits(per2, per) and same_bits(out2, out)
    for j, k in enumerate(sel):
        assert same_bits(out[j, j, 0], g.exploitability(s["pols"][k])[3]), s["names"][k]
    one = sl.Context(0)
    try:
        for d in range(6):
            assert one.set_deal(X.SIX[d]) == s["cref"].I[d]
            local = np.stack([g.policy_for_deal(P, d) for P in pols])
            assert same_bits(local, np.stack([s["xref"].local(P, d) for P in pols]))
            assert same_bits(_single_cross(one, _dev(local)), per[d]), d
    finally:
        one.close()


def test_one_deal_and_the_same_deal_twice_reduce_to_the_single_deal_bits(ctx, sl):
    """One deal: scopa_cross_play's and scopa_best_response's bits.  The same deal twice: the single deal's d_out, because (v + v) / 2 is exact."""
    import torch
    perm = sl.deal_py_seed(42)
    I = ctx.set_deal(perm)
    g1, g2 = _game(ctx, sl, perm), _game(ctx, sl, [perm, perm])
    assert (g1.G, g2.G, g2.n) == (I, I, 2)
    keys, mp = g1.index()
    rows = mp[0, :I]
    n = ((keys >> np.uint64(1)) & np.uint64(7)).astype(np.int64)
    rng = np.random.default_rng(5)
    legal = np.arange(4)[None, :] < n[:, None]
    pols = []
    for shape in (0.7, 1.5):
        gam = np.where(legal, rng.gamma(shape, size=(I, 4)), 0.0)
        pols.append(gam / gam.sum(1, keepdims=True))
    pols.append(np.where(legal, 1.0 / n[:, None], 0.0))
    pols = np.stack(pols)                                                               # [3][G][4] over global ids
    local = _dev(pols[:, rows])
    want = _single_cross(ctx, local)
    per, out = _cross(g1, _dev(pols))
    assert same_bits(out, want) and same_bits(per[0], want)
    per2, out2 = _cross(g2, _dev(pols))
    assert same_bits(out2, want) and same_bits(per2[0], want) and same_bits(per2[1], want)
    out4_want = torch.full((3, 4), -9.0, dtype=torch.float64, device="cuda:0")
    br_want = torch.full((3, 2, I, 4), -9.0, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    ctx.best_response(3, local.data_ptr(), br_want.data_ptr(), out4_want.data_ptr())
    ctx.synchronize()
    out4, br = _best(g1, _dev(pols))
    assert same_bits(out4, out4_want.cpu().numpy())
    assert same_bits(br.cpu().numpy()[:, :, rows], br_want.cpu().numpy())
    assert same_bits(_best(g2, _dev(pols), tables=False)[0], out4)                       # every sum doubles, every mean halves: exact


# ---- best response --------------------------------------------------------------------------------------------------------------------
def _scale_policies(g, keys):
    """three tables over a set's keys: uniform, a seeded Dirichlet table, the average policy after five DCFR iterations on the device"""
    from scopa_amd.algorithms import schedule
    n = ((keys >> np.uint64(1)) & np.uint64(7)).astype(np.int64)
    legal = np.arange(4)[None, :] < n[:, None]
    gam = np.where(legal, np.random.default_rng(77).gamma(0.7, size=(n.size, 4)), 0.0)
    g.tables_reset()
    g.cfr_iterate_weighted(schedule("dcfr", 0, 5, 1.5, 0.0, 2.0))
    _, solved = g.exploitability(return_policy=True)
    return np.stack([np.where(legal, 1.0 / n[:, None], 0.0), gam / gam.sum(1, keepdims=True), solved])


def _check_best_response(g, xref, pols, want=None):
    """out4 per policy against scopa_chance_exploitability, the tables against the restatement's exactly, the tables played back within 1e-12"""
    import torch
    stack = _dev(pols)
    out4, br = _best(g, stack)
    tables = br.cpu().numpy()
    for k, P in enumerate(pols):
        assert same_bits(out4[k], g.exploitability(P)), k
        w4, (b0, b1) = want[k] if want is not None else xref.best_response(P)
        assert same_bits(out4[k], w4), k
        assert same_bits(tables[k, 0], b0) and same_bits(tables[k, 1], b1), k
        _, x = _cross(g, torch.stack([br[k, 0], stack[k], br[k, 1]]).contiguous(), per_deal=False)
        print(f"policy {k}: BR0 {out4[k, 1]!r} played back {x[0, 1, 0]!r}; BR1 {out4[k, 2]!r} played back {-x[1, 2, 0]!r}")
        assert abs(x[0, 1, 0] - out4[k, 1]) <= 1e-12 and abs(-x[1, 2, 0] - out4[k, 2]) <= 1e-12, k
    assert same_bits(_best(g, stack, tables=False)[0], out4)
    return out4, tables


def test_best_response_six_deals_and_chunks(ctx, sl, oracle):
    """K = 3 on the six deals; then the same call under scratch budgets that hold one and two policies (chunks of 1 + 1 + 1 and 2 + 1): same bits."""
    s = X.six(oracle)
    sel = [1, 2, 3]
    g = _game(ctx, sl, X.SIX)
    out4, tables = _check_best_response(g, s["xref"], s["pols"][sel], [X.six_best(oracle, k) for k in sel])
    per_policy = 6 * (2 * N_NODES * 8 + N_DECISION * 64) + 4 * g.G                        # include/scopa.h
    stack = _dev(s["pols"][sel])
    try:
        for budget in (per_policy + 8, 2 * per_policy + 16, 1):
            g.debug_scratch_budget(budget)
            o, br = _best(g, stack)
            assert same_bits(o, out4) and same_bits(br.cpu().numpy(), tables), budget
    finally:
        g.debug_scratch_budget(0)
    assert same_bits(_best(g, stack)[0], out4)


def test_best_response_rows_shared_by_up_to_eight_deals(ctx, sl, oracle):
    r = chance_sets.ref(oracle, "BOTH25")
    chance_sets.check_figures(r, "BOTH25")
    g = _game(ctx, sl, chance_sets.perms("BOTH25"))
    assert np.array_equal(g.index()[0], r.keys)
    _check_best_response(g, X.ChanceXRef(r), _scale_policies(g, r.keys))


def test_best_response_a_row_in_all_seventy_deals(ctx, sl, oracle):
    r = chance_sets.ref(oracle, "HIDDEN70")
    chance_sets.check_figures(r, "HIDDEN70")
    g = _game(ctx, sl, chance_sets.perms("HIDDEN70"))
    assert np.array_equal(g.index()[0], r.keys) and int((r.count == 70).sum()) >= 1
    _check_best_response(g, X.ChanceXRef(r), _scale_policies(g, r.keys)[1:])


# ---- the match ------------------------------------------------------------------------------------------------------------------------
def _check_against_contexts(sl, g, xref, A, B, n, first, sid, deal, idx, st, seed=None):
    """every deal's episodes end where scopa_eval_pair_match ends them on a context holding that deal, position by position; the sums are theirs"""
    one = sl.Context(0)
    try:
        if seed is not None:
            one.mccfr_seed(seed)
        sums = np.zeros((2, 5), np.int64)
        for d in range(g.n):
            one.set_deal(X.SIX[d])
            _, want = _single_pair(one, _dev(xref.local(A, d)), _dev(xref.local(B, d)), n, first, sid)
            mine = deal == d
            assert np.array_equal(idx[mine], want[mine]), d
            for half in (0, 1):
                sel = mine & ((np.arange(n) >= first) == bool(half))
                sums[half] += np.array(xref.x[d].match_stats(idx[sel], half), np.int64)
        assert np.array_equal(st, sums)
    finally:
        one.close()


def test_match_six_deals(ctx, sl, oracle):
    """n = 20 001, 10 001 in seat 0, solved against Dirichlet: deals, terminal indices and sums are the restatement's; the indices are those of
    scopa_eval_pair_match per deal; the mean lies within 4 standard errors (exact second moment) of the exact reward; two runs agree."""
    s = X.six(oracle)
    xref, pols = s["xref"], s["pols"]
    _, out = X.six_cross(oracle)
    n, first, sid = X.MATCH_N, X.MATCH_SEAT0, X.MATCH_STREAM
    want_deal, want_idx, want_st = X.six_match(oracle, 1, 2)
    g = _game(ctx, sl, X.SIX)
    a, b = _dev(pols[1]), _dev(pols[2])
    st, deal, idx = _match(g, a, b, n, first, sid)
    assert np.array_equal(deal, want_deal) and sorted(set(deal.tolist())) == list(range(6))
    assert np.array_equal(idx, want_idx) and np.array_equal(st, want_st)
    st2, deal2, idx2 = _match(g, a, b, n, first, sid)
    assert np.array_equal(st2, st) and np.array_equal(deal2, deal) and np.array_equal(idx2, idx)
    assert np.array_equal(_match(g, a, b, n, first, sid, want=False)[0], st)
    _check_against_contexts(sl, g, xref, pols[1], pols[2], n, first, sid, deal, idx, st)
    exact = (first * out[1, 2, 0] - (n - first) * out[2, 1, 0]) / n
    var = (first * (out[1, 2, 1] - out[1, 2, 0] ** 2) + (n - first) * (out[2, 1, 1] - out[2, 1, 0] ** 2)) / n
    mean, se = st[:, 1].sum() / 2 / n, np.sqrt(var / n)
    print(f"sampled {mean:+.6f}, exact {exact:+.6f}, standard error {se:.6f}, z = {(mean - exact) / se:+.2f}")
    assert se > 0.0 and abs(mean - exact) <= 4.0 * se


@pytest.mark.parametrize("first", [10001, 0, 20001])
def test_match_against_uniform_and_one_sided_splits(ctx, sl, oracle, first):
    """solved against uniform, with the even split and with either half empty: the deal draws do not depend on the tables or the split, the walks
    are scopa_eval_pair_match's on the drawn deal"""
    s = X.six(oracle)
    xref, pols = s["xref"], s["pols"]
    n, sid = X.MATCH_N, X.MATCH_STREAM
    g = _game(ctx, sl, X.SIX)
    st, deal, idx = _match(g, _dev(pols[1]), _dev(pols[0]), n, first, sid)
    assert np.array_equal(deal, X.six_match(oracle, 1, 2)[0])
    assert st[:, 0].tolist() == [first, n - first]
    _check_against_contexts(sl, g, xref, pols[1], pols[0], n, first, sid, deal, idx, st)


def test_match_one_hot_tables_and_another_seed(ctx, sl, oracle):
    """one-hot rows have thresholds 0 and 2^53 only: every episode of a (deal, seat half) ends at one terminal.  Under scopa_mccfr_seed the draws
    change with the seed and still match the restatement's."""
    s = X.six(oracle)
    xref, pols = s["xref"], s["pols"]
    thr = xref.x[0].thresholds(xref.local(pols[3], 0))
    assert set(np.unique(thr).tolist()) == {0, TWO53}
    seed, n, first, sid = 987654321123, 3000, 1400, 9
    ctx.mccfr_seed(seed)
    g = _game(ctx, sl, X.SIX)
    onehot_b = np.roll(pols[3], 1, axis=1) * s["cref"].legal                           # another one-hot table where the rolled slot is legal ...
    onehot_b[onehot_b.sum(1) == 0, 0] = 1.0                                             # ... the first action elsewhere
    st, deal, idx = _match(g, _dev(pols[3]), _dev(onehot_b), n, first, sid)
    assert np.array_equal(deal, xref.deals(range(n), sid, seed))
    assert not np.array_equal(deal, xref.deals(range(n), sid, X.MATCH_SEED))
    for d in range(6):
        for half in (0, 1):
            sel = (deal == d) & ((np.arange(n) >= first) == bool(half))
            assert sel.any() and len(set(idx[sel].tolist())) == 1, (d, half)
    _check_against_contexts(sl, g, xref, pols[3], onehot_b, n, first, sid, deal, idx, st, seed=seed)
    assert (_match(g, _dev(pols[3]), _dev(onehot_b), 0, 0, sid, want=False)[0] == 0).all()


# ---- the Python layer -----------------------------------------------------------------------------------------------------------------
def test_python_layer(ctx, sl, oracle):
    from scopa_amd.algorithms import chance
    s = X.six(oracle)
    pols = s["pols"]
    ref_per, ref_out = X.six_cross(oracle)
    g = _game(ctx, sl, X.SIX)
    chance.check_policy_table(g, pols[1])
    chance.check_policy_table(g, pols)
    chance.check_policy_table(g, _dev(pols[2]))
    r = int(np.flatnonzero(s["cref"].nlegal == 2)[0])
    bad = pols[2].copy()
    bad[r, 3] = 0.25                                                                    # mass on an illegal slot
    with pytest.raises(ValueError):
        chance.check_policy_table(g, bad)
    bad = pols[2].copy()
    bad[r] *= 0.9                                                                       # a row summing to 0.9
    with pytest.raises(ValueError):
        chance.cross_play(g, [pols[0], bad])
    with pytest.raises(ValueError):
        chance.best_response(g, bad)
    with pytest.raises(ValueError):
        chance.check_policy_table(g, pols[0][:-1])
    for given in (pols, [p for p in pols], _dev(pols)):
        x = chance.cross_play(g, given)
        assert same_bits(x["reward"], ref_out[..., 0]) and same_bits(x["scopas"], ref_out[..., 2:]) and same_bits(x["per_deal"], ref_per)
        assert same_bits(x["reward_std"], np.sqrt(np.maximum(ref_out[..., 1] - ref_out[..., 0] * ref_out[..., 0], 0.0)))
    assert x["reward"].shape == (4, 4) and x["scopas"].shape == (4, 4, 2) and x["per_deal"].shape == (6, 4, 4, 4)
    b = chance.best_response(g, pols[1])
    e = g.exploitability(pols[1])
    w4, (b0, b1) = X.six_best(oracle, 1)
    assert (b["exploitability"], b["br_values"], b["value"]) == (e[0], (e[1], e[2]), e[3])
    assert same_bits(b["tables"][0], b0) and same_bits(b["tables"][1], b1)
    chance.check_policy_table(g, np.stack(b["tables"]))
    assert same_bits(chance.uniform_table(g), pols[0])
    n = 4001
    first = 2001
    avg, stats = chance.evaluate(g, pols[1], n, opponent=pols[2], stream_id=5)
    assert stats["exact_by_seat"] == (float(ref_out[1, 2, 0]), float(-ref_out[2, 1, 0]))
    assert stats["exact_reward"] == (first * ref_out[1, 2, 0] + (n - first) * -ref_out[2, 1, 0]) / n
    assert [h["episodes"] for h in stats["by_seat"]] == [first, n - first] and stats["data_collected"]
    assert {"trained_avg", "opponent_avg", "difference", "reward_std_error", "by_seat", "exact_reward", "exact_by_seat"} <= set(stats)
    print(f"sampled {avg:+.5f}, exact {stats['exact_reward']:+.5f}, standard error {stats['reward_std_error']:.5f}")
    assert abs(avg - stats["exact_reward"]) <= 5.0 * stats["reward_std_error"]
    avg_u, stats_u = chance.evaluate(g, pols[1], n, stream_id=5)                        # opponent None: the uniform table
    assert stats_u["exact_by_seat"] == (float(ref_out[1, 0, 0]), float(-ref_out[0, 1, 0]))
    assert chance.evaluate(g, pols[1], 0)[1]["data_collected"] is False


def test_chance_deep_cfr_evaluates_against_random(ctx, sl):
    import torch
    from scopa_amd.algorithms import chance
    from scopa_amd.algorithms.deep_cfr import ChanceDeepCFR
    stream = torch.cuda.Stream(device=0)
    c = sl.Context(0, stream=stream.cuda_stream)
    try:
        g = _game(c, sl, X.SIX)
        torch.manual_seed(3)
        d = ChanceDeepCFR(g, batch=8, seed=0x5C09A)
        d.train(iterations=2, advantage_epochs=2)
        avg, scopas = d.evaluate_vs_random(2000)
        assert np.isfinite(avg) and len(scopas) == 2 and all(np.isfinite(x) for x in scopas)
        want_avg, want = chance.evaluate(g, d.policy_table(), 2000)
        assert avg == want_avg and scopas == [want["trained_avg"], want["opponent_avg"]]
        assert d.last_eval_by_seat == want["by_seat"] and [h["episodes"] for h in d.last_eval_by_seat] == [1000, 1000]
        assert abs(avg - want["exact_reward"]) <= 5.0 * want["reward_std_error"]
    finally:
        c.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_alone(ctx, sl, oracle):
    import torch
    L = sl.lib()
    s = X.six(oracle)
    ref_per, ref_out = X.six_cross(oracle)
    g = _game(ctx, sl, X.SIX)
    stack = _dev(s["pols"][:2])
    before = stack.clone()
    out = torch.zeros((2, 2, 4), dtype=torch.float64, device="cuda:0")
    per = torch.zeros((6, 2, 2, 4), dtype=torch.float64, device="cuda:0")
    br = torch.zeros((2, 2, g.G, 4), dtype=torch.float64, device="cuda:0")
    idx = torch.zeros(16, dtype=torch.int32, device="cuda:0")
    st = np.full(10, 7, np.int64)
    P, O, D, B, I = stack.data_ptr(), out.data_ptr(), per.data_ptr(), br.data_ptr(), idx.data_ptr()
    torch.cuda.synchronize()
    for n_pol in (0, 257, -1):
        assert L.scopa_chance_cross_play(g._h, n_pol, P, D, O) == sl.SCOPA_EINVAL
        assert L.scopa_chance_best_response(g._h, n_pol, P, B, O) == sl.SCOPA_EINVAL
    assert L.scopa_chance_cross_play(g._h, 2, None, D, O) == sl.SCOPA_EINVAL and L.scopa_chance_cross_play(g._h, 2, P, D, None) == sl.SCOPA_EINVAL
    assert L.scopa_chance_cross_play(None, 2, P, D, O) == sl.SCOPA_EINVAL
    assert L.scopa_chance_best_response(g._h, 2, None, B, O) == sl.SCOPA_EINVAL and L.scopa_chance_best_response(g._h, 2, P, B, None) == sl.SCOPA_EINVAL
    assert L.scopa_chance_best_response(None, 2, P, B, O) == sl.SCOPA_EINVAL
    assert L.scopa_chance_match(g._h, None, P, 10, 5, 0, I, I, sl._ptr(st)) == sl.SCOPA_EINVAL
    assert L.scopa_chance_match(g._h, P, None, 10, 5, 0, I, I, sl._ptr(st)) == sl.SCOPA_EINVAL
    assert L.scopa_chance_match(g._h, P, P, 10, 5, 0, I, I, None) == sl.SCOPA_EINVAL
    assert L.scopa_chance_match(g._h, P, P, 10, 11, 0, I, I, sl._ptr(st)) == sl.SCOPA_EINVAL
    assert L.scopa_chance_match(g._h, P, P, 10, -1, 0, I, I, sl._ptr(st)) == sl.SCOPA_EINVAL
    assert L.scopa_chance_match(g._h, P, P, -1, 0, 0, I, I, sl._ptr(st)) == sl.SCOPA_EINVAL
    assert L.scopa_chance_debug_scratch_budget(g._h, -1) == sl.SCOPA_EINVAL
    assert (st == 7).all()
    try:
        ctx.debug_lds_limit(KB64)
        # include/scopa.h: 32 * I_max + 36 864 + 3 312 bytes; the six deals' largest has 1 142 infosets: 76 720 bytes
        assert max(s["cref"].I) == 1142
        assert L.scopa_chance_cross_play(g._h, 2, P, D, O) == sl.SCOPA_ELIMIT
        assert L.scopa_chance_cross_play(g._h, 2, P, None, O) == sl.SCOPA_ELIMIT
    finally:
        ctx.debug_lds_limit(0)
    ctx.synchronize()
    assert (out.cpu().numpy() == 0.0).all() and (per.cpu().numpy() == 0.0).all() and (br.cpu().numpy() == 0.0).all() and (idx.cpu().numpy() == 0).all()
    assert torch.equal(stack, before)                                                   # nothing was launched, nothing written
    got_per, got_out = _cross(g, stack)
    assert same_bits(got_per, ref_per[:, :2, :2]) and same_bits(got_out, ref_out[:2, :2])
    assert same_bits(_best(g, stack, tables=False)[0], np.stack([X.six_best(oracle, 0)[0], X.six_best(oracle, 1)[0]]))


def test_cross_play_under_a_64_kib_lds_limit(ctx, sl, oracle):
    """The first three of the six deals have 308, 436 and 625 infosets (<= 792: 32 * 625 + 40 176 = 60 176 bytes): cross-play runs under the limit
    with the bits it has without it -- per deal the six-deal run's, the tables carried over by key."""
    s = X.six(oracle)
    c = s["cref"]
    ref_per, _ = X.six_cross(oracle)
    assert c.I[:3] == [308, 436, 625]
    g = _game(ctx, sl, X.SIX[:3])
    keys, _ = g.index()
    pols = s["pols"][:, np.searchsorted(c.keys, keys)]
    assert np.array_equal(c.keys[np.searchsorted(c.keys, keys)], keys)
    stack = _dev(pols)
    per, out = _cross(g, stack)
    assert same_bits(per, ref_per[:3])
    with np.errstate(invalid="ignore"):
        assert same_bits(out, ((ref_per[0] + ref_per[1]) + ref_per[2]) / 3.0)
    try:
        ctx.debug_lds_limit(KB64)
        per_l, out_l = _cross(g, stack)
    finally:
        ctx.debug_lds_limit(0)
    assert same_bits(per_l, per) and same_bits(out_l, out)


def test_too_many_workgroups_is_refused(ctx, sl):
    """n * n_pol * n_pol >= 2^31: 32 768 copies of one deal and 256 policies.  Refused before any pointer is looked at."""
    import torch
    perm = sl.deal_py_seed(42)
    g = _game(ctx, sl, np.tile(perm, (32768, 1)))
    small = torch.zeros(64, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    L = sl.lib()
    assert L.scopa_chance_cross_play(g._h, 256, small.data_ptr(), None, small.data_ptr()) == sl.SCOPA_ELIMIT
    ctx.synchronize()
    assert (small.cpu().numpy() == 0.0).all()
