"""scopa_cross_play, scopa_best_response and scopa_eval_pair_match (scopa_amd/csrc/scopa_xplay.hip) and the Python layer on them, on the GPU.

The exact kernels are held BIT FOR BIT to tests/xplay_ref.py (a float64 numpy restatement that tests/test_xplay_ref.py anchors to the C oracle) and
to scopa_exploitability; the sampled match episode for episode to the restatement's Philox walks, and its mean to the exact value within five
standard errors taken from the exact second moment.  Two deals (py seeds 42 and 7: 738 and 702 infosets), six tables each (xplay_ref.policy_set):
uniform, an average policy, a Dirichlet table, one with zeros in legal slots, two random one-hot tables."""
import numpy as np
import pytest

from cfr_edges import same_bits
from xplay_ref import Ref, policy_set

pytestmark = pytest.mark.gpu

KB64 = 64 * 1024
ORDER = ("average", "dirichlet", "zeros", "uniform", "onehot_a", "onehot_b")
SUBSETS = {1: (1,), 2: (0, 4), 3: (2, 3, 5), 6: (0, 1, 2, 3, 4, 5)}


def _case(oracle, deal, _cache={}):
    """(tree, ref, [6][I][4] tables in ORDER, reference matrix [6][6][4], reference best responses) of a deal, computed once"""
    if deal not in _cache:
        t = oracle.Tree(seed=deal)
        ref = Ref(t)
        pols = np.stack([policy_set(t)[k] for k in ORDER])
        matrix = np.array([[ref.cross(a, b) for b in pols] for a in pols])
        brs = [ref.best_response(p) for p in pols]
        for a in (pols, matrix):
            a.setflags(write=False)
        _cache[deal] = (t, ref, pols, matrix, brs)
    return _cache[deal]


def _deal(ctx, sl, oracle, deal):
    case = _case(oracle, deal)
    assert ctx.set_deal(sl.deal_py_seed(deal)) == case[0].n_infosets
    return case


def _dev(a, dtype=None):
    import torch
    return torch.as_tensor(np.array(a, dtype=dtype, order="C"), device="cuda:0")          # a copy: the cached tables are read-only


def _cross(ctx, stack):
    """raw scopa_cross_play of a [K][I][4] device tensor -> numpy [K][K][4]"""
    import torch
    k = stack.shape[0]
    out = torch.full((k, k, 4), -9.0, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    ctx.cross_play(k, stack.data_ptr(), out.data_ptr())
    ctx.synchronize()
    return out.cpu().numpy()


def _best(ctx, stack, tables=True):
    import torch
    k, I = stack.shape[0], stack.shape[1]
    out4 = torch.full((k, 4), -9.0, dtype=torch.float64, device="cuda:0")
    br = torch.full((k, 2, I, 4), -9.0, dtype=torch.float64, device="cuda:0") if tables else None
    torch.cuda.synchronize()
    ctx.best_response(k, stack.data_ptr(), br.data_ptr() if tables else 0, out4.data_ptr())
    ctx.synchronize()
    return out4.cpu().numpy(), br


def _pair(ctx, a, b, n, n_seat0, stream_id, want_idx=True):
    import torch
    idx = torch.full((max(n, 1),), -1, dtype=torch.int32, device="cuda:0") if want_idx else None
    torch.cuda.synchronize()
    st = ctx.eval_pair_match(a.data_ptr(), b.data_ptr(), n, n_seat0, stream_id, idx.data_ptr() if want_idx else 0)
    return st, (idx.cpu().numpy()[:n].astype(np.int64) if want_idx else None)


# ---- cross-play -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pol", [1, 2, 3, 6])
@pytest.mark.parametrize("deal", [42, 7])
def test_cross_play_bits(ctx, sl, oracle, deal, n_pol):
    """All ordered pairs, all four outputs, bit for bit against the restatement; a repeat gives the same bits; the diagonal's value is what
    scopa_exploitability reports for that policy."""
    t, ref, pols, matrix, _ = _deal(ctx, sl, oracle, deal)
    sel = list(SUBSETS[n_pol])
    stack = _dev(pols[sel])
    got = _cross(ctx, stack)
    assert same_bits(got, matrix[np.ix_(sel, sel)]), (deal, n_pol)
    assert same_bits(_cross(ctx, stack), got)
    for j, k in enumerate(sel):
        assert same_bits(got[j, j, 0], ctx.exploitability(policy=pols[k])["value_p0"]), (deal, k)


def test_cross_play_propagates_non_finite_rows_by_ieee_rules(ctx, sl, oracle):
    """Rows are used as given: a NaN in a player-0 row of table 0 reaches every pair with table 0 in seat 0 and no other; an unnormalised table
    (rows x 2 for player 1) scales nothing it should not.  Finite cells bit for bit against the restatement, the others NaN on both sides."""
    t, ref, pols, matrix, _ = _deal(ctx, sl, oracle, 42)
    A, B = pols[1].copy(), pols[0].copy()
    A[int(ref.levels[0]["inf"][0]), 0] = np.nan                                         # the root's infoset: every line of play passes it
    B[ref.player == 1] *= 2.0
    got = _cross(ctx, _dev(np.stack([A, B])))
    want = np.array([[ref.cross(a, b) for b in (A, B)] for a in (A, B)])
    assert np.isnan(got[0]).all() and np.isnan(want[0]).all()
    assert same_bits(got[1], want[1]) and np.isfinite(got[1]).all()


# ---- best response --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deal", [42, 7])
def test_best_response_bits(ctx, sl, oracle, deal):
    """Six policies in one call: out4 bit for bit what scopa_exploitability returns for each and what the restatement gives; the tables equal the
    restatement's exactly; without the tables (NULL) and one policy at a time the same out4."""
    t, ref, pols, _, brs = _deal(ctx, sl, oracle, deal)
    stack = _dev(pols)
    out4, br = _best(ctx, stack)
    tables = br.cpu().numpy()
    for k in range(len(ORDER)):
        e = ctx.exploitability(policy=pols[k])
        assert same_bits(out4[k], [e["exploitability"], e["br0"], e["br1"], e["value_p0"]]), (deal, ORDER[k])
        assert same_bits(out4[k], brs[k][0]), (deal, ORDER[k])
        assert same_bits(tables[k, 0], brs[k][1][0]) and same_bits(tables[k, 1], brs[k][1][1]), (deal, ORDER[k])
    assert same_bits(_best(ctx, stack, tables=False)[0], out4)
    assert same_bits(_best(ctx, stack[2:3].contiguous())[0], out4[2:3])
    assert same_bits(_best(ctx, stack)[0], out4)                                          # run to run


@pytest.mark.parametrize("deal", [42, 7])
def test_best_response_tables_compose_with_cross_play_on_the_device(ctx, sl, oracle, deal):
    """The tables go back into scopa_cross_play without leaving the device: br0_k against P_k earns BR0_k, P_k against br1_k loses BR1_k."""
    import torch
    t, ref, pols, _, _ = _deal(ctx, sl, oracle, deal)
    stack = _dev(pols)
    out4, br = _best(ctx, stack)
    for k in range(len(ORDER)):
        got = _cross(ctx, torch.stack([br[k, 0], stack[k], br[k, 1]]).contiguous())
        assert got[0, 1, 0] == out4[k, 1] and -got[1, 2, 0] == out4[k, 2], (deal, ORDER[k])
        assert out4[k, 1] >= out4[k, 3] >= -out4[k, 2]


# ---- the sampled match ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deal", [42, 7])
def test_one_hot_tables_send_every_episode_of_a_half_to_one_terminal(ctx, sl, oracle, deal):
    t, ref, pols, _, _ = _deal(ctx, sl, oracle, deal)
    a, b = pols[4], pols[5]
    n, first = 1000, 389
    st, idx = _pair(ctx, _dev(a), _dev(b), n, first, 3)
    ta, tb = ref.thresholds(a), ref.thresholds(b)
    t0 = int(ref.episodes(oracle, ta, tb, [0], 3, 0x5C09A)[0])                            # a in seat 0
    t1 = int(ref.episodes(oracle, tb, ta, [first], 3, 0x5C09A)[0])                        # a in seat 1
    assert (idx[:first] == t0).all() and (idx[first:] == t1).all()
    assert st[0].tolist() == ref.match_stats(np.full(first, t0), 0) and st[1].tolist() == ref.match_stats(np.full(n - first, t1), 1)
    assert st[0, 1] == first * int(ref.term_r2[t0, 0]) and st[1, 1] == (n - first) * int(ref.term_r2[t1, 1])


@pytest.mark.parametrize("deal,ia,ib,seed", [(42, 1, 2, None), (7, 0, 1, 987654321123)])
def test_stochastic_match_is_the_restatements_walks_episode_for_episode(ctx, sl, oracle, deal, ia, ib, seed):
    """n = 4 096 with an uneven seat split: every terminal index equals the host's (thresholds, Philox (episode, ply, stream; seed), integer
    compares), the sums are the sums over those terminals; without the index buffer the same sums."""
    t, ref, pols, _, _ = _deal(ctx, sl, oracle, deal)
    if seed is not None:
        ctx.mccfr_seed(seed)
    n, first, sid = 4096, 1901, 21
    a, b = _dev(pols[ia]), _dev(pols[ib])
    st, idx = _pair(ctx, a, b, n, first, sid)
    ta, tb = ref.thresholds(pols[ia]), ref.thresholds(pols[ib])
    s = 0x5C09A if seed is None else seed
    want = np.concatenate([ref.episodes(oracle, ta, tb, range(first), sid, s), ref.episodes(oracle, tb, ta, range(first, n), sid, s)])
    assert np.array_equal(idx, want)
    assert st[0].tolist() == ref.match_stats(want[:first], 0) and st[1].tolist() == ref.match_stats(want[first:], 1)
    assert (_pair(ctx, a, b, n, first, sid, want_idx=False)[0] == st).all()
    assert len(set(want.tolist())) > 50                                                   # a stochastic match indeed
    assert (_pair(ctx, a, b, n, n, sid)[0][1] == 0).all() and (_pair(ctx, a, b, n, 0, sid)[0][0] == 0).all()    # one half only, either way
    assert (_pair(ctx, a, b, 0, 0, sid, want_idx=False)[0] == 0).all()


def _within_five_standard_errors(st, exact_halves):
    """st int64 [2][5]; exact_halves = per seat half (value, second moment) of the policy of interest's reward"""
    for half, (v, m2) in enumerate(exact_halves):
        m = int(st[half, 0])
        mean = st[half, 1] / 2 / m
        se = np.sqrt((m2 - v * v) / m)
        print(f"half {half}: sampled {mean:+.6f}, exact {v:+.6f}, standard error {se:.6f}, off by {abs(mean - v) / se:.2f} SE")
        assert se > 0.0 and abs(mean - v) <= 5.0 * se, (half, mean, v, se)


@pytest.mark.parametrize("deal", [42, 7])
def test_sample_means_lie_within_five_standard_errors_of_the_exact_values(ctx, sl, oracle, deal):
    """n = 2 x 65 536, fixed Philox seed.  The pair match against cross_play of the two tables, and the EXISTING scopa_eval_tabular_match against
    cross_play(policy, uniform): per seat half |mean - v| <= 5 sqrt((m2 - v^2) / n), v and m2 exact."""
    t, ref, pols, _, _ = _deal(ctx, sl, oracle, deal)
    m = 65536
    a, b, u = pols[0], pols[1], pols[3]
    x = _cross(ctx, _dev(np.stack([a, b, u])))
    st, _ = _pair(ctx, _dev(a), _dev(b), 2 * m, m, 40, want_idx=False)
    assert st[:, 0].tolist() == [m, m]
    _within_five_standard_errors(st, [(x[0, 1, 0], x[0, 1, 1]), (-x[1, 0, 0], x[1, 0, 1])])
    pa = _dev(a)
    ctx.eval_tabular_prepare(pa.data_ptr())
    st = ctx.eval_tabular_match(2 * m, m, 41)
    _within_five_standard_errors(st, [(x[0, 2, 0], x[0, 2, 1]), (-x[2, 0, 0], x[2, 0, 1])])
    for half, (own, opp) in enumerate([(x[0, 2, 2], x[0, 2, 3]), (x[2, 0, 3], x[2, 0, 2])]):   # scopas: a count X <= 4 (four cards a seat), so Var X <= E X^2 <= 4 E X
        for col, v in ((3, own), (4, opp)):
            assert abs(st[half, col] / m - v) <= 5.0 * np.sqrt(4.0 * max(v, 1e-3) / m)


@pytest.mark.parametrize("deal,k", [(42, 2), (7, 1)])
def test_pair_thresholds_are_the_prepared_thresholds(ctx, sl, oracle, deal, k):
    """k_pair_thresholds restates k_eval_thresholds: a pair match of P against the UNIFORM table walks the episodes scopa_eval_tabular_match walks for
    P prepared -- P's seat by either kernel's thresholds, the other seat #{c : ceil(c / n * 2^53) <= N} = floor(N * n / 2^53), the uniform opponent's
    choice (the two can differ only where c / n rounds across an integer multiple of 2^-53: not at these draws)."""
    import torch
    t, ref, pols, _, _ = _deal(ctx, sl, oracle, deal)
    n, first, sid = 4096, 2100, 13
    p = _dev(pols[k])
    ctx.eval_tabular_prepare(p.data_ptr())
    idx = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    want = ctx.eval_tabular_match(n, first, sid, 0, idx.data_ptr())
    st, got = _pair(ctx, p, _dev(pols[3]), n, first, sid)
    assert np.array_equal(got, idx.cpu().numpy()) and (st == want).all()


def test_a_pair_match_leaves_the_prepared_thresholds_alone(ctx, sl, oracle):
    t, ref, pols, _, _ = _deal(ctx, sl, oracle, 42)
    p = _dev(pols[1])
    ctx.eval_tabular_prepare(p.data_ptr())
    before = ctx.eval_tabular_match(5001, 2501, 8)
    _pair(ctx, _dev(pols[2]), _dev(pols[4]), 3000, 1500, 8)
    assert (ctx.eval_tabular_match(5001, 2501, 8) == before).all()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx, sl, oracle):
    import torch
    L = sl.lib()
    t, ref, pols, matrix, brs = _case(oracle, 42)
    stack = _dev(pols[:2])
    out = torch.zeros((2, 2, 4), dtype=torch.float64, device="cuda:0")
    br = torch.zeros((2, 2, t.n_infosets, 4), dtype=torch.float64, device="cuda:0")
    st = np.zeros(10, np.int64)
    P, O, B = stack.data_ptr(), out.data_ptr(), br.data_ptr()
    torch.cuda.synchronize()
    assert L.scopa_cross_play(ctx._h, 2, P, O) == sl.SCOPA_ESTATE                       # no deal yet
    assert L.scopa_best_response(ctx._h, 2, P, B, O) == sl.SCOPA_ESTATE
    assert L.scopa_eval_pair_match(ctx._h, P, P, 10, 5, 0, None, sl._ptr(st)) == sl.SCOPA_ESTATE
    _deal(ctx, sl, oracle, 42)
    for n_pol in (0, 257, -1):
        assert L.scopa_cross_play(ctx._h, n_pol, P, O) == sl.SCOPA_EINVAL
        assert L.scopa_best_response(ctx._h, n_pol, P, B, O) == sl.SCOPA_EINVAL
    assert L.scopa_cross_play(ctx._h, 2, None, O) == sl.SCOPA_EINVAL and L.scopa_cross_play(ctx._h, 2, P, None) == sl.SCOPA_EINVAL
    assert L.scopa_best_response(ctx._h, 2, None, B, O) == sl.SCOPA_EINVAL and L.scopa_best_response(ctx._h, 2, P, B, None) == sl.SCOPA_EINVAL
    assert L.scopa_eval_pair_match(ctx._h, None, P, 10, 5, 0, None, sl._ptr(st)) == sl.SCOPA_EINVAL
    assert L.scopa_eval_pair_match(ctx._h, P, None, 10, 5, 0, None, sl._ptr(st)) == sl.SCOPA_EINVAL
    assert L.scopa_eval_pair_match(ctx._h, P, P, 10, 5, 0, None, None) == sl.SCOPA_EINVAL
    assert L.scopa_eval_pair_match(ctx._h, P, P, 10, 11, 0, None, sl._ptr(st)) == sl.SCOPA_EINVAL
    assert L.scopa_eval_pair_match(ctx._h, P, P, -1, 0, 0, None, sl._ptr(st)) == sl.SCOPA_EINVAL
    ctx.synchronize()
    assert (out.cpu().numpy() == 0.0).all() and (br.cpu().numpy() == 0.0).all()         # nothing was launched
    try:
        ctx.debug_lds_limit(KB64)
        # include/scopa.h: the best-response kernel needs 89 160 bytes at 738 infosets, the cross-play kernel 63 792
        with pytest.raises(sl.ScopaError) as e:
            ctx.best_response(2, P, B, O)
        assert e.value.status == sl.SCOPA_ELIMIT
        assert same_bits(_cross(ctx, stack), matrix[:2, :2])
    finally:
        ctx.debug_lds_limit(0)
    assert same_bits(_best(ctx, stack)[0], np.stack([brs[0][0], brs[1][0]]))


# ---- the Python layer -----------------------------------------------------------------------------------------------------------------
def test_python_layer(ctx, sl, oracle):
    import torch
    from scopa_amd.algorithms import evaluation as E
    t, ref, pols, matrix, brs = _deal(ctx, sl, oracle, 7)
    E.check_policy_table(ctx, pols[0])
    E.check_policy_table(ctx, pols)
    E.check_policy_table(ctx, _dev(pols[2]))
    bad = pols[1].copy()
    r = int(np.flatnonzero(ref.nlegal == 2)[0])
    bad[r, 3] = 0.25                                                                    # mass on an illegal slot
    with pytest.raises(ValueError):
        E.check_policy_table(ctx, bad)
    bad = pols[1].copy()
    bad[r] *= 0.9                                                                       # a row summing to 0.9
    with pytest.raises(ValueError):
        E.check_policy_table(ctx, bad)
    with pytest.raises(ValueError):
        E.check_policy_table(ctx, pols[0][:-1])
    with pytest.raises(ValueError):
        E.cross_play(ctx, [pols[0], bad])
    with pytest.raises(ValueError):
        E.best_response(ctx, bad)
    for given in (pols, [p for p in pols], _dev(pols), [_dev(p) for p in pols]):
        x = E.cross_play(ctx, given)
        assert same_bits(x["reward"], matrix[..., 0]) and same_bits(x["scopas"], matrix[..., 2:])
        assert same_bits(x["reward_std"], np.sqrt(np.maximum(matrix[..., 1] - matrix[..., 0] * matrix[..., 0], 0.0)))
    assert x["reward"].shape == (6, 6) and x["reward_std"].shape == (6, 6) and x["scopas"].shape == (6, 6, 2)
    b = E.best_response(ctx, pols[1])
    e = ctx.exploitability(policy=pols[1])
    assert (b["exploitability"], b["br_values"], b["value"]) == (e["exploitability"], (e["br0"], e["br1"]), e["value_p0"])
    assert same_bits(b["tables"][0], brs[1][1][0]) and same_bits(b["tables"][1], brs[1][1][1])
    E.check_policy_table(ctx, np.stack(b["tables"]))                                    # ... and they are policies


def test_evaluate_agent_device_against_a_table(ctx, sl, oracle):
    from scopa_amd.algorithms import CFRTrainer, evaluate_agent_device
    from scopa_amd.envs.openspiel_mini_scopa import MiniScopaGame
    t, ref, pols, _, _ = _case(oracle, 42)
    tr = CFRTrainer(MiniScopaGame(seed=42), mode="sync")
    try:
        tr.train(20)
        avg, stats = evaluate_agent_device(tr, 40001, stream_id=5, opponent=pols[1])
        policy = tr._engine.ctx.exploitability(return_policy=True)["policy"]
        exact = (20001 * ref.cross(policy, pols[1])[0] - 20000 * ref.cross(pols[1], policy)[0]) / 40001
        assert stats["exact_reward"] == exact
        print(f"sampled {avg:+.5f}, exact {exact:+.5f}, standard error {stats['reward_std_error']:.5f}")
        assert abs(avg - stats["exact_reward"]) <= 5.0 * stats["reward_std_error"]
        assert [h["episodes"] for h in stats["by_seat"]] == [20001, 20000] and stats["data_collected"]
        assert {"trained_avg", "opponent_avg", "difference", "reward_std_error", "by_seat", "exact_reward"} <= set(stats)
        avg0, stats0 = evaluate_agent_device(tr, 4001, stream_id=5)                       # no opponent: today's path, today's fields
        assert "exact_reward" not in stats0 and stats0["by_seat"][0]["episodes"] == 2001
        with pytest.raises(ValueError):
            evaluate_agent_device(tr, 100, opponent=pols[1], per_ply=True)
    finally:
        tr._engine.close()
