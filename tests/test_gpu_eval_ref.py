"""The net-policy evaluator on the device (scopa_eval_init_states, scopa_features_from_states, scopa_eval_step: scopa_amd/csrc/scopa_sdcfr.hip) and
DeepCFR.evaluate_vs_random built on it, held EXACTLY to tests/eval_ref.py (a plain CPU restatement over the oracle's State, anchored on the CPU
by tests/test_eval_ref.py): packed states field for field after every ply of every episode, float32 features as bits.  No tolerances.

What these tests see, tried on mutated copies of the kernel: the hand order reversed at one ply, Philox keyed on i + 1, and a chunked initialisation
that leaves row 65 535 out each fail here; so did the kernel before it took the reference's fallback rule (a NaN in one legal slot beside positive
mass: 101-113 of 4 099 episodes differed at ply 0).  What they cannot see: `u <= c` in place of `u < c` differs only where a draw EQUALS a cumulative
sum (u = 0 under a one-hot row), one draw in 2^53; the strictness of the rule is pinned on the restatement (test_eval_ref.py::test_sampling_rule_edges)."""
import sys

import numpy as np
import pytest

import eval_ref as R

pytestmark = pytest.mark.gpu

DEFAULT_SEED = 0x5C09A                   # scopa_ctx's seed before any scopa_mccfr_seed (scopa_ctx.h); DeepCFR's default too
WIDE_SEED = 0xC2B2AE3D27D4EB4F           # a 64-bit seed with a non-zero high word: the second Philox key word
SENTINEL = 0x5A5A5A5A
CATEGORIES = ("dirichlet over the hand", "one-hot on a legal card", "all mass on cards not in hand", "all zero",
              "one NaN in a legal slot, positive mass elsewhere", "NaN only in illegal slots", "all NaN",
              "a negative entry beside positive ones", "denormal-only mass (1e-42)", "entries of 3e38")


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")


def _states_dev(packed, extra=0):
    """STATE_DTYPE [n] -> int32 [n + extra][4] device tensor, the extra rows filled with the sentinel"""
    buf = np.full((packed.size + extra, 4), SENTINEL, np.uint32)
    buf[:packed.size] = packed.view(np.uint32).reshape(-1, 4)
    return _dev(buf.view(np.int32))


def _states_host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint32).reshape(-1).view(R.STATE_DTYPE)


def _differ(got, want):
    """indices of the states that differ in any of their 16 bytes"""
    assert got.shape == want.shape and got.dtype == want.dtype == R.STATE_DTYPE
    a, b = (np.ascontiguousarray(x).view(np.uint32).reshape(-1, 4) for x in (got, want))
    return np.flatnonzero((a != b).any(1))


def _assert_states(got, want, what):
    bad = _differ(got, want)
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {want.size} episodes differ; first episode {i}: device {got[i]} restatement {want[i]}")


def _seed(ctx, seed):
    if seed != DEFAULT_SEED:
        ctx.mccfr_seed(seed)


# ---- scopa_eval_init_states ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deal", [42, 7])
@pytest.mark.parametrize("n", [1, 65535, 65536, 65537])          # the host loop copies the root in chunks of 65 536 states
def test_eval_init_states_every_row_is_the_root(ctx, oracle, n, deal):
    import torch
    perm = oracle.deal_py_seed(deal)
    ctx.set_deal(perm)
    buf = torch.full((n + 1, 4), SENTINEL, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    ctx.eval_init_states(buf.data_ptr(), n)
    got = buf.cpu().numpy().view(np.uint32)
    root = R.pack(R.root_state(perm))
    assert list(root["hand"]) == [sum(int(perm[4 * p + i]) << (4 * i) for i in range(4)) for p in (0, 1)] and root["step"] == 0
    want = np.empty(n, R.STATE_DTYPE)
    want[:] = root
    _assert_states(got[:n].reshape(-1).view(R.STATE_DTYPE), want, f"init n={n} deal={deal}")
    assert (got[n] == SENTINEL).all()                               # the row past the end is untouched


# ---- scopa_features_from_states --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def feature_states(oracle):
    """260 states and their restated features: random play stopped at every ply 0..8 (terminal states included) on ten deals, and clones
    (step limit 16) pushed past step 8 with no-op actions (cards not in the mover's hand), some of them up to the limit."""
    rng = np.random.RandomState(17)
    states = []
    for k in range(260):
        st = R.root_state(oracle.deal_py_seed(int(rng.randint(10))))
        for _ in range(k % 9):
            lg = st.legal()
            st.step(lg[rng.randint(len(lg))])
        if k % 4 == 3 and not st.is_terminal():
            st = st.clone()
            target = int(rng.choice([9, 10, 11, 13, 16]))
            while int(st.s.step) < target and not st.is_terminal():
                p = int(st.s.step) & 1
                hand = [int(st.s.hand[p][i]) for i in range(st.s.nh[p])]
                if hand and rng.rand() < 0.3:
                    st.step(hand[rng.randint(len(hand))])
                else:
                    st.step([c for c in range(16) if c not in hand][rng.randint(16 - len(hand))])
        states.append(st)
    order = rng.permutation(260)
    states = [states[i] for i in order]
    packed = R.pack_all(states)
    steps = packed["step"] & 0x7F
    cloned = (packed["step"] & R.STEP_CLONED) != 0
    term = np.array([s.is_terminal() for s in states])
    assert set(steps[~cloned]) == set(range(9)) and (cloned & (steps > 8) & ~term).sum() >= 10 and (cloned & (steps == 16)).sum() >= 3
    assert (term & ~cloned).sum() >= 15 and not (cloned[:1] | term[:1]).any()
    fm = [R.features(s) for s in states]
    return packed, np.stack([f for f, _ in fm]), np.stack([m for _, m in fm])


@pytest.mark.parametrize("n", [1, 255, 256, 257])                 # one block is 256 lanes
def test_features_from_states_bits(ctx, feature_states, n):
    import torch
    packed, want_f, want_m = feature_states
    st = _states_dev(packed[:n])
    feats = torch.full((n + 2, 34), -7.5, dtype=torch.float32, device="cuda:0")
    mask = torch.full((n + 2, 16), -7.5, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    ctx.features_from_states(st.data_ptr(), n, feats.data_ptr(), mask.data_ptr())
    torch.cuda.synchronize()
    f, m = feats.cpu().numpy(), mask.cpu().numpy()
    assert np.array_equal(f[:n].view(np.uint32), want_f[:n].view(np.uint32))
    assert np.array_equal(m[:n].view(np.uint32), want_m[:n].view(np.uint32))
    assert (f[n:] == -7.5).all() and (m[n:] == -7.5).all()          # rows beyond n are untouched
    assert np.array_equal(_states_host(st), packed[:n])             # the states are read only


# ---- scopa_eval_step ---------------------------------------------------------------------------------------------------------------------
def _category_row(cat, hand, rng):
    """One float32 [16] policy row of category `cat` for a mover holding `hand` (hand order)."""
    nan = np.float32(np.nan)
    off = [c for c in range(16) if c not in hand]
    k = len(hand)
    row = np.zeros(16, np.float32)
    if cat == 0:
        row[hand] = rng.dirichlet(np.full(k, 0.8))
    elif cat == 1:
        row[hand[rng.randint(k)]] = 1.0
    elif cat == 2:
        row[off] = rng.dirichlet(np.ones(len(off)))
    elif cat == 3:
        pass
    elif cat == 4:                      # the reference plays uniform here, whatever the other slots hold
        row[hand] = rng.dirichlet(np.full(k, 0.8)) + 0.05
        row[off] = 0.01
        row[hand[rng.randint(k)]] = nan
    elif cat == 5:                      # slots of cards not in hand are never read
        row[hand] = rng.dirichlet(np.full(k, 0.8))
        row[off] = nan
    elif cat == 6:
        row[:] = nan
    elif cat == 7:
        row[hand] = rng.dirichlet(np.full(k, 0.8)) + 0.05
        row[off] = 0.02
        row[hand[rng.randint(k)]] = -rng.rand() - 0.1
    elif cat == 8:
        sel = rng.rand(k) < 0.6
        sel[rng.randint(k)] = True
        row[np.array(hand)[sel]] = np.float32(1e-42) * rng.randint(1, 4, sel.sum()).astype(np.float32)
    elif cat == 9:
        sel = rng.rand(k) < 0.7
        sel[rng.randint(k)] = True
        row[np.array(hand)[sel]] = 3e38
        row[off[0]] = 3e38
    return row


def _ply_probs(states, seat, rng, counts):
    """probs [n][16] for this ply: a seeded category per lane; `counts` tallies the categories that reach a trained-seat move."""
    n = len(states)
    probs = np.zeros((n, 16), np.float32)
    cats = rng.randint(len(CATEGORIES), size=n)
    for i, st in enumerate(states):
        p = int(st.s.step) & 1
        hand = [int(st.s.hand[p][q]) for q in range(st.s.nh[p])]
        if not hand:
            continue
        probs[i] = _category_row(int(cats[i]), hand, rng)
        if p == seat[i]:
            counts[cats[i]] += 1
    return probs, cats


@pytest.mark.parametrize("seed", [DEFAULT_SEED, WIDE_SEED])
@pytest.mark.parametrize("deal", [42, 7])
@pytest.mark.parametrize("n", [1, 257, 4099])                       # a lone lane; one block + 1; 16 blocks + 3
def test_eval_step_eight_plies_every_episode(ctx, oracle, n, deal, seed):
    """Eight plies of n episodes, the states compared with the restatement after EVERY ply; the trained seat's rows cycle through the categories
    above (drawn per lane per ply), the seats split at (n + 1) // 2 as evaluate_vs_random splits them; then a ninth step, which must change nothing."""
    perm = oracle.deal_py_seed(deal)
    ctx.set_deal(perm)
    _seed(ctx, seed)
    rng = np.random.RandomState(1000 + n)
    seat = (np.arange(n) >= (n + 1) // 2).astype(np.int32)
    cpu = [R.root_state(perm) for _ in range(n)]
    st = _states_dev(R.pack_all(cpu), extra=1)
    d_seat = _dev(seat)
    counts = np.zeros(len(CATEGORIES), np.int64)
    for ply in range(8):
        probs, cats = _ply_probs(cpu, seat, rng, counts)
        d_probs = _dev(probs)
        tag = (3 << 4) | ply
        before = R.pack_all(cpu)
        ctx.eval_step(st.data_ptr(), n, d_probs.data_ptr(), d_seat.data_ptr(), 8, tag)
        R.eval_step(cpu, probs, seat, seed, 8, tag)
        got, want = _states_host(st), R.pack_all(cpu)
        bad = _differ(got[:n], want)
        if bad.size:
            i = int(bad[0])
            trained = (before["step"][bad] & 1) == seat[bad]
            by_cat = {CATEGORIES[c]: int(((cats[bad] == c) & trained).sum()) for c in range(len(CATEGORIES)) if ((cats[bad] == c) & trained).any()}
            raise AssertionError(f"ply {ply}: {bad.size} of {n} episodes differ ({int((~trained).sum())} on a random-seat move; trained-seat moves by "
                                 f"category: {by_cat}); first: episode {i}, seat {seat[i]}, category '{CATEGORIES[cats[i]]}', row {probs[i]}, "
                                 f"before {before[i]}, device {got[i]}, restatement {want[i]}")
        assert (got[n:].view(np.uint32) == SENTINEL).all()
    assert all(s.is_terminal() for s in cpu) and (R.pack_all(cpu)["step"] == 8).all()
    if n == 4099:
        assert counts.min() >= 20, dict(zip(CATEGORIES, counts))    # a condition on the inputs: every category reaches the trained seat
    final = R.pack_all(cpu)
    ctx.eval_step(st.data_ptr(), n, _dev(np.full((n, 16), 0.0625, np.float32)).data_ptr(), d_seat.data_ptr(), 8, (3 << 4) | 8)
    _assert_states(_states_host(st)[:n], final, "a ninth step on the all-terminal batch")


@pytest.mark.parametrize("seed", [DEFAULT_SEED, WIDE_SEED])
def test_eval_step_without_probs_both_seats_uniform(ctx, oracle, seed):
    """probs = NULL: both seats play uniform, whatever the seat array says."""
    n = 257
    perm = oracle.deal_py_seed(7)
    ctx.set_deal(perm)
    _seed(ctx, seed)
    seat = (np.arange(n) >= (n + 1) // 2).astype(np.int32)
    cpu = [R.root_state(perm) for _ in range(n)]
    st = _states_dev(R.pack_all(cpu), extra=1)
    d_seat = _dev(seat)
    for ply in range(8):
        ctx.eval_step(st.data_ptr(), n, 0, d_seat.data_ptr(), 5, 100 + ply)
        R.eval_step(cpu, None, seat, seed, 5, 100 + ply)
        _assert_states(_states_host(st)[:n], R.pack_all(cpu), f"probs=NULL ply {ply}")
    assert len({bytes(s) for s in R.pack_all(cpu)}) > 20            # the lanes do not all play the same game


def test_eval_step_terminal_and_cloned_terminal_states_are_left_alone(ctx, feature_states):
    """Terminal states in the batch -- clones at their step limit of 16 among them -- come back unchanged."""
    packed = feature_states[0]
    steps, cloned = packed["step"] & 0x7F, (packed["step"] & R.STEP_CLONED) != 0
    nh = packed["nh"].astype(np.int64).sum(1)
    term = (nh == 0) | (steps >= np.where(cloned, 16, 8))
    sel = packed[term]
    assert (cloned[term] & (steps[term] == 16) & (nh[term] > 0)).sum() >= 3 and sel.size >= 30
    st = _states_dev(sel, extra=1)
    n = sel.size
    ctx.eval_step(st.data_ptr(), n, _dev(np.full((n, 16), 0.0625, np.float32)).data_ptr(), _dev(np.zeros(n, np.int32)).data_ptr(), 8, 1)
    got = _states_host(st)
    _assert_states(got[:n], sel, "terminal states")
    assert (got[n:].view(np.uint32) == SENTINEL).all()


def test_eval_step_same_tag_reproduces_another_tag_differs(ctx, oracle):
    n = 257
    perm = oracle.deal_py_seed(42)
    ctx.set_deal(perm)
    seat = np.zeros(n, np.int32)
    root = R.pack_all([R.root_state(perm)] * n)
    probs = np.zeros((n, 16), np.float32)
    probs[:, perm[:4]] = np.array([0.1, 0.2, 0.3, 0.4], np.float32)
    d_probs, d_seat = _dev(probs), _dev(seat)
    out = {}
    for name, (sid, tag) in dict(a=(8, 0x10), again=(8, 0x10), other_tag=(8, 0x20), other_stream=(9, 0x10)).items():
        st = _states_dev(root)
        ctx.eval_step(st.data_ptr(), n, d_probs.data_ptr(), d_seat.data_ptr(), sid, tag)
        out[name] = _states_host(st).copy()
        cpu = [R.root_state(perm) for _ in range(n)]
        R.eval_step(cpu, probs, seat, DEFAULT_SEED, sid, tag)
        _assert_states(out[name], R.pack_all(cpu), name)
    assert np.array_equal(out["a"], out["again"])
    assert _differ(out["a"], out["other_tag"]).size > n // 4 and _differ(out["a"], out["other_stream"]).size > n // 4
    played = [int(np.flatnonzero(perm[:4] == (s["table"] & 15))[0]) for s in out["a"]]       # the card laid on the empty table, as a hand position
    assert np.bincount(played, minlength=4).argmax() == 3 and len(set(played)) == 4           # weights 0.1 .. 0.4 in HAND order


# ---- DeepCFR.evaluate_vs_random end to end ---------------------------------------------------------------------------------------------------
def _tensor_at(frame, ptr):
    """the tensor among the caller's locals that starts at device address ptr"""
    import torch
    for v in frame.f_locals.values():
        if isinstance(v, torch.Tensor) and v.is_cuda and v.data_ptr() == ptr:
            return v
    raise AssertionError("no tensor of the caller starts at the pointer handed to eval_step")


def test_evaluate_vs_random_is_the_restatements_episodes(oracle, golden):
    """DeepCFR.evaluate_vs_random with the fixture's two nets as the only snapshots, n = 1 001 (501 episodes in seat 0): the probs, seats and tags
    it hands to ctx.eval_step are recorded as host copies and replayed through the restatement from the root -- the float32 forward pass is never
    redone on the CPU.  Final states, returned figures, history entries and last_eval_by_seat must be the restatement's."""
    import torch
    from scopa_amd.algorithms.deep_cfr import DeepCFR, FlexibleNet
    from scopa_amd.envs import load_game
    g = golden.npz("sdcfr.npz")
    d = DeepCFR(load_game("mini_scopa"), num_players=2, device="cuda:0")
    for p in range(2):
        sd = {str(k): torch.from_numpy(g[f"net{p}__{k}"]) for k in g[f"net{p}_names"]}
        snap = FlexibleNet(mode="mlp", input_shape=(34,), output_dim=16, mlp_hidden=[128, 64]).to("cuda:0")
        snap.load_state_dict(sd)
        d.strategy_buffers[p].add_strategy(snap, 1)
    ctx = d._engine.ctx
    inner = ctx.eval_step
    calls = []

    def recording(states_ptr, n, probs_ptr, seat_ptr, stream_id, ply_tag):
        fr = sys._getframe(1)
        states, probs, seat = _tensor_at(fr, states_ptr), _tensor_at(fr, probs_ptr), _tensor_at(fr, seat_ptr)
        rec = dict(n=n, stream=stream_id, tag=ply_tag, probs=probs.cpu().numpy().copy(), seat=seat.cpu().numpy().copy())
        inner(states_ptr, n, probs_ptr, seat_ptr, stream_id, ply_tag)
        rec["after"] = states.cpu().numpy().copy().view(np.uint32).reshape(-1).view(R.STATE_DTYPE)
        calls.append(rec)

    n = 1001
    perm = oracle.deal_py_seed(42)
    results = []
    ctx.eval_step = recording
    try:
        for call in (1, 2):
            del calls[:]
            h0 = len(d.training_history["eval_rewards"])
            ret = d.evaluate_vs_random(n)
            assert d._eval_calls == call and [c["tag"] for c in calls] == [(call << 4) | ply for ply in range(8)]
            assert all(c["stream"] == 8 and c["n"] == n and c["probs"].shape == (n, 16) and c["probs"].dtype == np.float32 for c in calls)
            seat = calls[0]["seat"]
            assert all(np.array_equal(c["seat"], seat) for c in calls) and (seat == 0).sum() == 501 and (seat[:501] == 0).all() and (seat[501:] == 1).all()
            cpu = [R.root_state(perm) for _ in range(n)]
            for ply, c in enumerate(calls):
                R.eval_step(cpu, c["probs"], seat, DEFAULT_SEED, c["stream"], c["tag"])
                _assert_states(c["after"], R.pack_all(cpu), f"evaluate_vs_random call {call}, ply {ply}")
            final = R.pack_all(cpu)
            avg, scopas, halves = R.match_numbers(final, seat)
            assert ret == (avg, scopas)
            assert len(d.training_history["eval_rewards"]) == h0 + 1 == len(d.training_history["eval_scopas"])
            assert d.training_history["eval_rewards"][-1] == avg and d.training_history["eval_scopas"][-1] == scopas
            assert d.last_eval_by_seat == halves and [h["episodes"] for h in halves] == [501, 500]
            results.append(final)
    finally:
        del ctx.eval_step
    assert _differ(results[0], results[1]).size > n // 4             # the second call draws under the next tag: other episodes
    mid = calls[2]["probs"][:501]                                    # seat-0 lanes at their second move: real policies, not one row, not flat
    assert len(np.unique(mid, axis=0)) > 3 and ((mid > 0).sum(1) <= 3).all() and (np.abs(mid.sum(1) - 1) < 1e-5).all()
