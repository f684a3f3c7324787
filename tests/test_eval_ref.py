"""CPU checks of the net-policy evaluator's restatement (tests/eval_ref.py), which tests/test_gpu_eval_ref.py holds the device to exactly: its
sampling rule against numpy's inverse-cdf rule, its fallback rule on the reference's own cases (deep_cfr.py:394-397), its features against the
product's host encoders, and its match figures on a hand-made batch."""
import numpy as np

import eval_ref as R

SAMPLING_SEED = 20250117


def _sampling_rows(seed, n=10_000):
    """n rows (float32 policy over 1-4 legal actions, u): Dirichlet rows, and rows with zeros in legal slots (at least one positive entry)."""
    rng = np.random.RandomState(seed)
    rows = []
    for r in range(n):
        k = 1 + r % 4
        p = rng.dirichlet(np.full(k, 0.7)).astype(np.float32)
        if r % 2 and k > 1:
            zero = rng.rand(k) < 0.5
            zero[rng.randint(k)] = False
            p[zero] = 0.0
        if not p.sum() > 0:           # a Dirichlet draw that underflowed to zeros in float32: keep the row inside the rule's domain
            p[0] = 1.0
        rows.append((p, float(rng.random_sample())))
    return rows


def test_sampling_rule_is_numpys_inverse_cdf_on_10k_rows():
    """`first q with u < running sum of w_q / tot` against np.searchsorted(cdf / cdf[-1], u, side="right") on 10 000 seeded rows: the count of rows
    where they differ is asserted to be 0 (no tolerance: normalising with `tot` instead of the last cumulative value moves a boundary by an ulp or
    two, which a draw of this seed does not hit; the seed was chosen with the restatement alone)."""
    differ, zeros, by_k = 0, 0, [0] * 5
    for p, u in _sampling_rows(SAMPLING_SEED):
        k = len(p)
        row = np.zeros(16, np.float32)
        hand = list(range(3, 3 + k))
        row[hand] = p
        w, tot = R.action_weights(row, hand)
        got = R.pick(w, tot, u)
        cdf = np.cumsum(p.astype(np.float64))
        want = int(np.searchsorted(cdf / cdf[-1], u, side="right"))
        differ += got != want
        zeros += bool((p == 0).any())
        by_k[k] += 1
        assert p[got] > 0                          # a zero slot is never played
    assert differ == 0, differ
    assert by_k[1:] == [2500] * 4 and zeros > 1500


def test_sampling_rule_edges():
    w, tot = R.action_weights(np.array([0, 1, 0, 0] + [0] * 12, np.float32), [0, 1, 2])
    assert (w, tot) == ([0.0, 1.0, 0.0], 1.0)
    assert [R.pick(w, tot, u) for u in (0.0, 0.5, 1.0 - 2.0 ** -53)] == [1, 1, 1]       # one-hot: u < 0 never, u < 1 always
    w, tot = R.action_weights(None, [5, 9])
    assert (w, tot) == ([1.0, 1.0], 2.0)
    assert [R.pick(w, tot, u) for u in (0.0, 0.5 - 2.0 ** -54, 0.5, 1.0 - 2.0 ** -53)] == [0, 0, 1, 1]    # strict <: u == c goes to the next action
    assert R.pick([1.0, 1.0, 1.0], 3.0, 1.0) == 2                                         # nothing found: the last action
    assert R.u53(0xFFFFFFFF, 0xFFFFFFFF) == 1.0 - 2.0 ** -53 and R.u53(0, 0) == 0.0 and R.u53(1 << 5, 0) == 2.0 ** -27


def test_fallback_rule_on_the_references_cases():
    """deep_cfr.py:394-397: `np.any(np.isnan(action_probs)) or np.sum(action_probs) <= 0` over the LEGAL slots gives uniform."""
    nan = np.float32(np.nan)
    hand = [2, 7, 11]

    def reference(row):
        ap = np.array([row[a] for a in hand], np.float64)
        if np.any(np.isnan(ap)) or np.sum(ap) <= 0:
            return np.ones(3) / 3
        return ap / np.sum(ap)

    def restated(row):
        w, tot = R.action_weights(row, hand)
        return np.array(w) / tot

    def row(**kw):
        r = np.zeros(16, np.float32)
        for k, v in kw.items():
            r[int(k[1:])] = v
        return r

    cases = {"nan in a legal slot": row(c2=nan, c7=0.5, c11=0.5),
             "nan only in an illegal slot": row(c2=0.25, c7=0.5, c11=0.25, c3=nan, c15=nan),
             "all zero": row(),
             "all mass on cards not in hand": row(c0=0.5, c8=0.5),
             "plain": row(c2=0.125, c7=0.5, c11=0.375)}
    for name, r in cases.items():
        assert np.array_equal(restated(r), reference(r)), name
    assert np.array_equal(restated(cases["nan in a legal slot"]), np.ones(3) / 3)
    assert np.array_equal(restated(cases["nan only in an illegal slot"]), [0.25, 0.5, 0.25])
    # outside the reference's domain (np.random.choice raises on a negative probability): the negative entry is clamped to 0 before the sum
    assert np.array_equal(restated(row(c2=-0.5, c7=0.5, c11=1.5)), [0.0, 0.25, 0.75])
    assert np.array_equal(restated(row(c2=-0.5, c7=0.0, c11=0.0)), np.ones(3) / 3)
    # float32 extremes: denormal-only mass and entries of 3e38 are summed in float64
    assert np.array_equal(restated(row(c2=1e-42, c7=0.0, c11=1e-42)), [0.5, 0.0, 0.5])
    big = row(c2=3e38, c7=3e38, c11=3e38)
    assert np.array_equal(restated(big), np.ones(3) / 3) and R.action_weights(big, hand)[1] == 3.0 * float(np.float32(3e38))


def test_features_against_the_host_encoders(sl, oracle):
    """eval_ref.features against DeepCFR._state_to_features / _get_legal_actions_mask on the states of 50 random games (50 deals), every ply 0..8.
    At the terminal state the host encoder returns a zero row before it encodes anything; the (zero) hand and mask are compared there, and the
    restatement's table part with the env's table."""
    from scopa_amd.algorithms.deep_cfr.deep_cfr import DeepCFR
    from scopa_amd.envs.openspiel_mini_scopa import MiniScopaGame
    rng = np.random.RandomState(3)
    seen_plies = set()
    for seed in range(50):
        host = MiniScopaGame(seed=seed).new_initial_state()
        st = R.root_state(oracle.deal_py_seed(seed))
        assert np.array_equal(R.pack(st), np.frombuffer(bytes(host.env.game.packed), R.STATE_DTYPE)[0])
        for ply in range(9):
            f, m = R.features(st)
            assert f.dtype == np.float32 and m.dtype == np.float32 and f.shape == (34,) and m.shape == (16,)
            player = ply & 1
            hf = DeepCFR._state_to_features(None, host, player)
            hm = DeepCFR._get_legal_actions_mask(None, host, player)
            if ply < 8:
                assert not host.is_terminal() and host.current_player() == player
                assert np.array_equal(f.view(np.uint32), hf.view(np.uint32)) and np.array_equal(m.view(np.uint32), hm.view(np.uint32)), (seed, ply)
                assert f[:16].sum() == 4 - ply // 2 and f[32] == 1.0 and f[33] == 0.0 and np.array_equal(f[:16], m)
                a = host.legal_actions()[rng.randint(len(host.legal_actions()))]
                host.apply_action(a)
                st.step(a)
            else:
                assert host.is_terminal() and st.is_terminal()
                assert not f[:16].any() and not m.any() and not hm.any() and np.array_equal(f[:16], hf[:16]) and f[32] == 1.0 and f[33] == 0.0
                assert sorted(np.flatnonzero(f[16:32])) == sorted(c.id for c in host.env.game.table)
            seen_plies.add(ply)
    assert seen_plies == set(range(9))


def test_match_numbers_on_a_hand_made_batch():
    fin = np.zeros(5, R.STATE_DTYPE)
    fin["ncap"] = [[10, 6], [4, 12], [0, 0], [16, 0], [8, 8]]
    fin["scopas"] = [[1, 0], [0, 2], [0, 0], [3, 0], [0, 1]]
    seat = np.array([0, 0, 0, 1, 1])
    # r = captures + 2 scopas: (12, 6) (4, 16) (0, 0) (22, 0) (8, 10); reward of the trained seat: 3, -6, 0 | -11, 1
    avg, (own, opp), halves = R.match_numbers(fin, seat)
    assert avg == (3 - 6 + 0 - 11 + 1) / 5 and own == (1 + 0 + 0 + 0 + 1) / 5 and opp == (0 + 2 + 0 + 3 + 0) / 5
    assert halves[0]["episodes"] == 3 and halves[0]["reward"] == -1.0 and halves[0]["trained_scopas"] == 1 / 3 and halves[0]["opponent_scopas"] == 2 / 3
    assert halves[1]["episodes"] == 2 and halves[1]["reward"] == -5.0 and halves[1]["trained_scopas"] == 0.5 and halves[1]["opponent_scopas"] == 1.5
    assert halves[1]["reward_std_error"] == 6.0 / np.sqrt(2) and abs(halves[0]["reward_std_error"] - np.sqrt(14.0) / np.sqrt(3)) < 1e-15
