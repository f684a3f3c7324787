"""CPU checks of tests/full_chance_net_match_ref.py, the restatement the GPU suite of the nets' match (test_gpu_full_chance_net_match.py) is held to, and
of what the feature adds on the host: names in header, binding and library, the refusals that come before the device is touched.

The level-by-level match is held to full_chance_ref.match with the agent's rows planted as a store, to a per-episode depth-first replay that asks the
policy one node at a time (uniform, store and net opponents), and to the Philox separation guard of DESIGN section 2: a seed cut to 32 bits or a
stream id cut to 16 bits must change what the restatement expects."""
import os
import re

import numpy as np
import pytest

import full_chance_net_match_ref as M
import full_chance_ref as W
import full_chance_sdcfr_ref as S
import full_mccfr_ref as F

from conftest import ROOT

SEED = 0x5C09A
WIDE_SEED = 0x9E3779B97F4A7C15
NEW = ("scopa_full_chance_sdcfr_average_at", "scopa_full_chance_sdcfr_match", "scopa_full_chance_debug_sdcfr_average_grid")


def game_of(oracle, R, n):
    from scopa_amd.algorithms import packet_decks
    r0 = 6 - R
    deck = oracle.full_deal_py_seed(42)
    st, _ = F.random_root(deck, r0, np.random.RandomState(100 * r0 + 42))
    return st, packet_decks(deck, r0, n, 5, fix_seat=0)


def planted(root, decks):
    """a strategy row per pair of the sub-game (full_chance_ref.rows_for), as a store dict and as an agent_fn that looks the rows up"""
    keys = W.subgame_keys(root, decks)
    rows = W.rows_for(keys)[1]
    store = {(int(a), int(b)): [float(x) for x in r] for (a, b), r in zip(keys.tolist(), rows)}
    return store, lambda keys2, player: np.array([store[(int(a), int(b))] for a, b in np.asarray(keys2, np.uint64).reshape(-1, 2).tolist()])


@pytest.mark.parametrize("R,n_decks,n", [(1, 3, 1), (1, 3, 2), (1, 3, 33), (2, 2, 21)])
def test_levels_equal_the_store_match(oracle, R, n_decks, n):
    root, decks = game_of(oracle, R, n_decks)
    store, fn = planted(root, decks)
    sums, r2, trace = M.match_levels(root, decks, n, SEED, fn, stream_id=5)
    want_sums, want_r2 = W.match(root, decks, store, n, SEED, stream_id=5)
    assert np.array_equal(sums, want_sums) and np.array_equal(r2, want_r2)
    level0 = 4 * (6 - R)
    assert (trace[:, :level0] == -1).all() and (trace[:, level0:] >= 0).all() and (trace[:, level0:] < 3).all()
    # an agent whose rows are all zero plays uniformly: the match on an empty store
    zero = lambda keys2, player: np.zeros((len(keys2), 3))
    got = M.match_levels(root, decks, n, SEED, zero, stream_id=5)
    empty = W.match(root, decks, {}, n, SEED, stream_id=5)
    assert np.array_equal(got[0], empty[0]) and np.array_equal(got[1], empty[1])
    # the uniform rows average_at writes without snapshots give the same episodes
    uni = lambda keys2, player: (np.arange(3)[None, :] < M.held(keys2)[:, None]) / M.held(keys2)[:, None].astype(np.float64)
    got = M.match_levels(root, decks, n, SEED, uni, stream_id=5)
    assert np.array_equal(got[0], empty[0]) and np.array_equal(got[1], empty[1])


@pytest.mark.parametrize("kind", ["uniform", "store", "nets"])
def test_levels_equal_depth_first_episodes(oracle, kind):
    root, decks = game_of(oracle, 2, 3)
    agent = M.host_rows_fn([([S.exact_net(7)], [1.0]), ([S.exact_net(8)], [1.0])], exact=True)
    opponent = {"uniform": None, "store": ("store", planted(root, decks)[0]),
                "nets": ("nets", M.host_rows_fn([([S.xavier_net(3), S.xavier_net(4)], [0.25, 0.75]), ([S.xavier_net(5)], [1.0])]))}[kind]
    n = 14
    sums, r2, trace = M.match_levels(root, decks, n, SEED, agent, opponent, stream_id=2)
    want = np.zeros(6, np.int64)
    for i in range(n):
        seat = 0 if 2 * i < n else 1
        e_r2, mine, theirs, e_trace = M.episode(root, decks, i, n, SEED, agent, opponent, stream_id=2)
        assert e_r2 == r2[i] and np.array_equal(e_trace, trace[i]), (kind, i)
        want += [e_r2 * (seat == 0), e_r2 * (seat == 1), e_r2 * e_r2 * (seat == 0), e_r2 * e_r2 * (seat == 1), mine, theirs]
    assert np.array_equal(sums, want)
    # the trace replays to the same rewards, every slot legal
    got = M.replay(root, decks, n, trace)
    assert np.array_equal(got[0], sums) and np.array_equal(got[1], r2) and all(len(m) == 8 for m in got[2])
    assert len(set(trace[:, 16:].reshape(-1).tolist())) > 1                # the draws are not all one slot


def test_exact_rows_equal_the_float64_average(oracle):
    root, decks = game_of(oracle, 1, 3)
    keys = W.subgame_keys(root, decks)
    for player in (0, 1):
        mine = keys[((keys[:, 0] >> np.uint64(62)) & np.uint64(1)) == player]
        snaps, coefs = [S.exact_net(7 + player), S.exact_net(17 + player)], [0.25, 0.75]
        exact = M.average_rows(snaps, coefs, mine, exact=True)
        ref, tol, amb = S.average_policy(snaps, coefs, mine, M.held(mine))
        assert (np.abs(exact - ref)[~amb] <= tol[~amb] + 1e-15).all()
        assert np.allclose(exact.sum(1), 1.0, atol=1e-12)
    none = M.average_rows([], [], keys)
    assert np.array_equal(none, (np.arange(3)[None, :] < M.held(keys)[:, None]) / M.held(keys)[:, None].astype(np.float64))


def test_every_philox_word_reaches_the_draw(oracle):
    """DESIGN section 2's separation guard: a seed with a non-zero high word and a stream id above 16 bits; cutting either changes the expectation, so
    a kernel that drops the bits cannot pass the GPU comparison"""
    root, decks = game_of(oracle, 2, 3)
    store, fn = planted(root, decks)
    stream = (1 << 24) - 1
    n = 40
    full = M.match_levels(root, decks, n, WIDE_SEED, fn, stream_id=stream)
    cut_seed = M.match_levels(root, decks, n, WIDE_SEED, fn, stream_id=stream, seed_bits=32)
    cut_stream = M.match_levels(root, decks, n, WIDE_SEED, fn, stream_id=stream, stream_bits=16)
    assert not np.array_equal(full[2], cut_seed[2]) and not np.array_equal(full[2], cut_stream[2])
    assert not np.array_equal(full[1], cut_seed[1]) and not np.array_equal(full[1], cut_stream[1])
    want = W.match(root, decks, store, n, WIDE_SEED, stream_id=stream)
    assert np.array_equal(full[0], want[0]) and np.array_equal(full[1], want[1])


def test_new_names_and_host_refusals(sl):
    hdr = open(os.path.join(ROOT, "include", "scopa.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = sl.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in sl.SYMBOLS and hasattr(L, name) and getattr(L, name).argtypes is not None
    assert L.scopa_full_chance_sdcfr_match.argtypes[2] is sl.C.c_uint32           # stream_id at full width
    assert hasattr(sl.FullChanceMCCFR, "sdcfr_match") and hasattr(sl.Context, "full_chance_sdcfr_average_at")
    assert sl.C.sizeof(sl.FullSdcfrSnapshots) == 8 + 8 * sl.C.sizeof(sl.C.c_void_p)
    # refusals that need no GPU: they come before the device is touched
    sums = np.full(6, 77, np.int64)
    assert L.scopa_full_chance_sdcfr_match(None, 4, 0, None, 0, None, None, None, sl._ptr(sums), None, None) == sl.SCOPA_EINVAL
    assert (sums == 77).all()
    assert L.scopa_full_chance_sdcfr_average_at(None, 0, None, 0, 0, *([None] * 7), 0, None, None) == sl.SCOPA_EINVAL
    assert L.scopa_full_chance_debug_sdcfr_average_grid(None, 0) == sl.SCOPA_EINVAL and hasattr(sl.Context, "full_chance_debug_sdcfr_average_grid")
    import inspect
    from scopa_amd.algorithms.deep_cfr import FullChanceDeepCFR
    sig = inspect.signature(FullChanceDeepCFR.match).parameters
    assert [sig[k].default for k in ("opponent", "decks", "root_actions", "stream_id", "per_episode")] == [None, None, None, 0, False]
    assert list(inspect.signature(FullChanceDeepCFR.average_policy_at).parameters) == ["self", "keys2", "player"]
    from scopa_amd.algorithms.full_chance import match_report
    rep = match_report(np.array([4, -2, 8, 2, 3, 1], np.int64), 4)
    assert rep["reward"] == 0.25 and rep["by_seat"][0]["reward"] == 1.0 and rep["by_seat"][1]["reward"] == -0.5 and rep["exact_reward"] is None
