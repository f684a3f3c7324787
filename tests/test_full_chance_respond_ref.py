"""CPU checks that hold the restatement of the sampled best response (tests/full_chance_respond_ref.py) to things not written for it: exact
enumeration of the counterfactual regret under a planted opponent, full_chance_ref.traverse on bits where the two walks must coincide, the Philox
separation of the new tag, and -- for tests/test_gpu_full_chance_respond.py -- the exact sweeps' best response at one round to go, which is where
that file's N and B come from."""
import os
import re

import numpy as np
import pytest

import full_chance_exploit_ref as E
import full_chance_ref as X
import full_chance_respond_ref as Q
import full_chance_xplay_ref as XP
import full_mccfr_ref as F
import test_gpu_full_chance as G                   # (fixture builders are plain CPU code; only the module's tests carry the gpu mark)
import test_gpu_full_chance_respond as GR

SEED = G.SEED
CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "scopa_amd", "csrc")


def edge_opponent(keys):
    """an opponent over `keys` whose rows cycle through the edges: strategy rows summing to zero (played uniformly), one-hot, mixed dyadic and
    X.rows_for's; regret rows with negatives only (uniform), one positive, (2, 1, 1) / (3, 1) and X.rows_for's"""
    keys = np.asarray(keys, np.uint64).reshape(-1, 2)
    R, S = X.rows_for(keys)
    for i, k in enumerate(keys.tolist()):
        n, kind = X.key_actions(k), i % 4
        hot = [1.0 if a == (i // 4) % n else 0.0 for a in range(3)]
        mixed = [2.0, 1.0, 1.0] if n == 3 else [3.0, 1.0, 0.0]
        if kind == 0:
            S[i], R[i] = 0.0, [-1.0, -2.0, -0.5 if n == 3 else 0.0]
        elif kind == 1:
            S[i], R[i] = [4.0 * x for x in hot], [2.0 * x for x in hot]
        elif kind == 2:
            S[i], R[i] = [2.0 * x for x in mixed], mixed
    return GR.planted_rows(keys, R, S)


# ---- 1. the walk is external sampling against the fixed opponent ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("resp", [0, 1])
def test_walk_is_unbiased_under_a_planted_opponent(oracle, resp, which):
    """R = 1 on 3 decks: sample t is the sum over the decks of traversal id t's d_regret rows from zero tables (the responder plays uniformly); its mean
    over 4 096 ids is held, cell by cell, to the depth-first exact counterfactual regret under the opponent's probabilities, within 5 standard errors"""
    st, decks, keys = GR.bound_case(oracle)[:3]
    opp = edge_opponent(keys)
    exact = Q.exact_regret(st, decks, resp, opp, which)
    n = 4096
    cells = sorted(exact)
    col = {k: i for i, k in enumerate(cells)}
    inc = np.zeros((n, len(cells), 3))
    starts = [X.root_on(st, d) for d in decks]
    for t in range(n):
        rows = X.Rows()
        for d, s0 in enumerate(starts):
            Q.walk(s0, resp, t, 0, SEED, rows, d, opp, which)
        assert not any(any(v) for v in rows.dS.values()) and all(GR.player_of(k) == resp for k in rows.count)
        for k, dr in rows.dR.items():
            inc[t, col[k]] = dr                                                # (a pair outside `exact` would be a KeyError)
    mean, se = inc.mean(0), inc.std(0, ddof=1) / np.sqrt(n)
    want = np.array([exact[k] for k in cells])
    err = np.abs(mean - want)
    sure = se == 0.0
    assert (err[sure] <= 1e-12).all()
    ratio = err[~sure] / se[~sure]
    print("rows", len(cells), "largest |mean - exact| / se:", ratio.max())
    assert len(cells) >= 10 and (~sure).sum() >= 20
    assert (ratio <= 5.0).all()
    # the opponent matters: under uniform play the exact regrets are others
    uniform = Q.exact_regret(st, decks, resp)
    assert max(abs(a - b) for k in cells for a, b in zip(exact[k], uniform[k])) > 1e-3


# ---- 2. where the two walks must coincide they do, on bits --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("trav", [0, 1])
def test_response_equals_traverse_on_the_traversers_rows(oracle, trav, which):
    """Dyadic regret rows on every pair of a round-4 sub-game (one-hot, (2, 1, 1) / (3, 1), zeros), the opponent's strategy rows planted so that
    strategy / total IS regret matching of those rows, and the tag overridden to traverse's: the responder's increments equal
    full_chance_ref.traverse's on the traverser's rows bit for bit, counts and counters included"""
    decks, _, st = G.deck_set(oracle, 42, 4)
    keys = X.subgame_keys(st, decks)
    R = np.zeros((len(keys), 3))
    for i, k in enumerate(keys.tolist()):
        n = X.key_actions(k)
        if i % 3 == 0:
            R[i, (i // 3) % n] = 2.0
        elif i % 3 == 1:
            R[i] = [2.0, 1.0, 1.0] if n == 3 else [3.0, 1.0, 0.0]
    S = 4.0 * np.array([F.sigma_of(r, X.key_actions(k)) + [0.0] * (3 - X.key_actions(k)) for r, k in zip(R, keys.tolist())])
    for r, s, k in zip(R, S, keys.tolist()):
        n = X.key_actions(k)
        assert F.average_probs({0: list(s)}, 0, n) == F.sigma_of(r, n)         # the same bits by either rule
    base, mine = GR.planted_rows(keys, R, np.zeros_like(R)), GR.planted_rows(keys, R, np.zeros_like(R))
    X.traverse(st, decks, trav, 3, 5, 3, SEED, base)
    Q.traverse(st, decks, trav, 3, 5, 3, SEED, mine, GR.planted_rows(keys, R, S), which, tag=X.WALK_TAG)
    own = [k for k in base.count if GR.player_of(k) == trav]
    assert sorted(own) == sorted(mine.count) and len(own) > 20 and (base.choice, base.terminal) == (mine.choice, mine.terminal)
    for k in own:
        assert base.count[k] == mine.count[k]
        assert np.array(base.dR[k]).tobytes() == np.array(mine.dR[k]).tobytes() and not any(mine.dS[k])
    # ... and with the tag its own the draws are others
    other = GR.planted_rows(keys, R, np.zeros_like(R))
    Q.traverse(st, decks, trav, 3, 5, 3, SEED, other, GR.planted_rows(keys, R, S), which)
    assert other.arrays("count")[1].tolist() != mine.arrays("count")[1].tolist() or other.arrays("count")[0].tolist() != mine.arrays("count")[0].tolist()


# ---- 3. the tag ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_response_tag_is_free_and_separates(oracle):
    """144 + responder is no other kernel's Philox tag (every k...Tag constant of the sources, each with its + traverser, and the low tags the comment
    in scopa_team_mccfr_walk.h lists), the source and the restatement agree on it, and the GPU tests' counts change with traverse's tag in its place"""
    tags = {}
    for name in sorted(os.listdir(CSRC)):
        with open(os.path.join(CSRC, name)) as fh:
            for m in re.finditer(r"constexpr uint32_t ((?:k\w*Tag\w*\s*=\s*\d+u,?\s*)+);", fh.read()):
                for const, value in re.findall(r"(k\w*Tag\w*)\s*=\s*(\d+)u", m.group(1)):
                    tags[const] = int(value)
    assert tags["kRespondTag"] == Q.RESPOND_TAG == 144 and tags["kWalkTag"] in (160, 192) and len(tags) >= 8
    taken = set(range(0, 9)) | set(range(32, 45)) | {48}
    for const, value in tags.items():
        if const != "kRespondTag":
            taken |= {value, value + 1}
    assert not {144, 145} & taken, sorted(taken)
    decks, _, st = G.deck_set(oracle, 42, 4)
    for resp in range(2):
        right, wrong, swapped = X.Rows(), X.Rows(), X.Rows()
        Q.traverse(st, decks, resp, 0, 0, 5, SEED, right)
        Q.traverse(st, decks, resp, 0, 0, 5, SEED, wrong, tag=X.WALK_TAG)
        Q.traverse(st, decks, resp, 0, 0, 5, SEED, swapped, tag=Q.RESPOND_TAG + 1 - 2 * resp)     # the other responder's tag
        count = lambda rows: (rows.arrays("count")[0].tolist(), rows.arrays("count")[1].tolist())
        assert count(right) != count(wrong) and count(right) != count(swapped)


# ---- 4. harden ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_harden_picks_the_first_maximal_regret_of_the_legal_slots():
    three, two = (1 << 63, 0b111), (1 << 63, 0b11)
    for key, R, want in ((three, [1.0, 1.0, 0.5], 0), (three, [0.0, 0.0, 0.0], 0), (three, [-1.0, -2.0, -0.5], 2), (three, [0.25, 0.5, 0.5], 1),
                         (two, [-1.0, -2.0, 0.0], 0), (two, [-3.0, -2.0, 5.0], 1)):
        rows = X.Rows()
        rows.R[key], rows.S[key] = list(R), [3.0, 3.0, 3.0]
        Q.harden(rows)
        assert rows.S[key] == [1.0 if a == want else 0.0 for a in range(3)] and rows.R[key] == R


# ---- 5. the inputs of the GPU file's bound test -----------------------------------------------------------------------------------------------------------------------
def test_bound_case_is_what_the_gpu_test_needs(oracle):
    """BOUND of tests/test_gpu_full_chance_respond.py: after every iteration the restatement's hardened response wins, exactly, at most BR0 / BR1 of
    the exact sweeps, and after N iterations at batch B exactly those (1e-9).  No argmax turns on the order of adds: a row's best and second regret
    are more than 1e-6 apart, or they are equal and either every add into the two cells was exactly 0.0 or the two slots' exact response values
    agree (1e-12), so that a flip changes no value"""
    b = GR.BOUND
    st, decks, keys, _, R, S = GR.bound_case(oracle)
    opp = GR.planted_rows(keys, R, S)
    sol = E.solve(E.tree_of(st, decks, 1), opp.R, opp.S)
    br0, br1 = float(sol["out4"][1]), float(sol["out4"][2])
    q_of = {tuple(k): q for p in range(2) for k, q in zip(sol["rows"][p][0].tolist(), sol["rows"][p][3])}
    tree = XP.tree_of(st, decks, 1)
    rows, counter, added = X.Rows(), 0, {}
    for n in range(1, b["iterations"] + 1):
        for resp in range(2):
            Q.traverse(st, decks, resp, counter, 0, b["batch"], SEED, rows, opp, 0)
            for k, a in rows.A.items():
                added[k] = [x + y for x, y in zip(added.get(k, [0.0] * 3), a)]
            rows.apply()
            counter += 1
        hard = rows.copy()
        Q.harden(hard)
        cp = XP.cross_play(tree, [(hard.R, hard.S), (opp.R, opp.S)])
        v0, v1 = float(cp[0, 1, 0]), -float(cp[1, 0, 0])
        assert v0 <= br0 + 1e-12 and v1 <= br1 + 1e-12, n
    assert abs(v0 - br0) <= 1e-9 and abs(v1 - br1) <= 1e-9 and br0 > 1.0 and br1 < 0.0
    gap, ties = Q.regret_gap(rows)
    print("rows", len(rows.R), "smallest positive gap", gap, "tied rows", len(ties))
    assert gap > 1e-6 and len(rows.R) >= 60
    for k, a, c in ties:
        assert (added[k][a] == 0.0 and added[k][c] == 0.0) or abs(q_of[k][a] - q_of[k][c]) <= 1e-12, X.key_to_string(k)
    # fewer traversals do not get there: half the batch misses a value at N iterations
    rows, counter = X.Rows(), 0
    for n in range(b["iterations"]):
        counter = Q.iterate(st, decks, b["batch"] // 2, SEED, rows, counter, opp, 0)
    Q.harden(rows)
    cp = XP.cross_play(tree, [(rows.R, rows.S), (opp.R, opp.S)])
    assert float(cp[0, 1, 0]) < br0 - 1e-9 or -float(cp[1, 0, 0]) < br1 - 1e-9
