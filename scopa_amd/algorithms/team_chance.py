"""Team MiniScopa over a set of deals with the deal as a chance move (scopa_team_chance_* in include/scopa.h, _lib.TeamChanceGame).

On one deal the information-state string ends in the whole action history: every node is its own infoset and the team game is one of perfect
information.  Here chance picks one of n deals uniformly and a team's rows are shared, by key, between all deals the acting seat cannot tell apart
-- it sees neither its partner's hand nor its opponents'.  The iterations, the reduction across deals and the best response across deals run in the
library's kernels; this module is the host loop, the deal sets and the key dictionaries.  solve(sample=m) sweeps m of the n deals per iteration
(TeamChanceGame.cfr_iterate_sampled, lists from chance.sample_deals) and solve(alternating=False) updates both teams against one sigma.

Key of a choice node (depths 0..11), 64 bits: bits 60-63 the depth, bits 44-59 the acting seat's initial hand in hand order (nibble i = position i),
bits 0-43 the card ids played so far (nibble i = ply i).  It refines the reference's information_state_string (sorted hand) by the hand's order.
"""
from itertools import permutations

import numpy as np

from .cfr_variants import schedule


def solve(perms, variant="cfr+", eps=1e-3, max_iters=1000, check_every=10, device=0, alternating=True, sample=None, seed=0, **params):
    """Run `variant` ("vanilla", "cfr+", "linear", "dcfr"; params: alpha, beta, gamma) on the team chance game over the deals `perms` ([n][16])
    from iteration 1 until its exploitability is below eps or max_iters is reached: chunks of check_every weighted iterations with the schedule
    continued, exploitability() after each.  sample=m: every iteration sweeps only m of the n deals, chance.sample_deals(n, m, t, k, seed), through
    cfr_iterate_sampled; the exploitability stays the exact one over ALL deals.  alternating=False: both teams are updated against the sigma of the
    iteration's start.  The defaults run cfr_iterate.  -> (TeamChanceGame, iterations run, [(iteration, exploitability), ...])."""
    from .._lib import TeamChanceGame
    from .chance import sample_deals
    if sample is not None and int(sample) < 1:
        raise ValueError("solve: sample must be at least 1")
    game, t, curve = TeamChanceGame(perms, device), 0, []
    if sample is not None and int(sample) > game.n:
        game.close()
        raise ValueError("solve: sample must not exceed the number of deals")
    while t < max_iters:
        k = min(int(check_every), int(max_iters) - t)
        w = schedule(variant, t, k, **params)
        if sample is None and alternating:
            game.cfr_iterate(w)
        else:
            game.cfr_iterate_sampled(None if sample is None else sample_deals(game.n, sample, t, k, seed), w, alternating)
        t += k
        curve.append((t, float(game.exploitability()[0])))
        if curve[-1][1] < eps:
            break
    return game, t, curve


def solve_mccfr(perms, batch, eps=1e-3, max_iters=1000, check_every=10, sample=None, seed=0x5C09A, device=0):
    """Run deal-sampled external-sampling MCCFR (TeamChanceGame.mccfr_iterate: `batch` traversal pairs per listed deal and iteration, Philox seed
    `seed` set on the game's context) on the team chance game over the deals `perms` ([n][16]) until its exploitability is below eps or max_iters is
    reached: chunks of check_every iterations, the exact exploitability() over ALL deals after each.  sample=m: every iteration walks only m of the
    n deals, chance.sample_deals(n, m, t, k, seed).  -> (TeamChanceGame, iterations run, [(iteration, exploitability), ...])."""
    from .._lib import TeamChanceGame
    from .chance import sample_deals
    game, t, curve = TeamChanceGame(perms, device), 0, []
    game.ctx.mccfr_seed(seed)
    while t < max_iters:
        k = min(int(check_every), int(max_iters) - t)
        game.mccfr_iterate(batch, k, None if sample is None else sample_deals(game.n, sample, t, k, seed))
        t += k
        curve.append((t, float(game.exploitability()[0])))
        if curve[-1][1] < eps:
            break
    return game, t, curve


def packet_deals(packets, fix_seat0=False):
    """The deals that hand four disjoint 4-card packets (each ascending) to the four seats: uint8 [24][16], deal k giving seat s the packet
    packets[a[s]] for the k-th arrangement a of itertools.permutations(range(4)) (lexicographic); fix_seat0: the 6 of them with a[0] = 0, in the
    same order (so deals 0 and 1 differ by swapping seats 2 and 3).  The closed game in which every seat knows its packet and not the
    arrangement of the others; hands are ascending, so equal hand sets share rows."""
    packets = [[int(c) for c in p] for p in packets]
    cards = [c for p in packets for c in p]
    if len(packets) != 4 or any(len(p) != 4 or p != sorted(p) for p in packets) or sorted(cards) != list(range(16)):
        raise ValueError("packet_deals: four disjoint ascending 4-card packets covering 0..15 are required")
    arrangements = [a for a in permutations(range(4)) if not fix_seat0 or a[0] == 0]
    return np.array([[c for s in range(4) for c in packets[a[s]]] for a in arrangements], np.uint8)


def make_key(depth, hand, history):
    """the 64-bit key from the depth, the acting seat's initial hand (4 cards, hand order) and the cards played so far"""
    key = (int(depth) << 60)
    for i, c in enumerate(hand):
        key |= int(c) << (44 + 4 * i)
    for i, c in enumerate(history):
        key |= int(c) << (4 * i)
    return key


def key_of(team_state):
    """the key of a live _lib.TeamState at a choice node (depths 0..11)"""
    d = int(team_state.s[0]["step"])
    if team_state.is_terminal() or d >= 12:
        raise ValueError("key_of: not a choice node (forced plies 12..15 have no row)")
    seat = d & 3
    return make_key(d, team_state.perm[4 * seat:4 * seat + 4], team_state.history())


def policy_by_key(game, policy=None):
    """{key: float64 [4] row} of `policy` ([G][4]; None = the game's average policy)"""
    keys, _ = game.index()
    if policy is None:
        _, policy = game.exploitability(return_policy=True)
    return {int(k): np.array(row, np.float64) for k, row in zip(keys, policy)}


# ---- policy against policy (scopa_team_chance_cross_play / scopa_team_chance_match; team_cfr.TeamCFRTrainer has the one-deal pair) ------------------
def device_stack(device, rows, policies):
    """policies (a [K][rows][4] array or tensor, one [rows][4] table, or a sequence of tables) -> contiguous float64 [K][rows][4] tensor on `device`"""
    import torch
    dev = f"cuda:{device}"
    if hasattr(policies, "detach"):
        stack = policies.detach().to(device=dev, dtype=torch.float64)
    elif isinstance(policies, (list, tuple)) and any(hasattr(p, "detach") for p in policies):
        stack = torch.stack([torch.as_tensor(p if hasattr(p, "detach") else np.array(p, dtype=np.float64), dtype=torch.float64, device=dev) for p in policies])
    else:
        stack = torch.as_tensor(np.array(policies, dtype=np.float64, order="C"), device=dev)     # a copy: the caller's arrays may be read-only
    if stack.dim() == 2:
        stack = stack.unsqueeze(0)
    if stack.dim() != 3 or tuple(stack.shape[1:]) != (int(rows), 4):
        raise ValueError(f"policy tables must be [{int(rows)}][4], got {tuple(stack.shape)}")
    return stack.contiguous()


def cross_play(game, policies):
    """Exact cross-play of K policies over keys on the team chance game: -> float64 [K][K][4] (numpy), entry [a][b] = (E[reward of team 0], E[its
    square], E[scopas of team 0], E[scopas of team 1]) with policy a as team 0 against policy b as team 1, averaged over the deals in deal order.
    Rows are used as given.  One call, three launches."""
    import torch
    stack = device_stack(game.ctx.device, game.G, policies)
    k = stack.shape[0]
    out = torch.empty((k, k, 4), dtype=torch.float64, device=stack.device)
    torch.cuda.synchronize()
    game.cross_play(k, stack.data_ptr(), out.data_ptr())
    game.ctx.synchronize()
    return out.cpu().numpy()


def match_report(st, exact):
    """what evaluate returns, from a match's integer sums st [2][5] (a's side) and the exact cross-play [2][2][4] of (a, b)"""
    halves, n = [], int(st[:, 0].sum())
    for half, (cell, sign) in enumerate((((0, 1), 1.0), ((1, 0), -1.0))):           # a as team 0; a as team 1 (the exact reward is team 0's: negate)
        m = int(st[half, 0])
        e, e2 = float(exact[cell][0]), float(exact[cell][1])
        halves.append({"episodes": m, "reward": 0.5 * int(st[half, 1]) / m if m else 0.0, "a_scopas": int(st[half, 3]) / m if m else 0.0,
                       "b_scopas": int(st[half, 4]) / m if m else 0.0, "exact_reward": sign * e,
                       "exact_std_error": float(np.sqrt(max(e2 - e * e, 0.0) / m)) if m else 0.0})
    var = sum(h["episodes"] * (h["exact_std_error"] ** 2 * h["episodes"]) for h in halves)       # sum of the episodes' exact variances
    return {"episodes": n, "reward": 0.5 * int(st[:, 1].sum()) / n if n else 0.0, "by_team": halves,
            "exact_by_team": (halves[0]["exact_reward"], halves[1]["exact_reward"]),
            "exact_reward": sum(h["episodes"] * h["exact_reward"] for h in halves) / n if n else 0.0,
            "exact_std_error": float(np.sqrt(var)) / n if n else 0.0, "sums": np.array(st)}


def evaluate(game, a, b, episodes=10000, seed=None, stream_id=16):
    """A sampled seat-swapped match of policy a against policy b ([G][4] each) on the team chance game, the deal drawn per episode
    (scopa_team_chance_match, one launch): the first (episodes + 1) // 2 episodes have a as team 0.  seed (or None = as it is) sets the Philox key on the
    game's context.  -> {"episodes", "reward": a's mean reward, "by_team": per half {episodes, reward, a_scopas, b_scopas, exact_reward,
    exact_std_error}, "exact_by_team", "exact_reward": a's exact reward from cross_play with the halves weighted as played, "exact_std_error": the
    standard error of "reward" from the exact second moments, "sums": the raw int64 [2][5]}.  The exact figures are those of the tables as given;
    they are the match's law where the rows are normalised."""
    import torch
    n = int(episodes)
    pair = device_stack(game.ctx.device, game.G, [a, b])
    if pair.shape[0] != 2:
        raise ValueError("evaluate: a and b must be one [G][4] table each")
    if seed is not None:
        game.ctx.mccfr_seed(seed)
    exact = cross_play(game, pair)
    torch.cuda.synchronize()
    st = game.match(pair[0].data_ptr(), pair[1].data_ptr(), n, (n + 1) // 2, stream_id)
    return match_report(st, exact)
