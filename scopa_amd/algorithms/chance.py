"""MiniScopa over a set of deals with the deal as a chance move (scopa_chance_* in include/scopa.h, _lib.ChanceGame).

A policy solved on one deal assumes the opponent's hand is known: that tree has no chance node.  Here chance picks one of a MultiDeal's deals
uniformly and infosets are shared across deals by key -- P{player}:H[own hand]_T[table], what a player who cannot see the other hand knows -- so
the solved policy is a table over KEYS and carries over to deals it never saw (table_for).  The iterations, the reduction across deals and the
exploitability run in the library's kernels; this module is the host loop, the deal sets and the key dictionaries.  Policies over keys are played
against each other by cross_play (exact, averaged over the deals), best_response (the best responses across deals as tables) and evaluate (the
sampled seat-swapped match that draws the deal per episode, next to its exact expectation).
"""
from itertools import combinations

import numpy as np

from .cfr_variants import schedule


def sample_deals(n, m, start, count, seed=0):
    """The deal samples of iterations start .. start + count - 1: int32 [count][m], row i holding m distinct deals of n, ascending, drawn with
    np.random.Generator(np.random.Philox(key=[seed, start + i])).choice(n, m, replace=False).  Keyed by the absolute iteration, so a continued
    run draws what one long run draws."""
    n, m, start, count = int(n), int(m), int(start), int(count)
    if not 1 <= m <= n or start < 0 or count < 0:
        raise ValueError("sample_deals: need 1 <= m <= n, start >= 0 and count >= 0")
    out = np.zeros((count, m), np.int32)
    for i in range(count):
        out[i] = np.sort(np.random.Generator(np.random.Philox(key=[int(seed), start + i])).choice(n, m, replace=False))
    return out


def solve(multi, variant="cfr+", eps=1e-3, max_iters=1000, check_every=10, alternating=False, sample=None, seed=0, **params):
    """Run `variant` ("vanilla", "cfr+", "linear", "dcfr"; params: alpha, beta, gamma) on the chance game over a built MultiDeal's deals from
    iteration 1 until its exploitability is below eps or max_iters is reached: chunks of check_every weighted iterations with the schedule
    continued, exploitability() after each.  sample=m: every iteration sweeps only m of the n deals, sample_deals(n, m, t, k, seed), through
    cfr_iterate_sampled; the exploitability stays the exact one over all deals.  -> (ChanceGame, iterations run, [(iteration, exploitability), ...])."""
    from .._lib import ChanceGame
    game, t, curve = ChanceGame(multi), 0, []
    while t < max_iters:
        k = min(int(check_every), int(max_iters) - t)
        if sample is None:
            game.cfr_iterate_weighted(schedule(variant, t, k, **params), alternating)
        else:
            game.cfr_iterate_sampled(sample_deals(game.n, sample, t, k, seed), schedule(variant, t, k, **params), alternating)
        t += k
        curve.append((t, float(game.exploitability()[0])))
        if curve[-1][1] < eps:
            break
    return game, t, curve


def solve_mccfr(multi, batch, eps=1e-3, max_iters=1000, check_every=10, sample=None, seed=0):
    """Run chance-sampled external-sampling MCCFR (ChanceGame.mccfr_iterate: `batch` traversal pairs per listed deal and iteration, Philox seed
    `seed`) on the chance game over a built MultiDeal's deals until its exploitability is below eps or max_iters is reached: chunks of check_every
    iterations, the exact exploitability() over all deals after each.  sample=m: every iteration walks only m of the n deals,
    sample_deals(n, m, t, k, seed).  -> (ChanceGame, iterations run, [(iteration, exploitability), ...])."""
    from .._lib import ChanceGame
    game, t, curve = ChanceGame(multi), 0, []
    while t < max_iters:
        k = min(int(check_every), int(max_iters) - t)
        game.mccfr_iterate(batch, k, seed, None if sample is None else sample_deals(game.n, sample, t, k, seed))
        t += k
        curve.append((t, float(game.exploitability()[0])))
        if curve[-1][1] < eps:
            break
    return game, t, curve


def hidden_hand_deals(hand0):
    """The 495 deals in which seat 0 holds `hand0` (4 cards, in this order) and seat 1 any 4 of the other 12 cards: uint8 [495][16] perms =
    seat-0 hand + seat-1 hand (ascending, the combinations in lexicographic order) + the remaining 8 cards ascending."""
    hand0 = [int(c) for c in hand0]
    if len(hand0) != 4 or len(set(hand0)) != 4 or not all(0 <= c < 16 for c in hand0):
        raise ValueError("hand0 must be 4 distinct cards in 0..15")
    rest = [c for c in range(16) if c not in hand0]
    perms = [hand0 + list(h1) + [c for c in rest if c not in h1] for h1 in combinations(rest, 4)]
    return np.array(perms, np.uint8)


def policy_by_key(game, policy=None):
    """{key: float64 [4] row} of `policy` ([G][4]; None = the game's average policy)"""
    keys, _ = game.index()
    if policy is None:
        _, policy = game.exploitability(return_policy=True)
    return {int(k): np.array(row, np.float64) for k, row in zip(keys, policy)}


def table_for(ctx, by_key):
    """A policy table [n_infosets][4] for the deal `ctx` holds -- any deal, held out or not: the row of every key in `by_key`, uniform over the
    legal actions (bits 1-3 of the key) for a key it does not have.  Host glue over the tree's exported keys."""
    keys = ctx.tree_export()["infoset_key"]
    P = np.zeros((len(keys), 4))
    for r, k in enumerate(keys):
        row = by_key.get(int(k))
        if row is None:
            n = (int(k) >> 1) & 7
            P[r, :n] = 1.0 / n
        else:
            P[r] = row
    return P


# ---- policy against policy across the deals (scopa_chance_cross_play, scopa_chance_best_response, scopa_chance_match) ------------------------
def _nlegal(game):
    cached = getattr(game, "_nlegal_of_keys", None)
    if cached is None:
        cached = game._nlegal_of_keys = ((game.index()[0] >> np.uint64(1)) & np.uint64(7)).astype(np.int64)
    return cached


def uniform_table(game):
    """[G][4]: 1 / legal count over every key's legal slots, zeros beyond"""
    n = _nlegal(game)
    return np.where(np.arange(4)[None, :] < n[:, None], 1.0 / n[:, None].astype(np.float64), 0.0)


def check_policy_table(game, table):
    """evaluation.check_policy_table against the game's keys: raise ValueError unless `table` ([G][4], or a stack [K][G][4]; numpy or torch) has rows
    whose legal slots (the first nlegal of the key, hand order) sum to 1 within 1e-9 and whose illegal slots are exactly 0"""
    from .evaluation import _host_table
    t = _host_table(table)
    if t.ndim not in (2, 3) or t.shape[-2:] != (game.G, 4):
        raise ValueError(f"policy table: expected [{game.G}][4] (or a stack of them), got {list(t.shape)}")
    legal = np.arange(4)[None, :] < _nlegal(game)[:, None]
    stack = t.reshape(-1, game.G, 4)
    if (np.where(legal, 0.0, stack) != 0.0).any():
        k, r, c = (int(x[0]) for x in np.nonzero(np.where(legal, 0.0, stack) != 0.0))
        raise ValueError(f"policy table {k}: key row {r} has mass {stack[k, r, c]!r} on the illegal slot {c}")
    off = ~(np.abs(np.where(legal, stack, 0.0).sum(2) - 1.0) <= 1e-9)                     # a NaN row fails too
    if off.any():
        k, r = (int(x[0]) for x in np.nonzero(off))
        raise ValueError(f"policy table {k}: the legal slots of key row {r} sum to {np.where(legal, stack, 0.0)[k, r].sum()!r}, not 1")


def _device_stack(game, policies):
    """evaluation._device_stack for [G][4] tables: -> contiguous float64 [K][G][4] tensor on the game's device, checked"""
    import torch
    dev = f"cuda:{game.ctx.device}"
    if hasattr(policies, "detach"):
        stack = policies.detach().to(device=dev, dtype=torch.float64)
    elif isinstance(policies, (list, tuple)) and any(hasattr(p, "detach") for p in policies):
        stack = torch.stack([torch.as_tensor(p if hasattr(p, "detach") else np.array(p, dtype=np.float64), dtype=torch.float64, device=dev) for p in policies])
    else:
        stack = torch.as_tensor(np.array(policies, dtype=np.float64, order="C"), device=dev)     # a copy: the caller's arrays may be read-only
    if stack.dim() == 2:
        stack = stack.unsqueeze(0)
    check_policy_table(game, stack)
    return stack.contiguous()


def cross_play(game, policies):
    """Exact cross-play of K policies over keys on the chance game: -> {"reward": [K][K], "reward_std": [K][K], "scopas": [K][K][2], "per_deal":
    [n][K][K][4]} (numpy), evaluation.cross_play's entries averaged over the deals -- entry [a][b] is policy a in seat 0 against policy b in seat 1,
    reward_std the standard deviation of seat 0's reward over the deal and the play of both -- and per deal the four raw quantities (reward, its
    square, scopas of seat 0, scopas of seat 1)."""
    import torch
    stack = _device_stack(game, policies)
    k = stack.shape[0]
    out = torch.empty((k, k, 4), dtype=torch.float64, device=stack.device)
    per_deal = torch.empty((game.n, k, k, 4), dtype=torch.float64, device=stack.device)
    torch.cuda.synchronize()
    game.cross_play(k, stack.data_ptr(), out.data_ptr(), per_deal.data_ptr())
    game.ctx.synchronize()
    o = out.cpu().numpy()
    with np.errstate(invalid="ignore"):
        std = np.sqrt(np.maximum(o[..., 1] - o[..., 0] * o[..., 0], 0.0))
    return {"reward": o[..., 0].copy(), "reward_std": std, "scopas": o[..., 2:].copy(), "per_deal": per_deal.cpu().numpy()}


def best_response(game, policy):
    """-> {"exploitability", "br_values": (BR0, BR1), "value", "tables": (br0, br1)}: the numbers game.exploitability(policy) gives, bit for bit, and
    the best responses across deals themselves -- br_p is `policy` with player p's rows one-hot at the best action, a [G][4] table cross_play or
    evaluate takes as it is."""
    import torch
    stack = _device_stack(game, policy)
    if stack.shape[0] != 1:
        raise ValueError("best_response takes one policy table")
    br = torch.empty((2, game.G, 4), dtype=torch.float64, device=stack.device)
    out4 = torch.empty(4, dtype=torch.float64, device=stack.device)
    torch.cuda.synchronize()
    game.best_response(1, stack.data_ptr(), br.data_ptr(), out4.data_ptr())
    game.ctx.synchronize()
    o, tables = out4.cpu().numpy(), br.cpu().numpy()
    return {"exploitability": float(o[0]), "br_values": (float(o[1]), float(o[2])), "value": float(o[3]), "tables": (tables[0], tables[1])}


def evaluate(game, policy, num_episodes=10000, opponent=None, stream_id=16):
    """-> (avg_reward, scopa_stats) of `policy` ([G][4]) in a seat-swapped sampled match that draws the deal per episode (scopa_chance_match, one
    launch), evaluate_agent_device(..., opponent=table)'s shape: the first (n + 1) // 2 episodes have the policy in seat 0.  opponent: a [G][4]
    table, or None = the uniform table built from the keys (the reference's evaluate_vs_random opponent).  scopa_stats carries "exact_reward" -- the
    match's expected reward from cross_play, seat halves weighted as played -- and "exact_by_seat"."""
    import torch
    from .evaluation import _halves_from_sums, _match_stats
    n = int(num_episodes)
    if n == 0:
        return 0.0, {"trained_avg": 0.0, "opponent_avg": 0.0, "difference": 0.0, "data_collected": False, "reward_std_error": 0.0,
                     "by_seat": _halves_from_sums(np.zeros((2, 5), np.int64))}
    first = (n + 1) // 2
    dev = f"cuda:{game.ctx.device}"
    pol = torch.as_tensor(np.array(policy.detach().cpu().numpy() if hasattr(policy, "detach") else policy, dtype=np.float64, order="C"), device=dev)   # a copy
    pair = _device_stack(game, [pol, uniform_table(game) if opponent is None else opponent])
    if pair.shape[0] != 2:
        raise ValueError("evaluate: policy and opponent must be one [G][4] table each")
    exact = cross_play(game, pair)["reward"]
    torch.cuda.synchronize()
    st = game.match(pair[0].data_ptr(), pair[1].data_ptr(), n, first, stream_id)
    avg, stats = _match_stats(st)
    by_seat = (float(exact[0, 1]), float(-exact[1, 0]))                  # the policy in seat 0; in seat 1 (the reward is seat 0's: negate)
    stats["exact_by_seat"] = by_seat
    stats["exact_reward"] = (first * by_seat[0] + (n - first) * by_seat[1]) / n
    return avg, stats
