"""FullScopa over a SET of decks, the deal as a chance move: external-sampling MCCFR on the device where every traversal walks one deck of the set and
all decks add into rows shared by infoset (scopa_full_chance_* in include/scopa.h, scopa_amd/csrc/scopa_full_chance.hip).

FullMCCFRTrainer solves ONE deck: its key names a hand by positions in that deck, so the opponent's hand and the stock are hidden in name only and the
policy cannot be asked about a deck it has not seen.  Here a row is kept by the deck-free key pair (A, B) -- what information_state_string says -- so

    decks = packet_decks(full_deal_py_seed(42), 4, 72, seed=1, fix_seat=0)      # decks seat 0 cannot tell apart at the start of round 4
    t = FullChanceMCCFRTrainer(decks=decks[:8], root_actions=prefix_of_4_rounds, batch=64)
    t.train(100, sample=4)                                                     # 4 of the 8 decks per iteration
    t.evaluate_vs_random(1 << 16)                                              # on the training decks
    t.evaluate_vs_random(1 << 16, decks=decks[8:])                             # on held-out decks: the generalisation figure
    t.exploitability()                                                         # exact, across the training decks: dict(exploitability, br0, br1, value)
    t.exploitability(decks=decks[8:])                                          # ... and across held-out decks
    t.solve_cfr(200, variant="dcfr")                                           # exact weighted CFR on the root's sub-games (at most 4 rounds to go)
    cross_play([t, u])                                                         # exact, store against store: [2][2][4] on t's root and decks
    evaluate(t, u, 1 << 16, decks=decks[8:])                                   # t's sampled match against u, with the exact target where R <= 4
    sampled_exploitability(t, 1000, 1 << 16)                                   # a LOWER bound on t's exploitability from ANY root, the deal included

Action slots of a key are the mover's cards in ASCENDING CARD ID (hand order is deal order and differs between decks that share an infoset);
average_policy maps them back to the state's own legal-action order by card.

`exploitability`, `policy_value` and `best_response` are exact on sub-games with at most 4 rounds to go (scopa_full_chance_exploitability): the responder
plays ONE action per information state on every deck, which is where FullScopa's hidden hands are real.  The state forgets the player's own plays of
earlier rounds, so the response is THE best response with one round to go and A pure response -- its value exact, (br0 + br1) / 2 a lower bound on
the true exploitability -- with more.
"""
import math

import numpy as np

from .. import _lib
from .mc_cfr import InfoNode


def packet_decks(deck, rounds_played, n, seed, fix_seat=None):
    """n distinct decks [n][40] that share `deck`'s first 4 + 6 * rounds_played cards (the table cards and the deals of the rounds played), the rest
    permuted with np.random.RandomState(seed); row 0 is `deck` itself.  fix_seat=p: seat p's hand of round `rounds_played` (in its deal order) stays
    too -- the decks seat p cannot tell apart at the root.  ValueError where fewer than n such decks exist."""
    deck = np.ascontiguousarray(deck, np.uint8).reshape(40)
    r, n = int(rounds_played), int(n)
    if not 0 <= r <= 5 or n < 1 or fix_seat not in (None, 0, 1):
        raise ValueError("packet_decks: need 0 <= rounds_played <= 5, n >= 1 and fix_seat in (None, 0, 1)")
    first = 4 + 6 * r
    free = [i for i in range(first, 40) if fix_seat is None or not first + 3 * fix_seat <= i < first + 3 * fix_seat + 3]
    if n > math.factorial(len(free)):
        raise ValueError(f"packet_decks: only {math.factorial(len(free))} distinct decks of that packet")
    rng = np.random.RandomState(seed)
    out, seen = [deck.copy()], {deck.tobytes()}
    while len(out) < n:
        d = deck.copy()
        d[free] = deck[free][rng.permutation(len(free))]
        if d.tobytes() not in seen:
            seen.add(d.tobytes())
            out.append(d)
    return np.array(out, np.uint8)


def sample_decks(n, m, iters, seed=0, start=0):
    """The deck samples of iterations start .. start + iters - 1: int32 [iters][m], row i holding m distinct decks of n, ascending, drawn as
    chance.sample_deals draws deals (keyed by the absolute iteration, so a continued run draws what one long run draws)."""
    from .chance import sample_deals
    return sample_deals(n, m, start, iters, seed)


def _root_id(root):
    """the bytes of a root record without its hands, which the solver ignores (they are the deck's)"""
    r = np.array(root, copy=True).reshape(1)
    r["hand"], r["nh"] = 0, 0
    return r.tobytes()


def _forest_fits(root, n_decks, n_handles):
    """the limits of scopa_full_chance_cross_play for a root record"""
    R = 6 - int(np.asarray(root).reshape(1)[0]["round"])
    return R <= 4 and n_decks * 36 ** R <= 1 << 22 and n_handles * n_decks * 36 ** R <= 1 << 24


def cross_play(trainers, root_actions=None, current=False, decks=None):
    """The exact cross-play of K trainers' stores (scopa_full_chance_cross_play) -> float64 [K][K][4]: out[a][b] = (expected reward of player 0, expected
    square of it, expected scopas of player 0, of player 1) with trainers[a] as player 0 against trainers[b] as player 1, their average policies
    (current=True: their current regret-matching strategies), on the sub-games after `root_actions` played on trainers[0].decks[0] (None:
    trainers[0]'s root) across `decks` ([k][40]; None: trainers[0]'s), the deal a uniform chance move.  A store's policy is a function of the key
    pair alone, so the trainers' own roots and decks do not matter.  K <= 16, at most 4 rounds to go, k * 36^R <= 1 << 22, K * k * 36^R <= 1 << 24.
    out[a][a][0] is trainers[a].policy_value(...) bit for bit."""
    trainers = list(trainers)
    root = None if root_actions is None else trainers[0]._root_after(root_actions).s
    return _lib.FullChanceMCCFR.cross_play([t.solver for t in trainers], root, 1 if current else 0, decks)


def evaluate(a, b, n, decks=None, stream_id=0):
    """A sampled seat-swapped match of trainer a's average policy against trainer b's from a's root (scopa_full_chance_pair_match, one launch): the first
    ceil(n / 2) episodes have a in seat 0, episode i on deck j mod k (j = i, or i - ceil(n / 2) in the second half) of `decks` ([k][40]; None: a's).
    -> {"episodes", "reward": a's mean reward, "std_error": its sampled standard error, "a_scopas", "b_scopas": mean scopas per episode,
    "by_seat": per seat of a {episodes, reward, exact_reward, exact_std_error}, "exact_by_seat", "exact_reward", "exact_std_error", "sums": the raw
    int64 [6]}.  Where a's root has at most 4 rounds to go and the forest fits cross_play's limits the exact fields come from cross_play([a, b]) on
    that root and those decks: exact_reward of seat 0 is out[a][b][0], of seat 1 -out[b][a][0], "exact_reward" their mean weighted by the episodes
    played in each seat, and the standard errors come from the exact second moments, sqrt((E[r^2] - E[r]^2) / episodes).  Otherwise (the deal's
    root) the exact fields are None: the match is then the only measure there is (sampled_exploitability gives a lower bound on a store's
    exploitability there).
    The exact target weights the decks uniformly while the match plays deck j mod k: the two describe the same law where ceil(n / 2) is a multiple
    of k and n is even (every deck then gets the same number of episodes in either seat)."""
    n = int(n)
    sums = a.solver.pair_match(b.solver, n, stream_id, decks)
    k = a.decks.shape[0] if decks is None else np.ascontiguousarray(decks, np.uint8).reshape(-1, 40).shape[0]
    exact = cross_play([a, b], decks=decks) if _forest_fits(a.solver.root, k, 2) else None
    return match_report(sums, n, exact)


def sampled_exploitability(trainer, iterations, n_episodes, batch=None, sample=None, seed=0, capacity_log2=None, decks=None, stream_id=0):
    """A LOWER BOUND on the exploitability of `trainer`'s average policy from ITS root, the deal included, where no exact sweep fits: a responder is
    trained `iterations` iterations against the frozen store with the external-sampling walk (trainer.sampled_response), made a pure policy, and
    played against the store in a seat-swapped match of n_episodes (pair_match, the response as "a").  -> match_report's dictionary with
    "lower_bound": True: "reward" is the sampled mean over both seatings -- an estimate of what this one responder wins, which is at most
    (BR0 + BR1) / 2 -- and by_seat[p]["reward"] what it wins in seat p (at most BR_p).  The responder is a real key-pair policy, so what it wins is
    achieved; more iterations can only find a better one, never prove that none exists.  Where the sub-game fits the sweeps (at most 4 rounds to
    go, decks * 36^R <= 1 << 22) the exact fields are cross_play([response, trainer])'s -- the responder's exact value, to set beside
    trainer.exploitability(), which it cannot exceed at one round to go -- and None otherwise.  decks: [k][40] to train the response and play the
    match on (None: the trainer's); batch, sample, seed and capacity_log2 are sampled_response's.  Its `current` is deliberately not offered:
    the match (pair_match) and cross_play's default play the store's AVERAGE policy, so the response is trained against the average policy too."""
    resp = trainer.sampled_response(iterations, batch=batch, sample=sample, seed=seed, capacity_log2=capacity_log2, decks=decks)
    try:
        return response_report(resp, trainer, n_episodes, decks, stream_id)
    finally:
        resp.close()


def response_report(response, trainer, n_episodes, decks=None, stream_id=0):
    """What a hardened response trainer (trainer.sampled_response) wins against `trainer`'s average policy: the seat-swapped match of n_episodes
    from the response's root on `decks` (None: the response's own), with cross_play([response, trainer])'s exact fields where the sub-game fits
    the sweeps -> match_report's dictionary with "lower_bound": True.  sampled_exploitability's measuring half, for a response that is trained on
    in steps (solver.respond_iterate, solver.harden) and measured after each."""
    n = int(n_episodes)
    sums = response.solver.pair_match(trainer.solver, n, stream_id, decks)
    k = response.decks.shape[0] if decks is None else np.ascontiguousarray(decks, np.uint8).reshape(-1, 40).shape[0]
    exact = cross_play([response, trainer], decks=decks) if _forest_fits(response.solver.root, k, 2) else None
    out = match_report(sums, n, exact)
    out["lower_bound"] = True
    return out


def match_report(sums, n, exact=None):
    """evaluate's dictionary from a match's six sums over n episodes and, where there is one, cross_play([a, b])'s exact table (None: the exact
    fields are None); shared by evaluate and FullChanceDeepCFR.match"""
    first = (n + 1) // 2
    counts = (first, n - first)
    seats = []
    for seat, m in enumerate(counts):
        rec = {"episodes": m, "reward": 0.5 * int(sums[seat]) / m if m else 0.0, "exact_reward": None, "exact_std_error": None}
        if exact is not None:
            cell = exact[0][1] if seat == 0 else exact[1][0]
            e, e2 = float(cell[0]), float(cell[1])
            rec["exact_reward"] = e if seat == 0 else -e
            rec["exact_std_error"] = float(np.sqrt(max(e2 - e * e, 0.0) / m)) if m else 0.0
        seats.append(rec)
    total, squares = float(sums[0] + sums[1]) / 2.0, float(sums[2] + sums[3]) / 4.0
    mean = total / n if n else 0.0
    var = max(squares / n - mean * mean, 0.0) * (n / (n - 1.0)) if n > 1 else 0.0
    out = {"episodes": n, "reward": mean, "std_error": float(np.sqrt(var / n)) if n else 0.0, "a_scopas": float(sums[4]) / n if n else 0.0,
           "b_scopas": float(sums[5]) / n if n else 0.0, "by_seat": seats, "exact_by_seat": None, "exact_reward": None, "exact_std_error": None,
           "sums": np.array(sums)}
    if exact is not None:
        out["exact_by_seat"] = (seats[0]["exact_reward"], seats[1]["exact_reward"])
        out["exact_reward"] = sum(h["episodes"] * h["exact_reward"] for h in seats) / n if n else 0.0
        out["exact_std_error"] = float(np.sqrt(sum((h["exact_std_error"] * h["episodes"]) ** 2 for h in seats))) / n if n else 0.0
    return out


class FullChanceMCCFRTrainer:
    def __init__(self, decks=None, seed=42, n_decks=8, root_actions=(), capacity_log2=22, batch=64, ctx=None, philox_seed=0x5C09A, fix_seat=None):
        """decks [n][40]: the set, `root_actions` (a prefix of whole rounds) played on decks[0]; or seed + n_decks:
        packet_decks(full_deal_py_seed(seed), rounds of root_actions, n_decks, seed, fix_seat)"""
        if int(batch) < 1:
            raise ValueError("batch must be a positive number of traversals per traverser and deck")
        if len(root_actions) % 6:
            raise ValueError("root_actions must end at a round boundary of a game in play (a multiple of 6 plies, fewer than 36)")
        if decks is None:
            decks = packet_decks(_lib.full_deal_py_seed(seed), len(root_actions) // 6, n_decks, seed, fix_seat)
        self.decks = np.ascontiguousarray(decks, np.uint8).reshape(-1, 40)
        root = _lib.FullState(deck=self.decks[0])
        for a in root_actions:
            if a not in root.legal():
                raise ValueError(f"root_actions: {a} is not legal after {list(root_actions)[:root.s[0]['step']]}")
            root.step(a)
        if root.is_terminal():
            raise ValueError("root_actions must end at a round boundary of a game in play (a multiple of 6 plies, fewer than 36)")
        self.batch = int(batch)
        self.root_actions = tuple(root_actions)
        self._own_ctx = ctx is None
        self.ctx = _lib.Context(0) if ctx is None else ctx
        if self._own_ctx:
            self.ctx.mccfr_seed(philox_seed)
        self.solver = _lib.FullChanceMCCFR(self.ctx, self.decks, root.s, capacity_log2)
        self.root = root
        self._tables = None
        self._cfr_t = 0

    def close(self):
        self.solver.close()
        if self._own_ctx:
            self.ctx.close()

    def _checked(self, call, *args):
        try:
            return call(*args)
        except _lib.ScopaError as e:
            if e.status == _lib.SCOPA_ENOMEM:
                c = self.solver.counters()
                raise RuntimeError(f"the infoset store (2^{self.solver.capacity_log2} slots, {c['rows']} rows) dropped {c['dropped']} updates: the rows "
                                   "kept are right, the dropped ones are lost -- save(), create a trainer with a larger capacity_log2, load()") from e
            raise
        finally:
            self._tables = None

    def _iterate(self, iterations, sample, seed):
        lists = None
        if sample is not None:
            lists = sample_decks(self.decks.shape[0], int(sample), iterations, seed, start=self.counters()["iterations"] // 2)
        self._checked(self.solver.iterate, self.batch, iterations, lists)

    def train(self, iterations, sample=None, seed=0, exploitability_freq=None):
        """`iterations` iterations of traverse(0), apply, traverse(1), apply with `batch` traversals per deck; sample=m: each iteration walks only m of
        the decks, sample_decks(n, m, iterations, seed, start=iterations done so far); nothing is rescaled.  exploitability_freq = k: in chunks of
        k, with one record (iteration, exploitability, br0, br1, value) of the average policy on the trainer's root and decks after each chunk (at
        most 4 rounds to go, decks x 36^R <= 1 << 22) -> the records; None: no records, one call, [].  The deck samples are keyed by the absolute
        iteration, so a chunked run walks the decks one long run walks."""
        iterations = int(iterations)
        if exploitability_freq is None:
            self._iterate(iterations, sample, seed)
            return []
        k = int(exploitability_freq)
        if k < 1:
            raise ValueError("exploitability_freq must be a positive number of iterations")
        records, done = [], 0
        while done + k <= iterations:
            self._iterate(k, sample, seed)
            done += k
            e = self.exploitability()
            records.append((self.counters()["iterations"] // 2, e["exploitability"], e["br0"], e["br1"], e["value"]))
        if done < iterations:
            self._iterate(iterations - done, sample, seed)
        return records

    def solve_cfr(self, iterations, variant="dcfr", alternating=True, root_actions=None, exploitability_freq=None, **params):
        """`iterations` exact weighted CFR iterations (scopa_full_chance_cfr_iterate) on the sub-games after `root_actions` (None: the trainer's
        root) on the trainer's decks, with the weights schedule(variant, t, n, **params); t counts the iterations of every solve_cfr call on this
        trainer, so a chunked run uses the weights of one long run.  exploitability_freq = k: in chunks of k, with one record
        (t, exploitability, br0, br1, value) of the average policy on that root after each chunk, kept in self.cfr_records -> the sweep values
        [2] of the last iteration (None where iterations is 0).  At most 4 rounds to go and decks x 36^R <= 1 << 22.  With more than one round to
        go the pair has imperfect recall and CFR has no convergence proof: watch the lower bound `exploitability`."""
        from .cfr_variants import schedule
        iterations = int(iterations)
        schedule(variant, 0, 0, **params)                       # raises ValueError on an unknown variant or bad parameters
        k = iterations if exploitability_freq is None else int(exploitability_freq)
        if exploitability_freq is not None and k < 1:
            raise ValueError("exploitability_freq must be a positive number of iterations")
        root = None if root_actions is None else self._root_after(root_actions).s
        self.cfr_records = []
        last, done = None, 0
        while done < iterations:
            chunk = min(k, iterations - done)
            values = self._checked(self.solver.cfr_iterate, chunk, schedule(variant, self._cfr_t, chunk, **params), alternating, root)
            self._cfr_t += chunk
            done += chunk
            last = values[-1].copy()
            if exploitability_freq is not None and chunk == k:
                e = self.solver.exploitability(root, 0)
                self.cfr_records.append((self._cfr_t, e["exploitability"], e["br0"], e["br1"], e["value"]))
        return last

    def _root_after(self, root_actions):
        """the state after `root_actions` from the deal of decks[0]: it must be a round boundary of a game in play"""
        root = _lib.FullState(deck=self.decks[0])
        for a in root_actions:
            if a not in root.legal():
                raise ValueError(f"root_actions: {a} is not legal after {list(root_actions)[:root.s[0]['step']]}")
            root.step(a)
        if root.is_terminal() or int(root.s[0]["step"]) % 6:
            raise ValueError("root_actions must end at a round boundary of a game in play (a multiple of 6 plies, fewer than 36)")
        return root

    def exploitability(self, root_actions=None, current=False, decks=None):
        """-> dict(exploitability, br0, br1, value) of the average policy (current=True: of the current regret-matching strategy) across `decks`
        ([k][40], e.g. held-out decks of the packet; None: the trainer's), the deal a uniform chance move, on the sub-games after `root_actions`
        played on decks[0] of the trainer (None: the trainer's root), exactly.  Every deck must fit that root; at most 4 rounds to go and
        k * 36^R <= 1 << 22.  The responder plays one action per information state on every deck; the state forgets the player's own plays of
        earlier rounds, so with more than one round to go br_p is the exact value of A pure response and `exploitability` a lower bound."""
        root = None if root_actions is None else self._root_after(root_actions).s
        return self.solver.exploitability(root, 1 if current else 0, decks)

    def policy_value(self, root_actions=None, current=False, decks=None):
        """the exact value, for player 0, of the policy against itself on those sub-games, averaged over the decks"""
        return self.exploitability(root_actions, current, decks)["value"]

    def cross_play(self, others, root_actions=None, current=False, decks=None):
        """cross_play([self] + others, ...): self is index 0, so its root and decks are the defaults"""
        return cross_play([self] + list(others), root_actions, current, decks)

    def evaluate_vs(self, other, n, decks=None, stream_id=0):
        """evaluate(self, other, n, decks, stream_id): this trainer's average policy against another trainer's, sampled and (R <= 4) exact"""
        return evaluate(self, other, n, decks, stream_id)

    def sampled_response(self, iterations, batch=None, sample=None, seed=0, current=False, capacity_log2=None, decks=None):
        """A sampled best response to this trainer's FROZEN store, from its root (the deal included): a new FullChanceMCCFRTrainer on the same root and
        context, on `decks` ([k][40] that fit the root; None: this trainer's), trained `iterations` iterations of respond_traverse(0), apply,
        respond_traverse(1), apply at `batch` traversals per deck (None: this trainer's batch) against this store's average policy (current=True:
        its current regret-matching sigma) and then hardened: its strategy rows are the pure policy of its regrets, which evaluate, cross_play and
        exploitability play unchanged.  sample / seed as for train; capacity_log2 None: this store's.  This store is only read.  The caller closes
        the response trainer; its solver.respond_iterate(self.solver, ...) and solver.harden() continue the training."""
        resp = FullChanceMCCFRTrainer(decks=self.decks if decks is None else decks, root_actions=self.root_actions,
                                      capacity_log2=self.solver.capacity_log2 if capacity_log2 is None else capacity_log2,
                                      batch=self.batch if batch is None else batch, ctx=self.ctx)
        try:
            iterations = int(iterations)
            lists = None if sample is None else sample_decks(resp.decks.shape[0], int(sample), iterations, seed)
            resp._checked(resp.solver.respond_iterate, self.solver, 1 if current else 0, resp.batch, iterations, lists)
            resp._checked(resp.solver.harden)
        except Exception:
            resp.close()
            raise
        return resp

    def sampled_exploitability(self, iterations, n_episodes, **kw):
        """sampled_exploitability(self, iterations, n_episodes, ...): a sampled LOWER bound on this store's exploitability, from any root"""
        return sampled_exploitability(self, iterations, n_episodes, **kw)

    def best_response(self, player):
        """{(player, information_state_string): action card} of the response of `player` from the last exploitability() call, decoded from the key
        pair alone as tables() does: the card is the chosen slot's, the slots being the hand in ascending card id"""
        keys, _, action, _ = self.solver.response_get(player)
        out = {}
        for (a, b), x in zip(keys.tolist(), action.tolist()):
            f = _lib.full_wide_key_fields(a, b)
            out[(f["player"], _lib.full_wide_key_to_string(a, b))] = int(f["hand"][int(x)])
        return out

    def counters(self):
        return self.solver.counters()

    def tables(self):
        """-> dict(keys [n][2], n_act, regret, strategy: arrays sorted by (A, B); info_sets: {(player, information_state_string): InfoNode}), the strings
        decoded from the key alone; an InfoNode's legal_actions are the cards in ascending id, the order of its rows"""
        if self._tables is None:
            keys, n_act, R, S = self.solver.tables_get()
            info, index = {}, {}
            for i, ((a, b), n, r, s) in enumerate(zip(keys.tolist(), n_act, R, S)):
                f = _lib.full_wide_key_fields(a, b)
                info[(f["player"], _lib.full_wide_key_to_string(a, b))] = InfoNode(f["hand"], r[:n].copy(), s[:n].copy())
                index[(a, b)] = i
            self._tables = dict(keys=keys, n_act=n_act, regret=R, strategy=S, info_sets=info, index=index)
        return self._tables

    @property
    def info_sets(self):
        return self.tables()["info_sets"]

    def average_policy(self, state):
        """{action: probability} of the mover at a FullScopaState / _lib.FullState on ANY deck, in the state's legal-action order: the strategy row
        normalised, its slots (ascending card id) mapped by card; uniform where the key is absent or the sum <= 1e-12 (ScopaLearnedPolicy)"""
        fs = getattr(state, "_fs", state)
        if fs.is_terminal():
            return {}
        player = fs.current_player()
        legal = fs.legal(player)
        t = self.tables()
        i = t["index"].get(_lib.full_infoset_key_wide(fs, player)) if len(legal) > 1 else None
        if i is not None:
            row = t["strategy"][i, :len(legal)]
            total = row.sum()
            if total > 1e-12:
                slot = {c: a for a, c in enumerate(sorted(legal))}
                return {c: float(row[slot[c]] / total) for c in legal}
        return {a: 1.0 / len(legal) for a in legal}

    def evaluate_vs_random(self, n=10000, decks=None, stream_id=0):
        """evaluate_agent's result for the average policy against uniform play from the root, first half of the episodes in seat 0, on the trainer's
        decks or on `decks` [k][40] (held-out decks that fit the root) -> (mean reward, its standard error, scopa statistics)"""
        n = int(n)
        sums = self.solver.match(n, stream_id, decks)
        total, squares = float(sums[0] + sums[1]) / 2.0, float(sums[2] + sums[3]) / 4.0
        mean = total / n if n else 0.0
        var = max(squares / n - mean * mean, 0.0) * (n / (n - 1.0)) if n > 1 else 0.0
        trained, opponent = (float(sums[4]) / n, float(sums[5]) / n) if n else (0.0, 0.0)
        return mean, float(np.sqrt(var / n)) if n else 0.0, {"trained_avg": trained, "opponent_avg": opponent, "difference": trained - opponent,
                                                               "data_collected": n > 0}

    def save(self, path):
        t = self.tables()
        with open(path, "wb") as f:
            np.savez(f, decks=self.decks, root=self.solver.root, keys=t["keys"], n_act=t["n_act"], regret=t["regret"], strategy=t["strategy"])

    def load(self, path):
        """the rows of a checkpoint of the same root; the decks may differ -- the rows are by key, not by deck"""
        with np.load(path, allow_pickle=False) as z:
            if _root_id(z["root"]) != _root_id(self.solver.root):
                raise ValueError("the checkpoint is of another root")
            self._checked(self.solver.tables_set, z["keys"], z["n_act"], z["regret"], z["strategy"])
