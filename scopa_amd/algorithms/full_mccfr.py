"""External-sampling MCCFR on FullScopa (40 cards), on the device: the one game of the library the reference's generic MCCFRTrainer cannot run on
(its FullScopaGame has no clone()), and whose tree cannot be enumerated -- 36^6 histories per deal -- so the rows live in a keyed device store that
grows as infosets are met (scopa_full_mccfr_* in include/scopa.h, scopa_amd/csrc/scopa_full_mccfr.hip).

    t = FullMCCFRTrainer(seed=42, batch=1024)
    t.train(100)
    t.evaluate_vs_random(1 << 20)        # the seat-swapped match of evaluate_agent, average policy against uniform play
    u = FullMCCFRTrainer(seed=42, root_actions=prefix_of_2_rounds)
    u.train(100, exploitability_freq=10) # [(iteration, exploitability, br0, br1, value), ...]: exact sweeps of the 36^4 histories below the root

`root_actions` plays a prefix of whole rounds from the deal first ("solve from here"): the solver's root must be a round boundary.  Textbook external
sampling against regrets frozen for a launch; traverser nodes add no strategy term, so a player's strategy sums grow while it is the opponent.

`exploitability`, `policy_value` and `best_response` are exact on a sub-game with at most 4 rounds to go (scopa_full_mccfr_exploitability).  The
infoset key forgets the player's own plays of earlier rounds, so across rounds the partition has imperfect recall: the response is built level by
level and is THE best response with one round to go, A pure response -- its value exact -- with more.  br_p is then a value some responder really
achieves and (br0 + br1) / 2 a lower bound on the true exploitability, not proved to be at least the policy's own value.
"""
import numpy as np

from .. import _lib
from .mc_cfr import InfoNode


class FullMCCFRTrainer:
    def __init__(self, seed=42, deck=None, root_actions=(), capacity_log2=22, batch=1024, ctx=None, philox_seed=0x5C09A):
        if int(batch) < 1:
            raise ValueError("batch must be a positive number of traversals per traverser")
        self.deck = np.ascontiguousarray(_lib.full_deal_py_seed(seed) if deck is None else deck, np.uint8)
        root = self._root_after(root_actions)
        self.batch = int(batch)
        self._own_ctx = ctx is None
        self.ctx = _lib.Context(0) if ctx is None else ctx
        if self._own_ctx:
            self.ctx.mccfr_seed(philox_seed)
        self.solver = _lib.FullMCCFR(self.ctx, self.deck, root.s, capacity_log2)
        self.root = root
        self._tables = None

    def _root_after(self, root_actions):
        """the state after `root_actions` from the deal: it must be a round boundary of a game in play"""
        root = _lib.FullState(deck=self.deck)
        for a in root_actions:
            if a not in root.legal():
                raise ValueError(f"root_actions: {a} is not legal after {list(root_actions)[:root.s[0]['step']]}")
            root.step(a)
        if root.is_terminal() or int(root.s[0]["step"]) % 6:
            raise ValueError("root_actions must end at a round boundary of a game in play (a multiple of 6 plies, fewer than 36)")
        return root

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

    def iteration(self):
        """traverse(0), apply, traverse(1), apply with `batch` traversals each"""
        self._checked(self.solver.iterate, self.batch, 1)

    def train(self, iterations, exploitability_freq=None):
        """`iterations` iterations.  exploitability_freq = k: in chunks of k, with one record (iteration, exploitability, br0, br1, value) of the average
        policy on the trainer's root after each chunk (the root must have at most 4 rounds to go); None: no records, one call"""
        if exploitability_freq is None:
            self._checked(self.solver.iterate, self.batch, int(iterations))
            return []
        k = int(exploitability_freq)
        if k < 1:
            raise ValueError("exploitability_freq must be a positive number of iterations")
        records, done = [], 0
        while done + k <= int(iterations):
            self._checked(self.solver.iterate, self.batch, k)
            done += k
            e = self.exploitability()
            records.append((self.counters()["iterations"] // 2, e["exploitability"], e["br0"], e["br1"], e["value"]))
        if done < int(iterations):
            self._checked(self.solver.iterate, self.batch, int(iterations) - done)
        return records

    def exploitability(self, root_actions=None, current=False):
        """-> dict(exploitability, br0, br1, value) of the average policy (current=True: of the current regret-matching strategy) on the sub-game after
        `root_actions` from the deal (None: the trainer's root), exactly; at most 4 rounds to go.  See the module docstring on imperfect recall."""
        root = None if root_actions is None else self._root_after(root_actions).s
        return self.solver.exploitability(root, 1 if current else 0)

    def policy_value(self, root_actions=None, current=False):
        """the exact value, for player 0, of the policy against itself on that sub-game"""
        return self.exploitability(root_actions, current)["value"]

    def best_response(self, player):
        """{(player, information_state_string): action card} of the response of `player` from the last exploitability() call, decoded as tables() does"""
        keys, _, action, _ = self.solver.response_get(player)
        out = {}
        for k, a in zip(keys, action):
            f = _lib.full_key_fields(k, self.deck)
            out[(f["player"], _lib.full_key_to_string(k, self.deck))] = int(f["hand"][int(a)])
        return out

    def counters(self):
        return self.solver.counters()

    def tables(self):
        """-> dict(keys, n_act, regret, strategy: arrays sorted by key; info_sets: {(player, information_state_string): InfoNode}), the strings decoded
        from key + deck, so the dict lines up with MCCFRTrainer.info_sets"""
        if self._tables is None:
            keys, n_act, R, S = self.solver.tables_get()
            info = {}
            for k, n, r, s in zip(keys, n_act, R, S):
                f = _lib.full_key_fields(k, self.deck)
                info[(f["player"], _lib.full_key_to_string(k, self.deck))] = InfoNode(f["hand"], r[:n].copy(), s[:n].copy())
            self._tables = dict(keys=keys, n_act=n_act, regret=R, strategy=S, info_sets=info)
        return self._tables

    @property
    def info_sets(self):
        return self.tables()["info_sets"]

    def average_policy(self, state):
        """{action: probability} of the mover at a FullScopaState / _lib.FullState: the strategy row normalised, uniform where the key is absent or the
        sum <= 1e-12 (ScopaLearnedPolicy)"""
        fs = getattr(state, "_fs", state)
        if fs.is_terminal():
            return {}
        if not np.array_equal(fs.deck, self.deck):
            raise ValueError("the state is not on this trainer's deck")
        player = fs.current_player()
        legal = fs.legal(player)
        t = self.tables()
        key = _lib.full_infoset_key(fs, self.deck, player)
        i = int(np.searchsorted(t["keys"], np.uint64(key)))
        if len(legal) > 1 and i < t["keys"].size and int(t["keys"][i]) == key:
            row = t["strategy"][i, :len(legal)]
            total = row.sum()
            if total > 1e-12:
                return {a: float(p) for a, p in zip(legal, row / total)}
        return {a: 1.0 / len(legal) for a in legal}

    def evaluate_vs_random(self, n=10000, stream_id=0):
        """evaluate_agent's result for the average policy against uniform play from the root, first half of the episodes in seat 0 -> (mean reward,
        its standard error, scopa statistics)"""
        n = int(n)
        sums = self.solver.match(n, stream_id)
        total, squares = float(sums[0] + sums[1]) / 2.0, float(sums[2] + sums[3]) / 4.0
        mean = total / n if n else 0.0
        var = max(squares / n - mean * mean, 0.0) * (n / (n - 1.0)) if n > 1 else 0.0
        trained, opponent = (float(sums[4]) / n, float(sums[5]) / n) if n else (0.0, 0.0)
        return mean, float(np.sqrt(var / n)) if n else 0.0, {"trained_avg": trained, "opponent_avg": opponent, "difference": trained - opponent,
                                                               "data_collected": n > 0}

    def save(self, path):
        t = self.tables()
        with open(path, "wb") as f:
            np.savez(f, deck=self.deck, root=self.root.s, keys=t["keys"], n_act=t["n_act"], regret=t["regret"], strategy=t["strategy"])

    def load(self, path):
        with np.load(path, allow_pickle=False) as z:
            if not np.array_equal(z["deck"], self.deck) or z["root"].tobytes() != self.root.s.tobytes():
                raise ValueError("the checkpoint is of another deck or root")
            self._checked(self.solver.tables_set, z["keys"], z["n_act"], z["regret"], z["strategy"])
