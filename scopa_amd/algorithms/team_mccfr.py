"""External-sampling MCCFR on Team MiniScopa (TPIMiniScopaGame) with the reference's interface: what the reference's generic
`MCCFRTrainer(TPIMiniScopaGame()).train(k)` (src/algorithms/mc_cfr.py on src/envs/openspiel_team_mini_scopa.py) computes, on the device.

Two modes behind one class, as for MiniScopa (mc_cfr.py here):
  * default (`batch=None`): the reference's own sequential semantics.  `iteration()` draws the 69 964 uniforms the reference's np.random.choice calls
    would draw from the GLOBAL numpy stream and replays them on the device (scopa_team_mccfr_replay): tables come out bit-identical to the reference
    under the same np.random.seed.
  * `batch=B`: the throughput path (scopa_team_mccfr_iterate): B traversals per traverser per iteration against regrets frozen for the iteration,
    Philox draws.  The documented semantic difference of the MiniScopa batched path, held to tests/team_mccfr_ref.py's definition.

The tables are the team solver's (scopa_team_* in include/scopa.h) and stay on the device; `info_sets` is a lazy Mapping over host snapshots.
"""
import re
from collections.abc import Mapping

import numpy as np

from .. import _lib
from .mc_cfr import InfoNode, ScopaLearnedPolicy
from .team_cfr import LEVEL_OFFSET, N_CHOICE_DEPTHS, _branch

DRAWS_PER_ITERATION = sum(_lib.TEAM_MCCFR_DRAWS)   # decision visits per iteration(), forced plies included: one np.random.choice each (mc_cfr.py:55)
_KEY = re.compile(r"Team([01]):P[0-3]:H\[[^\]]*\]:T\[[^\]]*\]:A\[([0-9-]*)\]")


class TeamMCInfoSets(Mapping):
    """dict[(team, information-state string) -> InfoNode] of the reference's trainer, computed on demand: only nodes a decision visit has reached are
    in it.  A choice node returns its regret_sum and strategy_sum rows (zeros where only the other team's traversals came by); a forced node returns
    regret_sum [0.] and the strategy_sum the reference holds: the exact solver's leaf_reach_sum plus, per arrival of its own team's traversals at its
    depth-12 ancestor, 1 for the team's first forced ply and 2 for its second.  len = visited choice rows + 4 x visited depth-12 nodes.

    Iteration yields the visited keys in DFS pre-order.  That is NOT the reference's dict order (first-visit insertion order, which depends on the
    draws); ScopaLearnedPolicy only looks keys up, so the order is not observable through the policy."""

    def __init__(self, trainer):
        self._t = trainer

    def _walk(self, key):
        """-> (state at the node, depth, index within its level or of its depth-12 ancestor) of a VISITED node, or None"""
        if not (isinstance(key, tuple) and len(key) == 2 and isinstance(key[1], str)):
            return None
        m = _KEY.fullmatch(key[1])
        if m is None or key[0] != int(m.group(1)):
            return None
        acts = [int(x) for x in m.group(2).split("-")] if m.group(2) else []
        if len(acts) > 15 or any(a > 15 for a in acts):
            return None
        s, idx = _lib.TeamState(perm=self._t._perm), 0
        for d, a in enumerate(acts):
            legal = s.legal()
            if a not in legal:
                return None
            if d < N_CHOICE_DEPTHS:
                idx = idx * _branch(d) + legal.index(a)
            s.step(a)
        if s.is_terminal() or s.current_player() != key[0] or s.infoset_string(key[0]) != key[1]:
            return None
        return (s, len(acts), idx) if self._visited(len(acts), idx) else None

    def _visited(self, d, idx):
        seen, lv = self._t._snapshot_visits()
        return bool(seen[LEVEL_OFFSET[d] + idx]) if d < N_CHOICE_DEPTHS else bool(lv[0, idx] or lv[1, idx])

    def __contains__(self, key):
        return self._walk(key) is not None

    def __getitem__(self, key):
        found = self._walk(key)
        if found is None:
            raise KeyError(key)
        s, d, idx = found
        R, S, Q = self._t._snapshot_tables()
        if d < N_CHOICE_DEPTHS:
            row, b = LEVEL_OFFSET[d] + idx, _branch(d)
            return InfoNode(s.legal(), R[row, :b].copy(), S[row, :b].copy())
        team = (d & 3) >> 1
        arrivals = float(self._t._snapshot_visits()[1][team, idx])
        return InfoNode(s.legal(), np.zeros(1), np.array([Q[team, idx] + arrivals * (1.0 if (d & 1) == 0 else 2.0)]))

    def __len__(self):
        seen, lv = self._t._snapshot_visits()
        return int(np.count_nonzero(seen)) + 4 * int(np.count_nonzero(lv[0] + lv[1]))

    def __iter__(self):
        if not self._visited(0, 0):
            return
        stack = [(_lib.TeamState(perm=self._t._perm), 0, 0)]
        while stack:
            s, d, idx = stack.pop()
            team = s.current_player()
            yield (team, s.infoset_string(team))
            children = []
            for c, a in enumerate(s.legal()):
                k = idx * _branch(d) + c if d < N_CHOICE_DEPTHS else idx
                if d + 1 < 16 and self._visited(d + 1, k):
                    n = s.copy()
                    n.step(a)
                    children.append((n, d + 1, k))
            stack.extend(reversed(children))


class TeamMCCFRTrainer:
    """`TeamMCCFRTrainer(game).train(iterations)` for a TPIMiniScopaGame; `MCCFRTrainer(TPIMiniScopaGame(seed=s))` hands one back."""

    def __init__(self, game, batch=None, seed=0x5C09A, device=0):
        if batch is not None and int(batch) < 1:
            raise ValueError("batch must be None or a positive number of traversals per traverser")
        self.game = game
        self.batch = None if batch is None else int(batch)
        self._perm = _lib.deal_py_seed(game.seed)
        self.ctx = _lib.Context(device)
        self.ctx.mccfr_seed(seed)
        self.ctx.team_set_deal(self._perm)
        self._tables = self._visits = None
        self.info_sets = TeamMCInfoSets(self)

    def iteration(self):
        """One pass per team (mc_cfr.py:88-92)."""
        self._run(1)

    def train(self, iterations=10000):
        self._run(iterations)
        return []

    def _run(self, iterations):
        if self.batch is None:
            chunk, done = 16, 0   # 16 x 69 964 float64 = 9 MB per upload; drawn from the global numpy stream exactly as the reference consumes it
            while done < iterations:
                k = min(chunk, iterations - done)
                u = np.random.random_sample(DRAWS_PER_ITERATION * k)
                used = self.ctx.team_mccfr_replay(k, u)
                assert used == u.size
                done += k
        else:
            self.ctx.team_mccfr_iterate(self.batch, iterations)
        self._tables = self._visits = None

    def tabular_policy(self):
        return ScopaLearnedPolicy(self.game, self.info_sets)

    def exploitability(self):
        """(BR0 + BR1) / 2 of the average policy of the choice rows, exact (scopa_team_exploitability)"""
        return float(self.ctx.team_exploitability()[0])

    def _snapshot_tables(self):
        if self._tables is None:
            R, S, _, Q = self.ctx.team_tables_get(local=False)
            self._tables = (R, S, Q)
        return self._tables

    def _snapshot_visits(self):
        if self._visits is None:
            self._visits = self.ctx.team_mccfr_visits_get()
        return self._visits
