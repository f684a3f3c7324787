"""Vanilla CFR on Team MiniScopa (TPIMiniScopaGame) with the reference's interface and its exact numbers: what the reference's generic
`CFRTrainer(TPIMiniScopaGame()).train(k)` (src/algorithms/vanilla_cfr.py on src/envs/openspiel_team_mini_scopa.py) computes, on the device.

The information-state string ends in the whole action history, so for the game's fixed deal every node is its own infoset: 321 365 nodes with a
choice and 4 x 331 776 forced ones.  The tables stay on the device (scopa_team_* in include/scopa.h); `info_set_map` is a lazy Mapping over host
snapshots of them, not 1.6 million Python objects.
"""
import re
from collections.abc import Mapping

import numpy as np

from .. import _lib
from .cfr_variants import schedule
from .vanilla_cfr import InfoNode, LearnedCFRPolicy

N_CHOICE_DEPTHS = 12
LEVEL_OFFSET = (0, 1, 5, 21, 85, 341, 1109, 3413, 10325, 31061, 72533, 155477)   # include/scopa.h: rows are level-major
_KEY = re.compile(r"Team[01]:P[0-3]:H\[[^\]]*\]:T\[[^\]]*\]:A\[([0-9-]*)\]")


def _branch(depth):
    return 4 - (depth >> 2)


class TeamInfoSetMap(Mapping):
    """dict[information-state string -> InfoNode] of the reference's trainer, computed on demand.  `map[key]` parses the key's A[...] history, walks
    the deal to the node and returns an InfoNode with the reference's arrays (a forced node: regret_sum [0.], strategy_sum [leaf_reach_sum],
    local_strategy [1.]); a string that is not the key of a node of this deal is a KeyError.  len is 0 before the first traversal and 1 648 469
    after it (every traversal visits every node); iteration yields the keys in the reference's dict insertion order, DFS pre-order."""

    def __init__(self, trainer):
        self._t = trainer

    def _walk(self, key):
        """-> (state at the node, path of legal-action indices) or None"""
        m = _KEY.fullmatch(key) if isinstance(key, str) else None
        if m is None or not self._t._traversed:
            return None
        acts = [int(x) for x in m.group(1).split("-")] if m.group(1) else []
        if len(acts) > 15 or any(a > 15 for a in acts):
            return None
        s, path = _lib.TeamState(perm=self._t._perm), []
        for a in acts:
            legal = s.legal()
            if a not in legal:
                return None
            path.append(legal.index(a))
            s.step(a)
        return (s, path) if s.infoset_string(s.current_player()) == key else None

    def __contains__(self, key):
        return self._walk(key) is not None

    def __getitem__(self, key):
        found = self._walk(key)
        if found is None:
            raise KeyError(key)
        s, path = found
        R, S, L, Q = self._t._tables()
        idx = 0
        for d, c in enumerate(path[:N_CHOICE_DEPTHS]):
            idx = idx * _branch(d) + c
        d = len(path)
        if d < N_CHOICE_DEPTHS:
            row, b = LEVEL_OFFSET[d] + idx, _branch(d)
            return InfoNode(s.legal(), R[row, :b].copy(), S[row, :b].copy(), L[row, :b].copy())
        return InfoNode(s.legal(), np.zeros(1), np.array([Q[(d & 3) >> 1, idx]]), np.ones(1))

    def __len__(self):
        return _lib.TEAM_N_INFOSETS if self._t._traversed else 0

    def __iter__(self):
        if not self._t._traversed:
            return
        stack = [_lib.TeamState(perm=self._t._perm)]
        while stack:
            s = stack.pop()
            yield s.infoset_string(s.current_player())
            children = []
            for a in s.legal():
                c = s.copy()
                c.step(a)
                if not c.is_terminal():
                    children.append(c)
            stack.extend(reversed(children))


class TeamCFRTrainer:
    """`TeamCFRTrainer(game).train(steps)` for a TPIMiniScopaGame.  variant=None is the reference's vanilla CFR, bit for bit; "vanilla", "cfr+",
    "linear" or "dcfr" (alpha, beta, gamma) weight the same alternating sweep by cfr_variants.schedule, continued across train() calls."""

    def __init__(self, game, device=0, variant=None, alpha=1.5, beta=0.0, gamma=2.0):
        if variant is not None:
            schedule(variant, 0, 0, alpha, beta, gamma)          # raises ValueError on an unknown variant or bad parameters
        self.game = game
        self.variant = variant
        self._params = dict(alpha=alpha, beta=beta, gamma=gamma)
        self._t = 0                                              # weighted iterations done: the schedule's t, owned here
        self._perm = _lib.deal_py_seed(game.seed)
        self.ctx = _lib.Context(device)
        self.ctx.team_set_deal(self._perm)
        self._traversed = False
        self._snapshot = None
        self.info_set_map = TeamInfoSetMap(self)

    # -- reference surface ---------------------------------------------------------------------------------
    def _cfr_recursive(self, state, traversing_player, reach_p0, reach_p1):
        """One traversal from the ROOT state with reaches (1.0, 1.0) (vanilla_cfr.py:56-99) on the device; returns the root value.  The device
        sweep covers the whole tree, so any other state or reach is a ValueError."""
        if (getattr(state, "get_game", lambda: None)() is not self.game or state.is_terminal() or len(state.action_history) != 0
                or (reach_p0, reach_p1) != (1.0, 1.0) or traversing_player not in (0, 1)):
            raise ValueError("_cfr_recursive: only the root state of this trainer's game with reaches (1.0, 1.0) runs on the device")
        value = self.ctx.team_cfr_traverse(traversing_player)
        self._traversed, self._snapshot = True, None
        return value

    def train(self, steps: int, eval_interval: int = 1000, compute_exploitability: bool = False):
        """vanilla_cfr.py:105-120.  Exploitability is the library's exact best-response pass (the reference calls OpenSpiel's), returned as
        [(iteration, value), ...]."""
        history, done = [], 0
        while done < steps:
            chunk = steps - done
            if compute_exploitability:
                chunk = min(chunk, eval_interval - (done % eval_interval))
            weights = None if self.variant is None else schedule(self.variant, self._t, chunk, **self._params)
            self.ctx.team_cfr_iterate(chunk, weights, root_values=False)
            self._t += chunk
            done += chunk
            self._traversed, self._snapshot = True, None
            if compute_exploitability and done % eval_interval == 0:
                history.append((done, self.exploitability()))
        return history

    def exploitability(self):
        """(BR0 + BR1) / 2 of the average policy, exact"""
        return float(self.ctx.team_exploitability()[0])

    def minimax(self):
        """the deal's game value for team 0 by backward induction (one fixed deal is a perfect-information game): CFR's yardstick"""
        return self.ctx.team_minimax()

    def cross_play(self, policies):
        """Exact cross-play of K [TEAM_N_CHOICE][4] tables on the trainer's deal: -> float64 [K][K][4] (numpy), entry [a][b] = (E[reward of team 0],
        E[its square], E[scopas of team 0], E[scopas of team 1]) with table a as team 0 against table b as team 1 (team_chance.cross_play's form)"""
        import torch
        from .team_chance import device_stack
        stack = device_stack(self.ctx.device, _lib.TEAM_N_CHOICE, policies)
        k = stack.shape[0]
        out = torch.empty((k, k, 4), dtype=torch.float64, device=stack.device)
        torch.cuda.synchronize()
        self.ctx.team_cross_play(k, stack.data_ptr(), out.data_ptr())
        self.ctx.synchronize()
        return out.cpu().numpy()

    def evaluate(self, a, b, episodes=10000, seed=None, stream_id=16):
        """team_chance.evaluate on the trainer's deal: a sampled seat-swapped match of table a against table b with a's exact reward at both
        seatings and the standard error from the exact second moment"""
        import torch
        from .team_chance import device_stack, match_report
        n = int(episodes)
        pair = device_stack(self.ctx.device, _lib.TEAM_N_CHOICE, [a, b])
        if pair.shape[0] != 2:
            raise ValueError("evaluate: a and b must be one [TEAM_N_CHOICE][4] table each")
        if seed is not None:
            self.ctx.mccfr_seed(seed)
        exact = self.cross_play(pair)
        torch.cuda.synchronize()
        return match_report(self.ctx.team_match(pair[0].data_ptr(), pair[1].data_ptr(), n, (n + 1) // 2, stream_id), exact)

    def get_openspiel_policy(self):
        return LearnedCFRPolicy(self.game, self.info_set_map)

    def _tables(self):
        if self._snapshot is None:
            self._snapshot = self.ctx.team_tables_get()
        return self._snapshot
