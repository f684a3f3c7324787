"""Single Deep CFR on Team MiniScopa over a set of deals (TeamChanceGame: chance picks one of n deals, a team's rows shared across deals by key).

The reference's DeepCFR runs unmodified on its team game: the "player" is the team of the seat to move, and the feature encoder reads the mover's hand
and the table only.  So MiniScopa's 34 features and 34-128-64-16 advantage net apply, ONE net per team, and a net is defined at keys of deals it
never trained on -- it is the one solver on this game whose memory does not grow with the number of deals.  An iteration, per team: the iteration's
deals (all, or a sample), ONE traversal call over them into the team's memory ring (scopa_team_chance_sdcfr_traverse: every listed deal's choice rows
and the traverser's forced nodes evaluated once, `batch` walks per deal, 1 653 rows per walk), the ring advanced, training as DeepCFR does.  The
average policy is a table over keys (scopa_team_chance_sdcfr_average_policy) and its exploitability across all deals is exact.  AdvantageNetwork,
DeviceMemory and StrategyBuffer are DeepCFR's, unchanged; the loop is ChanceDeepCFR's.
"""
import numpy as np
import torch

from ..._lib import TEAM_SDCFR_ROWS
from .chance_deep_cfr import ChanceDeepCFR, iteration_deals
from .deep_cfr import AdvantageNetwork, StrategyBuffer


def default_memory_size(deals_per_iteration, batch):
    """Rows of a team's ring: the reference's 100 000, or eight iterations' worth where an iteration writes more (1 653 rows per traversal)."""
    return max(100000, 8 * TEAM_SDCFR_ROWS * int(deals_per_iteration) * int(batch))


class TeamChanceDeepCFR(ChanceDeepCFR):
    """`TeamChanceDeepCFR(team_chance_game, batch=64).train(iterations, advantage_epochs)`; `.policy_table()` is [G][4] over the game's keys.

    The TeamChanceGame's Context must have been created on a caller's stream (`TeamChanceGame(perms, Context(device, stream=s.cuda_stream))`): the
    PyTorch side of the solver -- optimiser steps, snapshots -- is queued on that same stream, which is what orders it against the library's launches.
    The default batch is 64: the policy launch evaluates every choice row of a listed deal whatever the batch, as many net evaluations as a few
    hundred traversals visit, and a small batch wastes it."""

    ROWS_PER_TRAVERSAL = TEAM_SDCFR_ROWS

    def __init__(self, team_chance_game, batch=64, deals_per_iteration=None, seed=0x5C09A, memory_size=None, graph_training=False, train_backend="torch"):
        ctx = team_chance_game.ctx
        if ctx.stream is None:
            raise ValueError("TeamChanceDeepCFR needs a TeamChanceGame whose Context was created with stream=<torch stream>.cuda_stream")
        self.chance = team_chance_game
        self.game = None
        self.num_players = 2          # the two teams
        dev_index = int(ctx.device)
        self.device = f"cuda:{dev_index}"
        self.batch = int(batch)
        if self.batch < 1:
            raise ValueError("batch must be positive")
        self.deals_per_iteration = None if deals_per_iteration is None else int(deals_per_iteration)
        if self.deals_per_iteration is not None and not 1 <= self.deals_per_iteration <= team_chance_game.n:
            raise ValueError("deals_per_iteration must lie in 1 .. n")
        self.seed = int(seed)
        self._m = team_chance_game.n if self.deals_per_iteration is None else self.deals_per_iteration
        self._stream = torch.cuda.ExternalStream(ctx.stream, device=dev_index)
        ctx.mccfr_seed(self.seed)
        self.input_dim = 34
        rows = TEAM_SDCFR_ROWS * self._m * self.batch
        with torch.cuda.stream(self._stream):
            if memory_size is None:
                memory_size = default_memory_size(self._m, self.batch)
            if memory_size < rows:
                raise ValueError("memory_size must hold at least one iteration's traversals (1653 rows each)")
            self.advantage_nets = [AdvantageNetwork(self.input_dim, 16, self.device, memory_size=memory_size, use_graph=graph_training, train_backend=train_backend)
                                   for _ in range(self.num_players)]
            for a in self.advantage_nets:
                a._ctx, a._ctx_stream = ctx, self._stream
        self.strategy_buffers = [StrategyBuffer() for _ in range(self.num_players)]
        self.training_history = {"losses": [[] for _ in range(self.num_players)], "values": [[] for _ in range(self.num_players)],
                                 "buffer_sizes": [[] for _ in range(self.num_players)], "exploitability": []}
        self.deal_log = []           # (absolute iteration, the deals it listed: None = all) per queued iteration
        self._iteration = 0
        self.fused_traversal = True
        self.rank, self.world = 0, 1

    # ---- the traversal ----------------------------------------------------------------------------------------------
    def _traverse_batch_fused(self, player, batch, uniforms=None, sync=True):
        """One scopa_team_chance_sdcfr_traverse call: `batch` traversals of team `player` in each of the iteration's deals into its ring;
        -> root values [m * batch]."""
        if uniforms is not None:
            raise NotImplementedError("replayed draws are a single-deal MiniScopa form (scopa_sdcfr_traverse_fused)")
        deals = iteration_deals(self.chance.n, self.deals_per_iteration, self._iteration, self.seed)
        m = self.chance.n if deals is None else len(deals)
        mem = self.advantage_nets[player].buffer
        with torch.cuda.stream(self._stream), torch.no_grad():
            w = self._packed_weights()
            vals = torch.empty(m * batch, dtype=torch.float32, device=self.device)
            self.chance.sdcfr_traverse(player, batch, w.data_ptr(), mem.feat.data_ptr(), mem.regret.data_ptr(), 0,   # no mask stream: DeviceMemory.mask
                                       mem.capacity, mem.write_base, vals.data_ptr(), self._iteration, 0, deals)
            mem.advance(TEAM_SDCFR_ROWS * m * batch)
        if sync:
            self._stream.synchronize()
        return vals

    # ---- the average policy -----------------------------------------------------------------------------------------
    def get_policy(self, state, player):
        raise NotImplementedError("TeamChanceDeepCFR's policy is a table over keys: policy_table(), policy_table_for(other_game)")

    def uniform_table(self, game=None):
        """the uniform policy over a game's keys: [G][4] float64, 1 / legal count in the legal slots"""
        game = self.chance if game is None else game
        keys, _ = game.index()
        nl = 4 - ((keys >> np.uint64(60)).astype(np.int64) >> 2)
        return np.where(np.arange(4)[None, :] < nl[:, None], 1.0 / nl[:, None], 0.0)

    def evaluate_vs_random(self, num_episodes=100):
        """Average policy vs the uniform table over the game's deals, teams swapped at half time, the deal drawn per episode: (avg_reward, [trained
        scopas, random scopas]) from team_chance.evaluate on policy_table(); the halves apart are left in last_eval_by_team, the exact expectation in
        last_eval_exact_reward."""
        from ..team_chance import evaluate
        rep = evaluate(self.chance, self.policy_table(), self.uniform_table(), num_episodes)
        self.last_eval_by_team = rep["by_team"]
        self.last_eval_exact_reward = rep["exact_reward"]
        n = max(int(rep["episodes"]), 1)
        trained = sum(h["episodes"] * h["a_scopas"] for h in rep["by_team"]) / n
        opponent = sum(h["episodes"] * h["b_scopas"] for h in rep["by_team"]) / n
        return rep["reward"], [trained, opponent]

    def policy_table(self):
        """The average policy at every key of the game, both teams' rows: [G][4] float64, hand order, normalised with the uniform fallback of
        evaluate_vs_random -- TeamChanceGame.exploitability's format.  Queued on the solver's stream, behind any iteration queued before it."""
        return self._table_on(self.chance)

    def _table_on(self, game):
        with torch.cuda.stream(self._stream), torch.no_grad():
            out = torch.empty((game.G, 4), dtype=torch.float64, device=self.device)
            for team in range(self.num_players):
                self.strategy_buffers[team].policy_table_device(game, team, out)   # TeamChanceGame.sdcfr_average_policy: the same call over keys
            host = out.cpu()
        return host.numpy()

    def policy_table_for(self, other_game):
        """The average policy on the keys of another TeamChanceGame -- deals held out of training, say: [other_game.G][4] float64, the snapshots
        themselves evaluated at every key of that game (the same call on the other handle).  The other game must share this solver's stream, or its
        context's stream is synchronised against it here."""
        if other_game.ctx is self.chance.ctx or other_game.ctx.stream == self.chance.ctx.stream:
            return self._table_on(other_game)
        self._stream.synchronize()                  # the other context launches on a stream of its own: the snapshots must have landed
        out = torch.empty((other_game.G, 4), dtype=torch.float64, device=self.device)
        torch.cuda.current_stream(self.device).synchronize()
        for team in range(self.num_players):
            self.strategy_buffers[team].policy_table_device(other_game, team, out)
        other_game.ctx.synchronize()
        return out.cpu().numpy()

    def exploitability(self):
        """-> dict(exploitability, br0, br1, value_p0) of the average policy across all deals of the game, exact (TeamChanceGame.exploitability)."""
        out = self.chance.exploitability(self.policy_table())
        return dict(exploitability=float(out[0]), br0=float(out[1]), br1=float(out[2]), value_p0=float(out[3]))
