"""Single Deep CFR on the chance game over a set of deals (ChanceGame: chance picks one of n deals, infosets shared across deals by key).

An advantage net's 34 features -- own hand, table -- are a function of the infoset key alone, so ONE net per player serves every deal and is defined
at keys of deals it never trained on.  An iteration, per player: take the iteration's deals (all, or a sample), ONE traversal call over them into
the player's memory ring (scopa_chance_sdcfr_traverse: every listed deal's decision nodes evaluated once, `batch` walks per deal), advance the ring,
train as DeepCFR does.  The average policy is a table over keys (scopa_chance_sdcfr_average_policy) and its exploitability across all deals is exact.
AdvantageNetwork, DeviceMemory and StrategyBuffer are DeepCFR's, unchanged; on a one-deal game the traversal ids, ring rows, training samples and
snapshot schedule are DeepCFR's, so rings and nets stay equal bit for bit.
"""
import numpy as np
import torch

from ..chance import sample_deals
from .deep_cfr import ROWS_PER_TRAVERSAL, AdvantageNetwork, DeepCFR, StrategyBuffer


def default_memory_size(deals_per_iteration, batch):
    """Rows of a player's ring: the reference's 100 000, or eight iterations' worth where an iteration writes more (41 rows per traversal)."""
    return max(100000, 8 * ROWS_PER_TRAVERSAL * int(deals_per_iteration) * int(batch))


def iteration_deals(n, deals_per_iteration, iteration, seed):
    """The deals of absolute iteration `iteration`: None = all n, else chance.sample_deals(n, m, iteration, 1, seed)[0] (int32 [m], ascending).
    Keyed by the absolute iteration: a run continued over several train() calls lists what one long run lists."""
    if deals_per_iteration is None:
        return None
    return sample_deals(n, deals_per_iteration, iteration, 1, seed)[0]


class ChanceDeepCFR(DeepCFR):
    """`ChanceDeepCFR(chance_game, batch=8).train(iterations, advantage_epochs)`; `.policy_table()` is [G][4] over the game's keys.

    The ChanceGame's Context must have been created on a caller's stream (`Context(device, stream=torch_stream.cuda_stream)`): the PyTorch side of the
    solver -- optimiser steps, snapshots -- is queued on that same stream, which is what orders it against the library's launches."""

    def __init__(self, chance_game, batch=8, deals_per_iteration=None, seed=0x5C09A, memory_size=None, graph_training=False, train_backend="torch"):
        ctx = chance_game.ctx
        if ctx.stream is None:
            raise ValueError("ChanceDeepCFR needs a ChanceGame whose Context was created with stream=<torch stream>.cuda_stream")
        self.chance = chance_game
        self.game = None
        self.num_players = 2
        dev_index = int(ctx.device)
        self.device = f"cuda:{dev_index}"
        self.batch = int(batch)
        if self.batch < 1:
            raise ValueError("batch must be positive")
        self.deals_per_iteration = None if deals_per_iteration is None else int(deals_per_iteration)
        if self.deals_per_iteration is not None and not 1 <= self.deals_per_iteration <= chance_game.n:
            raise ValueError("deals_per_iteration must lie in 1 .. n")
        self.seed = int(seed)
        self._m = chance_game.n if self.deals_per_iteration is None else self.deals_per_iteration
        self._stream = torch.cuda.ExternalStream(ctx.stream, device=dev_index)
        ctx.mccfr_seed(self.seed)
        self.input_dim = 34
        rows = ROWS_PER_TRAVERSAL * self._m * self.batch
        with torch.cuda.stream(self._stream):
            if memory_size is None:
                memory_size = default_memory_size(self._m, self.batch)
            if memory_size < rows:
                raise ValueError("memory_size must hold at least one iteration's traversals (41 rows each)")
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

    @property
    def _ctx(self):
        return self.chance.ctx

    # ---- the traversal ----------------------------------------------------------------------------------------------
    def _traverse_batch_fused(self, player, batch, uniforms=None, sync=True):
        """One scopa_chance_sdcfr_traverse call: `batch` traversals in each of the iteration's deals into `player`'s ring; -> root values [m * batch]."""
        if uniforms is not None:
            raise NotImplementedError("replayed draws are a single-deal form (scopa_sdcfr_traverse_fused)")
        deals = iteration_deals(self.chance.n, self.deals_per_iteration, self._iteration, self.seed)
        m = self.chance.n if deals is None else len(deals)
        mem = self.advantage_nets[player].buffer
        with torch.cuda.stream(self._stream), torch.no_grad():
            w = self._packed_weights()
            vals = torch.empty(m * batch, dtype=torch.float32, device=self.device)
            self.chance.sdcfr_traverse(player, batch, w.data_ptr(), mem.feat.data_ptr(), mem.regret.data_ptr(), 0,   # no mask stream: DeviceMemory.mask
                                       mem.capacity, mem.write_base, vals.data_ptr(), self._iteration, 0, deals)
            mem.advance(ROWS_PER_TRAVERSAL * m * batch)
        if sync:
            self._stream.synchronize()
        return vals

    def _traverse_batch(self, player, batch, uniforms=None, advantage_fn=None, fused=None, sync=True):
        if advantage_fn is not None or fused is False:
            raise NotImplementedError("the chance game has the library's traversal call only (policy tables + walks)")
        return self._traverse_batch_fused(player, batch, uniforms, sync=sync)

    def _external_sampling_cfr(self, state, player, depth=0, prob=1.0):
        raise NotImplementedError("ChanceDeepCFR traverses whole iterations: see train()")

    def _queue_iteration(self, advantage_epochs, train_batch=128, loop_index=None):
        self.deal_log.append((self._iteration, iteration_deals(self.chance.n, self.deals_per_iteration, self._iteration, self.seed)))
        return super()._queue_iteration(advantage_epochs, train_batch, loop_index)

    # ---- the average policy -----------------------------------------------------------------------------------------
    def get_policy(self, state, player):
        raise NotImplementedError("ChanceDeepCFR's policy is a table over keys: policy_table(), policy_table_for(ctx)")

    def evaluate_vs_random(self, num_episodes=100):
        """Average policy vs uniform random over the game's deals, seats swapped at half time, the deal drawn per episode: what
        DeepCFR.evaluate_vs_random returns -- (avg_reward, [trained scopas, random scopas]) -- from chance.evaluate on policy_table(); the halves
        apart are left in last_eval_by_seat, the exact expectation in last_eval_exact_reward."""
        from ..chance import evaluate
        avg, stats = evaluate(self.chance, self.policy_table(), num_episodes)
        self.last_eval_by_seat = stats["by_seat"]
        self.last_eval_exact_reward = stats.get("exact_reward")
        return avg, [stats["trained_avg"], stats["opponent_avg"]]

    def policy_table(self):
        """The average policy at every key of the game, both players' rows: [G][4] float64, hand order, normalised with the uniform fallback of
        evaluate_vs_random -- ChanceGame.exploitability's format.  Queued on the solver's stream, behind any iteration queued before it."""
        with torch.cuda.stream(self._stream), torch.no_grad():
            out = torch.empty((self.chance.G, 4), dtype=torch.float64, device=self.device)
            for player in range(self.num_players):
                self.strategy_buffers[player].policy_table_device(self.chance, player, out)   # ChanceGame.sdcfr_average_policy: the same call over keys
            host = out.cpu()
        return host.numpy()

    def policy_table_for(self, ctx):
        """The average policy on the deal `ctx` holds -- in the set or held out: [n_infosets][4] float64 through StrategyBuffer.policy_table_device, i.e.
        the nets themselves evaluated at every key of that deal (chance.table_for fills keys the set lacks with the uniform row instead)."""
        self._stream.synchronize()                  # ctx launches on a stream of its own: the snapshots must have landed
        out = torch.empty((ctx.n_infosets, 4), dtype=torch.float64, device=self.device)
        torch.cuda.current_stream(self.device).synchronize()
        for player in range(self.num_players):
            self.strategy_buffers[player].policy_table_device(ctx, player, out)
        ctx.synchronize()
        return out.cpu().numpy()

    def exploitability(self):
        """-> dict(exploitability, br0, br1, value_p0) of the average policy across all deals of the game, exact (ChanceGame.exploitability)."""
        out = self.chance.exploitability(self.policy_table())
        return dict(exploitability=float(out[0]), br0=float(out[1]), br1=float(out[2]), value_p0=float(out[3]))

    # ---- training loop ----------------------------------------------------------------------------------------------
    def train(self, iterations=100, advantage_epochs=10, exploitability_freq=None, verbose=False):
        """DeepCFR.train's loop (the host one iteration ahead of the device, snapshots from the call's second iteration on, weight = loop index + 1)
        without the matches against a random player.  exploitability_freq=k: at every iteration i of this call with i % k == 0 the queue is drained
        and (absolute iteration, exploitability) appended to training_history["exploitability"]."""
        if exploitability_freq is not None and (int(exploitability_freq) != exploitability_freq or exploitability_freq < 1):
            raise ValueError("exploitability_freq must be None or a positive integer")
        ahead = None
        for iteration in range(iterations):
            queued = self._queue_iteration(advantage_epochs, loop_index=iteration)
            if ahead is not None:
                self._resolve(ahead)
            ahead = queued
            if exploitability_freq is not None and iteration % exploitability_freq == 0:
                self._resolve(ahead)
                ahead = None
                expl = self.exploitability()["exploitability"]
                self.training_history["exploitability"].append((self._iteration - 1, expl))
                if verbose:
                    print(f"iter {self._iteration - 1}: exploitability {expl:.5f}")
        if ahead is not None:
            self._resolve(ahead)
