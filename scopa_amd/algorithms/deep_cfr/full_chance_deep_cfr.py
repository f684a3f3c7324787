"""Single Deep CFR on FullScopa over a set of decks: scopa_full_chance_sdcfr_* in include/scopa.h, scopa_amd/csrc/scopa_full_chance_sdcfr.hip.
traversal="forest" (the default) lays out the whole forest below the root and so runs on the sub-games the exact sweeps cover (a round-boundary root
with at most 4 rounds to go and decks * 36^R <= 1 << 22); traversal="frontier" keeps only the sampled frontier of every level and runs from any
round-boundary root, the deal included, on as many decks as the trainer holds.  The nets are functions of the key pair, so either way they are
measured on any sub-game the sweeps cover: exploitability(decks=..., root_actions=...).

The tabular solvers keep a row per key pair (A, B) and have nothing to say at a pair they never walked, so their policy carries little to decks
they have not seen.  Here the advantage net's 96 features are a function of the pair alone: ONE 96-128-64-40 net per player serves every deck and is
defined at every pair of every deck.  An iteration, per player: take the iteration's decks (all, or a sample keyed by the absolute iteration), ONE
traversal call over them into the player's memory ring, advance the ring, train as DeepCFR does (PyTorch by default; `train_backend="hip"`: the
hand-written step of scopa_full_train.hip, three launches per Adam step).  The average policy is a function of the pair too, so
`policy_store()` writes it into a FullChanceMCCFRTrainer's store and the existing exploitability, cross_play, evaluate, evaluate_vs_random and
best_response measure it unchanged, on training or held-out decks.

    decks = packet_decks(full_deal_py_seed(42), 3, 16, seed=1, fix_seat=0)
    d = FullChanceDeepCFR(decks[:8], root_actions=prefix_of_3_rounds, batch=64)
    d.train(50, advantage_epochs=10)
    d.exploitability()                      # exact, on the training decks
    d.exploitability(decks=decks[8:])       # ... and on held-out decks: the figure the nets exist for
    d.match(1 << 16, decks=decks[8:])       # a sampled match against uniform play, from any root -- the deal included, where no table fits
    d.sampled_lower_bound(100, 1 << 16)     # ... and what a responder trained against the nets wins there: a lower bound on their exploitability
"""
import numpy as np
import torch

from ... import _lib
from ..full_chance import FullChanceMCCFRTrainer, sample_decks
from .deep_cfr import AdvantageNetwork, DeepCFR, StrategyBuffer

FEATURES, ACTIONS = 96, 40
FULL_TRAIN_PARAMS = 128 * 96 + 128 + 64 * 128 + 64 + 40 * 64 + 40   # 23 272 (scopa_full_sdcfr_train_params), in net.parameters() order


def rows_per_traversal(R):
    """memory rows of one traversal with R rounds to go: the traverser's choice nodes, 4 (6^R - 1) / 5"""
    return 4 * (6 ** int(R) - 1) // 5


def default_memory_size(R, decks_per_iteration, batch):
    """Rows of a player's ring: the reference's 100 000, or eight iterations' worth where an iteration writes more."""
    return max(100000, 8 * rows_per_traversal(R) * int(decks_per_iteration) * int(batch))


def sweep_fits(R, n_decks):
    """whether the exact sweeps (and the forest traversal) cover n_decks trees of R rounds: R <= 4 and n_decks * 36^R <= 1 << 22"""
    return R <= 4 and int(n_decks) * 36 ** int(R) <= 1 << 22


def iteration_decks(n, decks_per_iteration, iteration, seed):
    """The decks of absolute iteration `iteration`: None = all n, else sample_decks(n, m, 1, seed, start=iteration)[0] (int32 [m], ascending)."""
    if decks_per_iteration is None:
        return None
    return sample_decks(n, decks_per_iteration, 1, seed, start=iteration)[0]


def key_features(keys2):
    """float32 [n][96] features of key pairs [n][2] (host code)"""
    return _lib.full_chance_sdcfr_features(keys2)


class FullAdvantageNetwork(AdvantageNetwork):
    """The 96-128-64-40 advantage net whose optimiser step is the hand-written one of scopa_full_train.hip (scopa_full_sdcfr_train_steps: three
    launches per step, Adam's moments in one [2][23272] buffer).  AdvantageNetwork's own "hip" is the 34-128-64-16 net's step, so the base is built
    with "torch" and the backend set afterwards; train() -- the Adam-settings check, the stream contract of _train_hip, the fallback with a one-time
    warning to PyTorch for ragged batches or a gradient all-reduce, the deferred device-scalar loss -- is inherited."""

    def __init__(self, device="cuda", lr=5e-4, memory_size=100000, use_graph=False):
        super().__init__(FEATURES, ACTIONS, device, lr=lr, memory_size=memory_size, use_graph=use_graph, train_backend="torch")
        self.train_backend = "hip"

    def _train_hip_on_stream(self, params, n, batch_size, epochs, defer):
        if self._hip is None:
            self._hip = (torch.zeros(2 * FULL_TRAIN_PARAMS, dtype=torch.float32, device=self.device), torch.zeros(1, dtype=torch.float32, device=self.device))
        state, loss = self._hip
        rows_all = self._sample_rows(n, batch_size, epochs).contiguous()
        loss.zero_()
        lr = float(self.optimizer.param_groups[0]["lr"])
        mask_ptr, _keep = self.buffer.mask_ptr
        self._ctx.full_sdcfr_train_steps(rows_all.data_ptr(), batch_size, epochs, self.buffer.feat.data_ptr(), self.buffer.regret.data_ptr(), mask_ptr,
                                         self.buffer.capacity, tuple(p.data_ptr() for p in params), state.data_ptr(), self._hip_step + 1, lr, loss.data_ptr())
        self._hip_step += epochs
        return loss[0] / epochs if defer else float(loss.item()) / epochs


class FullChanceDeepCFR(DeepCFR):
    """`FullChanceDeepCFR(trainer_or_decks, root_actions, batch).train(iterations, advantage_epochs)`; `.policy_store()` is a trainer whose store
    holds the average policy.

    trainer_or_decks: a FullChanceMCCFRTrainer whose Context was created on a caller's stream (`Context(device, stream=s.cuda_stream)`) -- its decks
    and root are the game, its store is left alone -- or decks [n][40], for which a stream, a context and a trainer of the solver's own are made with
    `root_actions` played on decks[0]."""

    def __init__(self, trainer_or_decks, root_actions=(), batch=64, decks_per_iteration=None, seed=0x5C09A, memory_size=None, graph_training=False,
                 train_backend="torch", traversal="forest"):
        # "torch" (default) or "hip": the optimiser step of the 96-128-64-40 nets in three hand-written launches (FullAdvantageNetwork), opt-in
        if train_backend not in ("torch", "hip"):
            raise ValueError("train_backend must be 'torch' or 'hip'")
        self.train_backend = train_backend
        # "forest" (default): scopa_full_chance_sdcfr_traverse, on the sub-games the exact sweeps cover; "frontier": ..._traverse_frontier, any root
        if traversal not in ("forest", "frontier"):
            raise ValueError("traversal must be 'forest' or 'frontier'")
        self.traversal = traversal
        if isinstance(trainer_or_decks, FullChanceMCCFRTrainer):
            self.trainer, self._own = trainer_or_decks, False
            if self.trainer.ctx.stream is None:
                raise ValueError("FullChanceDeepCFR needs a trainer whose Context was created with stream=<torch stream>.cuda_stream")
        else:
            self._own_stream = torch.cuda.Stream(device=0)
            ctx = _lib.Context(0, stream=self._own_stream.cuda_stream)
            self.trainer, self._own = FullChanceMCCFRTrainer(decks=trainer_or_decks, root_actions=tuple(root_actions), capacity_log2=4, batch=1, ctx=ctx), True
        ctx = self.trainer.ctx
        self.solver = self.trainer.solver
        self.decks = self.trainer.decks
        self.n_decks = int(self.decks.shape[0])
        self.R = 6 - int(self.solver.root[0]["round"])
        if traversal == "forest" and not sweep_fits(self.R, self.n_decks):
            raise ValueError("FullChanceDeepCFR: at most 4 rounds to go and decks * 36^R <= 1 << 22 (traversal='frontier' has no such limit)")
        self.game = None
        self.num_players = 2
        dev_index = int(ctx.device)
        self.device = f"cuda:{dev_index}"
        self.batch = int(batch)
        if self.batch < 1:
            raise ValueError("batch must be positive")
        self.decks_per_iteration = None if decks_per_iteration is None else int(decks_per_iteration)
        if self.decks_per_iteration is not None and not 1 <= self.decks_per_iteration <= self.n_decks:
            raise ValueError("decks_per_iteration must lie in 1 .. n")
        self.seed = int(seed)
        self._m = self.n_decks if self.decks_per_iteration is None else self.decks_per_iteration
        self._stream = torch.cuda.ExternalStream(ctx.stream, device=dev_index)
        ctx.mccfr_seed(self.seed)
        self.input_dim = FEATURES
        self.rows_per_traversal = rows_per_traversal(self.R)
        rows = self.rows_per_traversal * self._m * self.batch
        with torch.cuda.stream(self._stream):
            if memory_size is None:
                memory_size = default_memory_size(self.R, self._m, self.batch)
            if memory_size < rows:
                raise ValueError(f"memory_size must hold at least one iteration's traversals ({self.rows_per_traversal} rows each)")
            self.advantage_nets = [FullAdvantageNetwork(self.device, memory_size=memory_size, use_graph=graph_training) if train_backend == "hip" else
                                   AdvantageNetwork(FEATURES, ACTIONS, self.device, memory_size=memory_size, use_graph=graph_training, train_backend="torch")
                                   for _ in range(self.num_players)]
            for a in self.advantage_nets:
                a._ctx, a._ctx_stream = ctx, self._stream
            self._wstack = None
        self.strategy_buffers = [StrategyBuffer() for _ in range(self.num_players)]
        self.training_history = {"losses": [[] for _ in range(self.num_players)], "values": [[] for _ in range(self.num_players)],
                                 "buffer_sizes": [[] for _ in range(self.num_players)], "exploitability": []}
        self.deck_log = []           # (absolute iteration, the decks it listed: None = all) per queued iteration
        self._iteration = 0
        self.fused_traversal = True
        self.rank, self.world = 0, 1

    @property
    def _ctx(self):
        return self.trainer.ctx

    def close(self):
        if self._own:
            self.trainer.close()
            self.trainer.ctx.close()

    # ---- the traversal ----------------------------------------------------------------------------------------------
    def _stacked_weights(self):
        """the two players' parameters as six tensors [2][...] (the traversal call's layout), copied on the solver's stream"""
        params = [a.param_list() for a in self.advantage_nets]
        if self._wstack is None:
            self._wstack = [torch.empty((2,) + tuple(p.shape), dtype=torch.float32, device=self.device) for p in params[0]]
        for k, t in enumerate(self._wstack):
            torch._foreach_copy_([t[0], t[1]], [params[0][k].detach(), params[1][k].detach()])
        return self._wstack

    def _traverse_batch_fused(self, player, batch, uniforms=None, sync=True):
        """One scopa_full_chance_sdcfr_traverse (or, with traversal="frontier", _traverse_frontier) call: `batch` traversals in each of the iteration's decks into `player`'s ring; -> root values [m * batch]."""
        if uniforms is not None:
            raise NotImplementedError("replayed draws are a single-deal MiniScopa form (scopa_sdcfr_traverse_fused)")
        decks = iteration_decks(self.n_decks, self.decks_per_iteration, self._iteration, self.seed)
        m = self.n_decks if decks is None else len(decks)
        mem = self.advantage_nets[player].buffer
        with torch.cuda.stream(self._stream), torch.no_grad():
            w = self._stacked_weights()
            vals = torch.empty(m * batch, dtype=torch.float32, device=self.device)
            call = self.solver.sdcfr_traverse_frontier if self.traversal == "frontier" else self.solver.sdcfr_traverse
            call(player, batch, [t.data_ptr() for t in w], mem.feat.data_ptr(), mem.regret.data_ptr(), mem.capacity, mem.write_base,
                 vals.data_ptr(), self._iteration, 0, decks)
            mem.advance(self.rows_per_traversal * m * batch)
        if sync:
            self._stream.synchronize()
        return vals

    def _traverse_batch(self, player, batch, uniforms=None, advantage_fn=None, fused=None, sync=True):
        if advantage_fn is not None or fused is False:
            raise NotImplementedError("FullScopa over decks has the library's traversal call only (policy tables + walks)")
        return self._traverse_batch_fused(player, batch, uniforms, sync=sync)

    def _external_sampling_cfr(self, state, player, depth=0, prob=1.0):
        raise NotImplementedError("FullChanceDeepCFR traverses whole iterations: see train()")

    def _queue_iteration(self, advantage_epochs, train_batch=128, loop_index=None):
        self.deck_log.append((self._iteration, iteration_decks(self.n_decks, self.decks_per_iteration, self._iteration, self.seed)))
        return super()._queue_iteration(advantage_epochs, train_batch, loop_index)

    # ---- the average policy -----------------------------------------------------------------------------------------
    def _root_of(self, root_actions):
        return None if root_actions is None else self.trainer._root_after(root_actions).s

    def _average_nodes(self, player, decks=None, root=None, buffers=None):
        """(keys [N][2], policy [N][3] float64) of every choice node of `player`: scopa_full_chance_sdcfr_average_policy behind the solver's stream;
        buffers: another solver's strategy buffers on this device in place of this one's (FullChanceDeepCFR.match's exact fields)"""
        buf = (self.strategy_buffers if buffers is None else buffers)[player]
        n = len(buf._slots)
        with torch.cuda.stream(self._stream), torch.no_grad():
            coef = None
            if n:
                total = float(sum(buf.weights))
                coef = torch.tensor([w / total for w in buf.weights], dtype=torch.float32, device=self.device)   # float32(weight / total), as the reference's product rounds it
            out = self.solver.sdcfr_average_policy(player, buf._slots if n else [], [t.data_ptr() for t in buf._store] if n else [0] * 6, buf.max_size,
                                                   coef.data_ptr() if n else 0, decks, root)
        return out

    def _check_sweep(self, decks, root_actions):
        """the exact sweeps behind the measurements lay out every tree below the root: refuse here, by name, what they would refuse below"""
        R = self.R if root_actions is None else 6 - len(tuple(root_actions)) // 6
        n = self.n_decks if decks is None else len(decks)
        if not sweep_fits(R, n):
            raise ValueError(f"the exact sweeps cover at most 4 rounds to go and decks * 36^R <= 1 << 22: {n} decks at R = {R} lie outside; "
                             "pass root_actions (a longer prefix) and/or decks (fewer) that fit")

    def policy_rows(self, decks=None, root_actions=None, buffers=None):
        """The average policy as distinct store rows -> (keys2 [n][2] uint64 sorted by (A, B), n_act [n] int32, strategy [n][3] float64), both players',
        from the per-node average policy on `decks` ([k][40] that fit the root; None: the solver's) below `root_actions` (None: the solver's root).
        Nodes that share a pair carry equal bits (the policy is a function of the pair), which is asserted."""
        self._check_sweep(decks, root_actions)
        root = self._root_of(root_actions)
        keys, pol = [], []
        for player in range(self.num_players):
            k, p = self._average_nodes(player, decks, root, buffers)
            keys.append(k)
            pol.append(p)
        keys, pol = np.concatenate(keys), np.concatenate(pol)
        order = np.lexsort((keys[:, 1], keys[:, 0]))
        keys, pol = keys[order], pol[order]
        first = np.ones(len(keys), bool)
        first[1:] = (keys[1:] != keys[:-1]).any(axis=1)
        group = np.cumsum(first) - 1
        ukeys, upol = keys[first], pol[first]
        assert np.array_equal(upol[group].view(np.uint64), pol.view(np.uint64)), "nodes of one key pair carry different policy bits"
        n_act = np.array([bin(int(b)).count("1") for b in ukeys[:, 1]], np.int32)
        return ukeys, n_act, upol

    def policy_store(self, decks=None, root_actions=None, capacity_log2=None):
        """A FullChanceMCCFRTrainer (on the solver's context, decks and root) whose store holds policy_rows(decks, root_actions) as strategy rows,
        written with tables_set: exploitability, cross_play, evaluate, evaluate_vs_random and best_response apply to it unchanged, on the training
        decks or, with `decks`, on held-out ones.  With `root_actions` the trainer stands at THAT root (on `decks`, or the solver's), so its sampled
        matches start there too.  The caller closes it.  ValueError where (decks, root) lies outside the exact sweeps' limits."""
        keys, n_act, pol = self.policy_rows(decks, root_actions)
        if capacity_log2 is None:
            capacity_log2 = max(4, int(np.ceil(np.log2(max(len(keys), 1) * 2 + 1))))
        if root_actions is None:
            t = FullChanceMCCFRTrainer(decks=self.decks, root_actions=self.trainer.root_actions, capacity_log2=capacity_log2, batch=1, ctx=self.trainer.ctx)
        else:
            t = FullChanceMCCFRTrainer(decks=self.decks if decks is None else decks, root_actions=tuple(root_actions), capacity_log2=capacity_log2, batch=1,
                                       ctx=self.trainer.ctx)
        if len(keys):
            t._checked(t.solver.tables_set, keys, n_act, np.zeros_like(pol), pol)
        return t

    def exploitability(self, decks=None, root_actions=None):
        """-> dict(exploitability, br0, br1, value) of the average policy across `decks` ([k][40]; None: the training decks) below `root_actions`
        (None: the solver's root), exact (FullChanceMCCFRTrainer.exploitability on policy_store(decks, root_actions)).  ValueError where the
        sub-game lies outside the exact sweeps' limits."""
        t = self.policy_store(decks, root_actions)
        try:
            return t.exploitability(decks=decks, root_actions=root_actions)
        finally:
            t.close()

    def sampled_exploitability(self, iterations, n_episodes, decks=None, root_actions=None, **kw):
        """full_chance.sampled_exploitability of the nets' average policy through policy_store(decks, root_actions): a sampled LOWER bound on its
        exploitability, with cross_play's exact value of the responder beside it.  A store of the policy exists only where the exact sweeps reach,
        so this covers those sub-games alone: ValueError (naming the limit) elsewhere -- from the deal, or on more decks than a store fits, use
        sampled_lower_bound, which trains the response against the nets themselves."""
        from ..full_chance import sampled_exploitability
        t = self.policy_store(decks, root_actions)
        try:
            return sampled_exploitability(t, iterations, n_episodes, decks=decks, **kw)
        finally:
            t.close()

    def sampled_response(self, iterations, batch=None, sample=None, seed=0, capacity_log2=None, decks=None, root_actions=None):
        """A sampled best response to the nets' average policy AS THE STRATEGY BUFFERS HOLD IT NOW, from any round-boundary root, the deal included
        (scopa_full_chance_respond_nets_iterate): a new FullChanceMCCFRTrainer on the solver's context, at `root_actions`' root (None: the solver's) on
        `decks` ([k][40] that fit the root; None: the training decks), trained `iterations` iterations of respond_nets_traverse(0), apply,
        respond_nets_traverse(1), apply at `batch` traversals per deck (None: the solver's batch) and then hardened: its strategy rows are the pure
        policy of its regrets, which match(opponent=...), cross_play and exploitability play unchanged.  sample / seed as for
        FullChanceMCCFRTrainer.train; capacity_log2 None: sized from the rows the traversals can claim, never below the store's default 22.  The
        nets and their snapshots are only read.  The caller closes the response trainer; its
        solver.respond_nets_iterate([self._snapshot_set(p)[0] for p in (0, 1)], batch) and solver.harden() continue the training."""
        iterations = int(iterations)
        batch = self.batch if batch is None else int(batch)
        if batch < 1:
            raise ValueError("batch must be positive")
        held = self.decks if decks is None else np.ascontiguousarray(decks, np.uint8).reshape(-1, 40)
        acts = self.trainer.root_actions if root_actions is None else tuple(root_actions)
        if capacity_log2 is None:
            R = 6 - len(acts) // 6
            per_iteration = 2 * rows_per_traversal(R) * (len(held) if sample is None else int(sample)) * batch
            capacity_log2 = min(28, max(22, int(np.ceil(np.log2(2 * max(iterations, 1) * per_iteration + 1)))))
        resp = FullChanceMCCFRTrainer(decks=held, root_actions=acts, capacity_log2=capacity_log2, batch=batch, ctx=self.trainer.ctx)
        try:
            lists = None if sample is None else sample_decks(resp.decks.shape[0], int(sample), iterations, seed)
            sets = [self._snapshot_set(p) for p in range(2)]          # (made on the solver's stream, where the walk's launches are queued)
            resp._checked(resp.solver.respond_nets_iterate, [s[0] for s in sets], batch, iterations, lists)
            resp._checked(resp.solver.harden)
            del sets
        except Exception:
            resp.close()
            raise
        return resp

    def sampled_lower_bound(self, iterations, n_episodes, batch=None, sample=None, seed=0, capacity_log2=None, decks=None, root_actions=None, stream_id=0):
        """A sampled LOWER BOUND on the exploitability of the nets' average policy from ANY round-boundary root, the deal included, where no store of
        the policy fits: sampled_response(iterations, ...) is trained against the nets and played against them in
        self.match(n_episodes, opponent=response, ...).  -> match_report's dictionary from the RESPONDER's side (the seats' sums exchanged, the
        rewards negated) with "lower_bound": True: "reward" estimates what this one responder wins over both seatings -- at most (BR0 + BR1) / 2
        -- and by_seat[p]["reward"] what it wins in seat p.  The responder is a real key-pair policy, so what it wins is achieved; more
        iterations can only find a better one.  n_episodes must be even, so that both seatings have the same count (ValueError otherwise).  Where
        the sub-game fits the sweeps the exact fields are cross_play([response, policy_store()])'s, and None otherwise."""
        if int(n_episodes) % 2:
            raise ValueError("n_episodes must be even: both seatings play the same number of episodes")
        resp = self.sampled_response(iterations, batch=batch, sample=sample, seed=seed, capacity_log2=capacity_log2, decks=decks, root_actions=root_actions)
        try:
            return self.response_report(resp, n_episodes, decks=decks, root_actions=root_actions, stream_id=stream_id)
        finally:
            resp.close()

    def response_report(self, response, n_episodes, decks=None, root_actions=None, stream_id=0):
        """sampled_lower_bound's measuring half, for a response that is trained on in steps (solver.respond_nets_iterate, solver.harden) and measured
        after each: what the hardened `response` (sampled_response(decks=decks, root_actions=root_actions)) wins against the nets in
        self.match(n_episodes, opponent=response, ...), reported from the responder's side."""
        from ..full_chance import _forest_fits, cross_play, match_report
        n = int(n_episodes)
        if n % 2:
            raise ValueError("n_episodes must be even: both seatings play the same number of episodes")
        s = self.match(n, opponent=response, decks=decks, root_actions=root_actions, stream_id=stream_id)["sums"]
        sums = np.array([-s[1], -s[0], s[3], s[2], s[5], s[4]], np.int64)           # the responder sits in seat 0 where the nets sit in seat 1
        exact = None
        if _forest_fits(response.solver.root, response.decks.shape[0], 2):
            store = self.policy_store(decks, root_actions)
            try:
                exact = cross_play([response, store], decks=decks)
            finally:
                store.close()
        out = match_report(sums, n, exact)
        out["lower_bound"] = True
        return out

    def get_policy(self, state, player):
        """{action card: probability} of `player` at a FullScopaState / _lib.FullState: the snapshots evaluated at the state's key pair on the host
        (StrategyBuffer.average_policy_batch on the 96 features; uniform without snapshots)."""
        fs = getattr(state, "_fs", state)
        legal = sorted(fs.legal(player))
        if len(legal) < 2:
            return {c: 1.0 for c in legal}
        feat = key_features(np.array([_lib.full_infoset_key_wide(fs, player)], np.uint64))
        buf = self.strategy_buffers[player]
        dev = buf._store[0].device if buf._store is not None else "cpu"
        f = torch.as_tensor(feat, dtype=torch.float32, device=dev)
        p = buf.average_policy_batch(f, f[:, :ACTIONS].contiguous())[0].double().cpu().numpy()
        total = p[legal].sum()
        return {c: float(p[c] / total) if total > 0 else 1.0 / len(legal) for c in legal}

    def evaluate_vs_random(self, num_episodes=100, decks=None, root_actions=None):
        """(avg_reward, [trained scopas, random scopas]) of the average policy against uniform play: FullChanceMCCFRTrainer.evaluate_vs_random on
        policy_store(decks, root_actions), the matches starting at `root_actions`' root where one is given."""
        t = self.policy_store(decks, root_actions)
        try:
            mean, _, stats = t.evaluate_vs_random(num_episodes, decks=decks)   # (the store trainer's root is root_actions': the match starts there)
        finally:
            t.close()
        return mean, [stats["trained_avg"], stats["opponent_avg"]]

    # ---- the nets in sampled matches ---------------------------------------------------------------------------------
    def _snapshot_set(self, player):
        """(slots, six device pointers, max_size, coefficient pointer) of `player`'s snapshots as the library's average-policy calls take them, and the
        coefficient tensor to keep alive; made on the solver's stream"""
        buf = self.strategy_buffers[player]
        n = len(buf._slots)
        if not n:
            return ([], [0] * 6, 0, 0), None
        total = float(sum(buf.weights))
        with torch.cuda.stream(self._stream), torch.no_grad():
            coef = torch.tensor([w / total for w in buf.weights], dtype=torch.float32, device=self.device)   # float32(weight / total), as _average_nodes
        return (list(buf._slots), [t.data_ptr() for t in buf._store], buf.max_size, coef.data_ptr()), coef

    def average_policy_at(self, keys2, player):
        """float64 [n][3] average policy of `player`'s snapshots at the key pairs keys2 [n][2] (all of mover `player`; any deck, any round), slots in
        ascending card id, zeros beyond the held cards: scopa_full_chance_sdcfr_average_at, one launch whatever the snapshot count.  Where a pair
        lies in a sub-game the sweeps cover, the row carries policy_rows' bits."""
        keys2 = np.ascontiguousarray(keys2, np.uint64).reshape(-1, 2)
        n = len(keys2)
        if not n:
            return np.zeros((0, 3), np.float64)
        (slots, ptrs, max_size, coef_ptr), keep = self._snapshot_set(player)
        with torch.cuda.stream(self._stream), torch.no_grad():
            k = torch.tensor(keys2.view(np.int64), device=self.device)
            out = torch.empty((n, 3), dtype=torch.float64, device=self.device)
            self._ctx.full_chance_sdcfr_average_at(player, k.data_ptr(), n, slots, ptrs, max_size, coef_ptr, out.data_ptr())
        self._stream.synchronize()
        del keep
        return out.cpu().numpy()

    def match(self, n, opponent=None, decks=None, root_actions=None, stream_id=0, per_episode=False):
        """A sampled seat-swapped match of the nets' average policy from ANY round-boundary root, the deal included (scopa_full_chance_sdcfr_match):
        the first ceil(n / 2) episodes have the nets in seat 0, episode i on deck j mod k of `decks` ([k][40] that fit the root; None: the
        solver's).  opponent: None (uniform play), a FullChanceMCCFRTrainer on the solver's context (its store's average policy), or another
        FullChanceDeepCFR (its nets' average policy).  root_actions: a prefix of whole rounds played on decks[0] (None: the solver's own root).
        -> full_chance.evaluate's dictionary (reward, std_error, a_scopas, b_scopas, by_seat, sums, ...); the exact fields are filled where the
        sub-game fits the sweeps, from policy_store + cross_play, and are None otherwise -- the match is then the only measure there is.
        per_episode: -> (dictionary, the nets' reward x2 of every episode, int8 [n])."""
        from ..full_chance import _forest_fits, cross_play, match_report
        n = int(n)
        if not (opponent is None or isinstance(opponent, (FullChanceMCCFRTrainer, FullChanceDeepCFR))):
            raise ValueError("opponent must be None, a FullChanceMCCFRTrainer or a FullChanceDeepCFR")
        sets = [self._snapshot_set(p) for p in range(2)]
        opp, opp_sets = None, None
        if isinstance(opponent, FullChanceMCCFRTrainer):
            opp = opponent.solver
        elif opponent is not None:
            opp_sets = [opponent._snapshot_set(p) for p in range(2)]
            opponent._stream.synchronize()                       # its snapshots and coefficients are written on its own stream
            opp = [s[0] for s in opp_sets]
        at_root = None
        try:
            if root_actions is None:
                solver, held = self.solver, decks
            else:
                at_root = FullChanceMCCFRTrainer(decks=self.decks if decks is None else decks, root_actions=tuple(root_actions), capacity_log2=4, batch=1,
                                                 ctx=self.trainer.ctx)
                solver, held = at_root.solver, None
            got = solver.sdcfr_match(n, [s[0] for s in sets], opp, stream_id, held, per_episode=per_episode)
            sums, r2 = got if per_episode else (got, None)
            k = (self.n_decks if root_actions is None else at_root.decks.shape[0]) if decks is None else len(decks)
            exact = None
            if _forest_fits(solver.root, k, 2):
                stores = [self.policy_store(decks, root_actions)]
                try:
                    if not isinstance(opponent, FullChanceMCCFRTrainer):
                        # a second set of nets is tabulated on THIS solver's forest (its decks, its root): the rows are a function of the pair
                        rows = None if opponent is None else self.policy_rows(decks, root_actions, buffers=opponent.strategy_buffers)
                        cap = 4 if rows is None else max(4, int(np.ceil(np.log2(max(len(rows[0]), 1) * 2 + 1))))
                        stores.append(FullChanceMCCFRTrainer(decks=stores[0].decks, root_actions=stores[0].root_actions, capacity_log2=cap, batch=1,
                                                             ctx=self.trainer.ctx))            # an empty store plays uniformly
                        if rows is not None and len(rows[0]):
                            stores[1]._checked(stores[1].solver.tables_set, rows[0], rows[1], np.zeros_like(rows[2]), rows[2])
                    exact = cross_play([stores[0], stores[1] if len(stores) > 1 else opponent], decks=decks)
                finally:
                    for t in stores:
                        t.close()
        finally:
            if at_root is not None:
                at_root.close()
        del sets, opp_sets
        out = match_report(sums, n, exact)
        return (out, r2) if per_episode else out

    # ---- training loop ----------------------------------------------------------------------------------------------
    def train(self, iterations=100, advantage_epochs=10, exploitability_freq=None, verbose=False, resume=False, train_batch=128):
        """DeepCFR.train's loop (the host one iteration ahead of the device, snapshots from the call's second iteration on, weight = loop index + 1)
        without the matches against a random player.  resume=True: the loop index goes on from the solver's running iteration count instead of
        starting at 0, so a run cut into several train() calls takes the snapshots, with the weights, of one long call (without it every call's
        first iteration takes none, as the reference's loop variable has it).  train_batch: rows of an optimiser step's batch.
        exploitability_freq=k: at every iteration i of this call with i % k == 0 the queue is drained and (absolute iteration, exploitability)
        appended to training_history["exploitability"]."""
        if exploitability_freq is not None and (int(exploitability_freq) != exploitability_freq or exploitability_freq < 1):
            raise ValueError("exploitability_freq must be None or a positive integer")
        ahead = None
        for iteration in range(iterations):
            queued = self._queue_iteration(advantage_epochs, train_batch, loop_index=self._iteration if resume else iteration)
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
