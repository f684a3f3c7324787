/*
 * scopa.h -- C ABI of libscopa_hip.so, the MI355X (gfx950) MiniScopa CFR traversal engine.
 *
 * The reference (rug-marl-group2/scopa) has no FFI: its boundary is a Python object protocol.
 * Each entry point below therefore cites the reference Python interface it stands behind
 * (paths relative to the reference repo root); INTEGRATION.md shows the ctypes binding a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - plain C, every function returns int32 status: 0 = SCOPA_OK, negative = SCOPA_E*.
 *     No exception or abort crosses the boundary; scopa_last_error(ctx) gives the detail string.
 *   - opaque scopa_ctx: one context <-> one HIP device + one HIP stream (+ one deal / tree / table set).
 *     A context is not thread-safe; distinct contexts are independent.
 *   - bulk buffers are caller-owned and only borrowed for the duration of the call.  Arguments named
 *     d_* are DEVICE pointers (e.g. torch.Tensor.data_ptr()), h_* are host pointers.
 *   - solver entry points need a GPU: scopa_ctx_create fails with SCOPA_ENODEV when there is none.
 *     There is no CPU fallback.  The scopa_state_* / scopa_deal_* helpers are host-side glue for the
 *     single-state object protocol (State.apply_action etc.) and need no context.
 */
#ifndef SCOPA_H
#define SCOPA_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCOPA_ABI_VERSION 1

enum {
    SCOPA_OK = 0,
    SCOPA_EINVAL = -1,   /* bad argument                                   */
    SCOPA_ENODEV = -2,   /* no usable HIP device                           */
    SCOPA_EHIP = -3,     /* a HIP runtime call failed (see last_error)     */
    SCOPA_ESTATE = -4,   /* call order violated (e.g. no deal set)         */
    SCOPA_ENOMEM = -5,
    SCOPA_ELIMIT = -6,   /* problem exceeds a compiled-in capacity         */
    SCOPA_ETIMEOUT = -7  /* a peer did not answer within the wait budget (N > 1 exchange): tables are not to be trusted */
};

/* Deal-independent shape of MiniScopa (src/envs/mini_scopa_game.py:59,127): 2 players x 4 cards,
 * 8 plies, legal-count profile 4,4,3,3,2,2,1,1. */
#define SCOPA_N_CARDS 16
#define SCOPA_N_PLIES 8
#define SCOPA_N_DECISION 1653
#define SCOPA_N_TERMINAL 576
#define SCOPA_N_NODES 2229
#define SCOPA_MAX_ACTIONS 4

/* Packed game state, 16 bytes, the unit the kernels keep in HBM.  Hands and table are ORDERED lists of
 * 4-bit card ids (card id = action id = suit*4 + rank_idx, mini_scopa_game.py:17-23,149-153); list order
 * is part of the infoset identity (openspiel_mini_scopa.py:86-95).  Unused nibbles are zero.
 * to_move = step & 1; terminal iff (nh[0]==0 && nh[1]==0) || step_count >= max_steps (mini_scopa_game.py:160), where
 * step_count = step & SCOPA_STEP_COUNT_MASK and max_steps = 8 (a fresh env, mini_scopa_game.py:127), or 16 when
 * SCOPA_STEP_CLONED is set: the env of a MiniScopaState.clone() (openspiel_mini_scopa.py:108).  Only illegal no-op actions make
 * the two differ; scopa_state_clone() sets the bit, every other entry point preserves it. */
#define SCOPA_STEP_CLONED 0x80u
#define SCOPA_STEP_COUNT_MASK 0x7Fu
typedef struct scopa_state {
    uint16_t hand[2];   /* nibble i = i-th card of the hand                  */
    uint32_t table;     /* nibble i = i-th card on the table                 */
    uint8_t  nh[2];     /* cards in hand                                     */
    uint8_t  nt;        /* cards on table                                    */
    uint8_t  step;      /* MiniScopaEnv.step_count | SCOPA_STEP_CLONED       */
    uint8_t  ncap[2];   /* len(player.captures)                              */
    uint8_t  scopas[2]; /* player.scopas                                     */
} scopa_state;

typedef struct scopa_ctx scopa_ctx;

int32_t     scopa_abi_version(void);
const char *scopa_strerror(int32_t status);
const char *scopa_last_error(const scopa_ctx *ctx);

/* device_id >= 0.  hip_stream: a hipStream_t to launch on (e.g. torch.cuda.current_stream().cuda_stream),
 * or NULL to let the context create its own. */
int32_t scopa_ctx_create(int32_t device_id, void *hip_stream, scopa_ctx **out);
int32_t scopa_ctx_destroy(scopa_ctx *ctx);
int32_t scopa_ctx_synchronize(scopa_ctx *ctx);

/* ---- host-side single-state protocol (no context, no device) ------------------------------------------
 * stands behind MiniScopaState / MiniScopaEnv: src/envs/openspiel_mini_scopa.py:17-115,
 * src/envs/mini_scopa_game.py:117-194 */
int32_t scopa_deal_py_seed(int64_t seed, uint8_t perm16[16]);              /* MiniDeck.__init__ :25-28        */
int32_t scopa_state_init(const uint8_t perm16[16], scopa_state *out);      /* MiniScopaGame.reset :56-64      */
int32_t scopa_state_step(scopa_state *s, int32_t action);                  /* MiniScopaEnv.step :140-167      */
int32_t scopa_state_clone(const scopa_state *s, scopa_state *out);         /* MiniScopaState.clone, openspiel_mini_scopa.py:97-115: a copy whose max_steps is 16 (:108) */
int32_t scopa_state_is_terminal(const scopa_state *s);                     /* 0/1                             */
int32_t scopa_state_current_player(const scopa_state *s);                  /* 0/1, -4 at terminal             */
int32_t scopa_state_legal(const scopa_state *s, int32_t player /* <0 = current */, int32_t out[4], int32_t *n);
int32_t scopa_state_rewards_x2(const scopa_state *s, int32_t r2[2]);       /* evaluate_game :106-114, x2      */
int32_t scopa_state_infoset_key(const scopa_state *s, int32_t player, uint64_t *key);
int32_t scopa_key_to_string(uint64_t key, char *buf, int32_t cap);         /* information_state_string :86-95 */
int32_t scopa_state_infoset_string(const scopa_state *s, int32_t player, char *buf, int32_t cap);

/* ---- batched game step (HIP kernel) --------------------------------------------------------------------
 * d_states[i] <- step(d_states[i], d_actions[i]); same semantics as scopa_state_step incl. the silent no-op. */
int32_t scopa_step_batch(scopa_ctx *ctx, scopa_state *d_states, const uint8_t *d_actions, int64_t n);
/* convenience for host buffers: H2D, kernel, D2H on the context's stream, synchronous */
int32_t scopa_step_batch_host(scopa_ctx *ctx, scopa_state *h_states, const uint8_t *h_actions, int64_t n);

/* ---- deal + game tree (built ON DEVICE by level-synchronous expansion with the step kernel) ------------
 * stands behind game.new_initial_state() + the clone()/apply_action() recursion of every solver.
 * scopa_set_deal drops everything derived from the previous deal: a caller-bound delta buffer, captured MCCFR graphs, the exact-CFR schedule, the
 * SDCFR node bits and policy table, prepared evaluation thresholds.  State getters after it, before any new launch: scopa_mccfr_iteration_counter
 * gives 0, scopa_visited_get zeros, the tables their reset state, scopa_cfr_exact_last_route -1; scopa_sdcfr_policy_get and scopa_eval_tabular_match
 * refuse with SCOPA_ESTATE.  scopa_counters and scopa_sdcfr_visits count since the context was created and are NOT reset: take differences. */
int32_t scopa_set_deal(scopa_ctx *ctx, const uint8_t perm16[16]);          /* builds tree, zeroes tables      */
int32_t scopa_tree_counts(scopa_ctx *ctx, int32_t *n_nodes, int32_t *n_decision, int32_t *n_infosets);
/* Export in REFERENCE DFS ORDER (the order vanilla_cfr.py:79-85 visits nodes); any pointer may be NULL.
 * h_states[n_nodes], h_infoset[n_nodes] (-1 at terminals; ids in first-visit order = dict insertion order),
 * h_r2[n_nodes][2], h_infoset_key[n_infosets], h_infoset_nlegal[n_infosets], h_infoset_legal[n_infosets][4] */
int32_t scopa_tree_export(scopa_ctx *ctx, scopa_state *h_states, int32_t *h_infoset, int8_t *h_r2,
                          uint64_t *h_infoset_key, int8_t *h_infoset_nlegal, int8_t *h_infoset_legal);

/* ---- tables: [n_infosets][4] float64, rows padded with 0; any pointer may be NULL ----------------------
 * stands behind CFRTrainer.info_set_map / MCCFRTrainer.info_sets (InfoNode.regret_sum, .strategy_sum,
 * .local_strategy): src/algorithms/vanilla_cfr.py:8-39,47-54, src/algorithms/mc_cfr.py:9-35 */
int32_t scopa_tables_reset(scopa_ctx *ctx);
int32_t scopa_tables_get(scopa_ctx *ctx, double *h_regret, double *h_strategy, double *h_local);
int32_t scopa_tables_set(scopa_ctx *ctx, const double *h_regret, const double *h_strategy, const double *h_local);

/* First-visit order of every infoset, h_seq[n_infosets]: 0 = never visited by any solver since the last reset,
 * otherwise a strictly increasing sequence number (sequential solvers) or 0x40000000 + id (first seen by a batched
 * launch).  Mirrors which keys the reference's dicts hold, and in which insertion order
 * (CFRTrainer._get_or_create_node vanilla_cfr.py:51-54, MCCFRTrainer._get_node mc_cfr.py:32-35). */
int32_t scopa_visited_get(scopa_ctx *ctx, uint32_t *h_seq);

/* ---- vanilla CFR, exact sequential semantics (CFRTrainer._cfr_recursive / .train, vanilla_cfr.py:56-110)
 * n_iters iterations of "for i in (0,1): traverse(root, i, 1.0, 1.0)"; h_root_values[n_iters][2] or NULL.
 * Reproduces the reference bit-for-bit, incl. the mid-traversal local_strategy refresh (:97). */
int32_t scopa_cfr_exact_iterate(scopa_ctx *ctx, int32_t n_iters, double *h_root_values);
/* one traversal: CFRTrainer._cfr_recursive(new_initial_state(), player, 1.0, 1.0) -> value */
int32_t scopa_cfr_exact_traverse(scopa_ctx *ctx, int32_t traverser, double *h_value);
/* whole-tree traversals run as a schedule of ~75 parallel steps (same per-infoset visit order, bit-identical tables); 1 forces the
 * one-lane sequential walk, the form the schedule is checked against */
int32_t scopa_cfr_exact_mode(scopa_ctx *ctx, int32_t sequential);
/* Which kernel the last exact-CFR call of this context ran (read-only): 0 the scheduled form, 1 the one-lane walk with the tables in LDS,
 * 2 the one-lane walk with the tables in HBM (they do not fit beside the maps), -1 none yet on the deal at hand (scopa_set_deal returns it to -1:
 * the route depends on the deal's sizes). */
int32_t scopa_cfr_exact_last_route(scopa_ctx *ctx, int32_t *route);
/* CFRTrainer._cfr_recursive(state, player, reach_p0, reach_p1) for any state of the tree: the state reached from the
 * root by legal-action INDICES path[0..depth) (index into legal_actions(), i.e. hand position) */
int32_t scopa_cfr_exact_traverse_from(scopa_ctx *ctx, int32_t traverser, int32_t depth, const int32_t *path,
                                      double reach_p0, double reach_p1, double *h_value);

/* ---- synchronous CFR (build-defined): sigma = regret-match(regret) frozen per iteration, both players updated from
 * one level-parallel sweep.  Not the reference's visit-order-dependent algorithm: same fixed point, different trajectory. */
int32_t scopa_cfr_sync_iterate(scopa_ctx *ctx, int32_t n_iters);
/* the same sweep with per-iteration weights h_w[n_iters][3] = (pos, neg, strat), each finite and in [0, 1]: after iteration t's increments every
 * touched cell becomes  R <- R + dR;  R <- !(R <= 0) ? R * pos : R * neg;  S <- (S + dS) * strat.  (1, 1, 1) is scopa_cfr_sync_iterate bit for bit;
 * (1, 0, t/(t+1)) is CFR+, (t/(t+1)) x 3 Linear CFR, (t^a/(t^a+1), t^b/(t^b+1), (t/(t+1))^g) DCFR(a, b, g).  The weights are the caller's data and
 * the caller owns t: the library computes no schedule and keeps no iteration count.  alternating = 1: two sweeps per iteration, sweep p updates
 * player p's rows only from sigma of the current regrets (player 0 first); counters count each sweep.  n_iters <= 1 << 20; 0 is a no-op. */
int32_t scopa_cfr_sync_iterate_weighted(scopa_ctx *ctx, int32_t n_iters, const double *h_w /*[n_iters][3]*/, int32_t alternating);

/* ---- MCCFR replay: MCCFRTrainer.iteration() (mc_cfr.py:37-92) driven by a host-supplied uniform stream
 * (one float64 per decision visit in DFS order = what np.random.choice draws); bit-exact vs the reference. */
int32_t scopa_mccfr_replay(scopa_ctx *ctx, int32_t n_iters, const double *h_uniforms, int64_t n_uniforms,
                           int64_t *consumed);

/* ---- batched external-sampling MCCFR (the throughput path) ----------------------------------------------
 * `batch` traversals per traverser per iteration against tables frozen for the iteration; random draws from
 * Philox4x32-10 keyed by (seed; recursion-path code, global traversal id, iteration, traverser), so results do
 * not depend on how traversals are split over launches or GPUs. */
int32_t scopa_mccfr_seed(scopa_ctx *ctx, uint64_t seed);
/* n_iters x { traverse [0,batch) ; apply } on this device */
int32_t scopa_mccfr_iterate(scopa_ctx *ctx, uint32_t batch, uint32_t n_iters);
/* multi-GPU building blocks: accumulate the deltas of global traversal ids [b0, b0+nb) of `iteration` ... */
int32_t scopa_mccfr_traverse(scopa_ctx *ctx, uint32_t iteration, uint32_t b0, uint32_t nb);
/* ... expose the delta buffer ([n_infosets][5] float64: 4 regret deltas + traverser-visit count) for one
 * sum-all-reduce (RCCL via torch.distributed) ... */
int32_t scopa_mccfr_delta_buffer(scopa_ctx *ctx, void **d_delta, size_t *bytes);
/* ... or bind a CALLER-OWNED device buffer of at least n_infosets*5 float64 (e.g. a torch tensor handed to
 * torch.distributed.all_reduce) as the delta buffer; it is zeroed here.  d_buf = NULL returns to the internal one.
 * The binding lasts until the next scopa_set_deal / scopa_mccfr_bind_delta. */
int32_t scopa_mccfr_bind_delta(scopa_ctx *ctx, void *d_buf, size_t bytes);
/* host copy of the delta buffer, h_delta[n_infosets][5] (tests, non-RCCL transports) and its inverse */
int32_t scopa_mccfr_delta_get(scopa_ctx *ctx, double *h_delta);
int32_t scopa_mccfr_delta_set(scopa_ctx *ctx, const double *h_delta);
/* ... then regret += delta[:, :4]; strategy += count * sigma; delta <- 0; iteration counter += 1 */
int32_t scopa_mccfr_apply(scopa_ctx *ctx);
int32_t scopa_mccfr_iteration_counter(scopa_ctx *ctx, uint32_t *iteration);
/* Graph mode of scopa_mccfr_iterate: on = chunks of up to 64 iterations are replayed as ONE captured HIP graph of (traverse, apply)
 * launches each (captured once per (batch, chunk length) and deal), the iteration number read from a device word that the apply
 * launch advances -- the same iteration ids, hence the same draws and results, as the eager loop.  Off by default (measured:
 * DESIGN.md section 4). */
int32_t scopa_mccfr_graph_mode(scopa_ctx *ctx, int32_t on);
/* Test hook: treat the device as offering only `bytes` of LDS per workgroup (0 = its real limit again), so that the launch
 * geometries only deals with very many infosets reach -- narrow traversal workgroups -- run on any deal.  Results do not change. */
int32_t scopa_debug_lds_limit(scopa_ctx *ctx, int32_t bytes);

/* ---- SDCFR: level-synchronous external-sampling traversal (DeepCFR._external_sampling_cfr, deep_cfr.py:284-365) ---------
 * B traversals of one traverser advance ply by ply; the advantage MLP runs in PyTorch between the two calls of a ply.
 * Frontier slot s of ply d refers to tree node d_idx[s] (index within the ply); a traversal owns `width` consecutive slots
 * (scopa_sdcfr_frontier_width: 1,4,4,12,12,24,24,24,24 for traverser 0; 1,1,4,4,12,12,24,24,24 for traverser 1).
 *   features : DeepCFR._state_to_features + ._get_legal_actions_mask (:213-282) -> d_feats[n][34], d_mask[n][16] float32
 *   expand   : positive_regret_policy (nets.py:93-101) of d_adv[n][16] (raw net output); traverser ply -> all legal
 *              children d_child_idx[n*nlegal] (hand order), opponent ply -> ONE sampled child d_child_idx[n]
 *              (np.random.choice arithmetic; draws from d_uniforms[n] if given, else Philox keyed by the global
 *              traversal id b0 + s/width); d_pol[n][4] = policy of the legal actions in hand order
 *   terminal_values : float(rewards[player]) at ply 8
 *   backward : traverser ply: value = sum pol*child value (float32, hand order), regrets = cfv - value over all 16 slots
 *              (illegal slots = -value, as the reference), divided by max|.|+1e-8, and the memory row (feats, regrets, mask)
 *              written to ring position (write_base + traversal*41 + DFS-post-order rank) % capacity, i.e. in the
 *              reference's append order (AdvantageNetwork.add_experience :70-75); opponent ply: value = child's value */
int32_t scopa_sdcfr_frontier_width(int32_t traverser, int32_t ply);
int32_t scopa_sdcfr_features(scopa_ctx *ctx, int32_t ply, int64_t n, const int32_t *d_idx, float *d_feats, float *d_mask);
int32_t scopa_sdcfr_expand(scopa_ctx *ctx, int32_t ply, int32_t traverser, int64_t n, const int32_t *d_idx, const float *d_adv,
                           int32_t *d_child_idx, float *d_pol, const double *d_uniforms, uint32_t iteration, uint32_t b0);
int32_t scopa_sdcfr_terminal_values(scopa_ctx *ctx, int32_t traverser, int64_t n, const int32_t *d_idx, float *d_val);
int32_t scopa_sdcfr_backward(scopa_ctx *ctx, int32_t ply, int32_t traverser, int64_t n, const int32_t *d_idx, const float *d_pol,
                             const float *d_child_val, float *d_val, const float *d_feats, const float *d_mask, float *d_mem_feat,
                             float *d_mem_regret, float *d_mem_mask, int64_t capacity, int64_t write_base);
int32_t scopa_sdcfr_visits(scopa_ctx *ctx, uint64_t *decision_visits);   /* counted on the host as traversals are launched: no wait */
/* Read-only, for tests: the policy table the last default-mode scopa_sdcfr_traverse_fused launch computed (k_sdcfr_policy), decision nodes in level
 * order (ply d, then j; the children of node j are j * nlegal + i).  h_policy [1653][4] float: the regret-matching policy, legal actions in hand
 * order, zeros beyond; h_thr [1653][3] uint64: the node's sampling thresholds -- action = #{k : h_thr[k] <= N} for a draw u = N * 2^-53, where
 * h_thr[k] = ceil(cdf_k / cdf_last * 2^53) for k < nlegal - 1 and 2^53 beyond, and h_thr[0] = ~0 marks a node whose policy sums to 0 (uniform
 * choice).  Either pointer may be NULL.  Synchronises the context's stream.  SCOPA_ESTATE before the first such launch, and again after every scopa_set_deal until the
 * first such launch on the new deal: the previous deal's table is never handed out as current. */
int32_t scopa_sdcfr_policy_get(scopa_ctx *ctx, float *h_policy, uint64_t *h_thr);
/* The same traversal as ONE launch: a wavefront walks four traversals together, both players' advantage MLPs (34-128-64-16
 * float32) resident in LDS and evaluated in-kernel on the matrix cores, sixteen frontier nodes per tile.
 * d_image[2][SCOPA_SDCFR_IMAGE_FLOATS]: per player the net as scopa_sdcfr_pack_weights lays it out (the operand layout of
 * v_mfma_f32_16x16x4_f32; the kernel copies it to LDS as it is).  d_uniforms (optional, tests): [batch][8][24] float64 draws
 * indexed (traversal, ply, slot).  d_mem_feat must be 8-byte, d_mem_regret / d_mem_mask 16-byte aligned.
 * d_mem_mask may be NULL (here and in scopa_sdcfr_backward): a traverser node's legal actions are the cards of the mover's hand
 * (openspiel_mini_scopa.py:36-45) and features[0..16) are that hand's one-hot (deep_cfr.py:213-275), so the mask row equals the first
 * sixteen floats of the feature row and need not be written a second time -- a memory row is then 200 bytes of HBM instead of 264.
 * Samples the same actions as the ply-by-ply path (same Philox keying); float32 sums run in a different order. */
#define SCOPA_SDCFR_IMAGE_FLOATS 13520
int32_t scopa_sdcfr_image_floats(void);
/* One advantage net (AdvantageNetwork.net = FlexibleNet(mode="mlp"), nets.py:296-331; torch tensors, row-major W[out][in]:
 * backbone.0.fc.weight [128][34] / .bias [128], backbone.1.fc.weight [64][128] / .bias [64], head.weight [16][64] / .bias [16],
 * all float32 device pointers) -> player's half of d_image.  One small launch on the context's stream; call it again
 * whenever the net changed (an optimiser step, load_state_dict). */
int32_t scopa_sdcfr_pack_weights(scopa_ctx *ctx, int32_t player, const float *d_w1, const float *d_b1, const float *d_w2,
                                 const float *d_b2, const float *d_w3, const float *d_b3, float *d_image);
int32_t scopa_sdcfr_traverse_fused(scopa_ctx *ctx, int32_t traverser, int32_t batch, const float *d_image, float *d_mem_feat,
                                   float *d_mem_regret, float *d_mem_mask, int64_t capacity, int64_t write_base,
                                   float *d_root_values, const double *d_uniforms, uint32_t iteration, uint32_t b0);
/* How scopa_sdcfr_traverse_fused evaluates the advantage nets.  0 (default): ONCE per decision node of the deal and launch -- the nets
 * are frozen while a launch runs and a node's features depend on the tree node alone, so its 1 653 policies are computed by one
 * small launch on the matrix cores and the traversals walk that table (two launches; the memory rows bound it).  1: a forward pass
 * per visit inside the traversal kernel (one launch; the form for batches that would not share a deal; also what d_uniforms takes).
 * Same rows, same values, same sampled actions either way. */
int32_t scopa_sdcfr_mode(scopa_ctx *ctx, int32_t forward_per_visit);
/* Kept for callers of earlier versions: accepts only (0, 0), the library's one task shape (one traversal per wavefront in the walk
 * kernel, four per wavefront in the forward-per-visit kernel).  The other shapes it used to select -- more traversals per wavefront,
 * teams of wavefronts sharing a task -- measured no faster and are retired: anything else is SCOPA_EINVAL. */
int32_t scopa_sdcfr_tuning(scopa_ctx *ctx, int32_t traversals_per_task, int32_t wavefronts_per_task);
/* One optimiser step of an advantage net WITHOUT PyTorch kernels (AdvantageNetwork.train, deep_cfr.py:99-112): gather the n_rows ring rows d_rows[],
 * forward 34-128-64-16, MSE(pred * mask, target * mask) over n_rows x 16, backward, clip_grad_norm_(1.0), Adam(lr, betas 0.9 / 0.999, eps 1e-8).
 * OPT-IN (the default trains with PyTorch-ROCm): DeepCFR(train_backend="hip").  d_w1 .. d_b3 are the net's own tensors (torch layout W[out][in]),
 * updated in place; d_state = [2][13776] float (exp_avg, exp_avg_sq in net.parameters() order), zero before the first step; step = 1, 2, ...;
 * the step's loss is ADDED to d_loss[0].  n_rows: a multiple of 16.  d_mask NULL = every row's mask is its features[0..16) (rows written by the
 * traversal calls with d_mem_mask NULL).  Two launches (k_sdcfr_train_grad, k_sdcfr_train_adam), no host synchronisation. */
int32_t scopa_sdcfr_train_params(void);   /* 13 776 */
/* n_steps consecutive steps in one call: step e trains on d_rows[e * n_rows .. (e + 1) * n_rows) with step number first_step + e (the epochs of one train() call) */
int32_t scopa_sdcfr_train_steps(scopa_ctx *ctx, const int64_t *d_rows, int32_t n_rows, int32_t n_steps, const float *d_feat, const float *d_regret, const float *d_mask,
                                int64_t capacity, float *d_w1, float *d_b1, float *d_w2, float *d_b2, float *d_w3, float *d_b3, float *d_state,
                                int32_t first_step, float lr, float *d_loss);
int32_t scopa_sdcfr_train_step(scopa_ctx *ctx, const int64_t *d_rows, int32_t n_rows, const float *d_feat, const float *d_regret, const float *d_mask,
                               int64_t capacity, float *d_w1, float *d_b1, float *d_w2, float *d_b2, float *d_w3, float *d_b3, float *d_state,
                               int32_t step, float lr, float *d_loss);
/* The same step for FullScopa's 96-128-64-40 net (FullChanceDeepCFR(train_backend="hip"); scopa_full_train.hip): loss over n_rows x 40, d_feat [capacity][96],
 * d_regret and d_mask [capacity][40], d_mask NULL = every row's mask is its features[0..40); d_w3 is [40][64] and d_b3 [40] (nothing beyond is read);
 * d_state = [2][23272] float.  scopa_sdcfr_train_steps' contract: n_rows a multiple of 16 in 16 .. 2^20, n_steps in 0 .. 4096, first_step >= 1, lr > 0,
 * capacity >= 1, d_w1 / d_w2 / d_w3 16-byte aligned -- anything else is SCOPA_EINVAL before any device work; row indices outside [0, capacity) are clamped.
 * Three launches per step on the context's stream (k_full_train_grad, k_full_train_reduce, k_full_train_adam), no host synchronisation; sums in a fixed
 * order (no float atomics): the same state and rows give the same bits.  The step's loss is ADDED to d_loss[0]. */
int32_t scopa_full_sdcfr_train_params(void);   /* 23 272 */
int32_t scopa_full_sdcfr_train_steps(scopa_ctx *ctx, const int64_t *d_rows, int32_t n_rows, int32_t n_steps, const float *d_feat /* [capacity][96] */,
                                     const float *d_regret /* [capacity][40] */, const float *d_mask /* [capacity][40] or NULL */, int64_t capacity, float *d_w1, float *d_b1,
                                     float *d_w2, float *d_b2, float *d_w3, float *d_b3, float *d_state /* [2][23272] */, int32_t first_step, float lr, float *d_loss);
/* The SDCFR average policy as a tabular policy (StrategyBuffer.get_average_policy, deep_cfr.py:137-160): at every decision node of `player`,
 * sum over the snapshots s = 0 .. n_snap - 1 in FIFO order of positive_regret_policy(net_s(features), mask) * d_coef[s] (nets.py:93-101: an
 * all-zero row when no advantage is positive), float32; then normalised over the legal actions in float64, uniform where that sum is 0 or not
 * finite (evaluate_vs_random, deep_cfr.py:391-397), and written to d_policy[infoset][4] (float64, hand order, zeros beyond nlegal).  The features
 * depend on the mover's hand and the table alone, so the value is one per infoset.  Rows of the other player's infosets are left untouched;
 * n_snap = 0 writes the uniform policy.  The StrategyBuffer store: d_w1 [max_size][128][34], d_b1 [max_size][128], d_w2 [max_size][64][128],
 * d_b2 [max_size][64], d_w3 [max_size][16][64], d_b3 [max_size][16] (float32, torch layout W[out][in]; all but d_w1 16-byte aligned); d_slots[s]
 * = the store slot of snapshot s (a slot outside [0, max_size) is not read: its term is NaN and the rows it reaches go uniform); d_coef[s] =
 * float32(weight_s / sum of weights).  Two launches on the context's stream, no host synchronisation; bit-identical from run to run.  The
 * exploitability of the table is scopa_exploitability(ctx, h_policy, ...) after a copy to the host. */
int32_t scopa_sdcfr_average_policy(scopa_ctx *ctx, int32_t player, int32_t n_snap, const float *d_w1, const float *d_b1, const float *d_w2,
                                   const float *d_b2, const float *d_w3, const float *d_b3, int32_t max_size, const int32_t *d_slots,
                                   const float *d_coef, double *d_policy);
/* features / masks of arbitrary device-resident states for the player to move (DeepCFR.get_policy, :497-504) */
int32_t scopa_features_from_states(scopa_ctx *ctx, const scopa_state *d_states, int64_t n, float *d_feats, float *d_mask);
/* batched evaluation episodes (evaluate_vs_random :367-429; evaluate_agent vanilla_cfr.py:157-216): n copies of the deal's
 * root state; one ply of play: the seat d_trained_seat[i] samples from d_probs[i][16] over the cards of its hand, in hand order,
 * the other seat (both seats when d_probs is NULL) plays uniformly at random; finished episodes are left untouched.
 * The reference's fallback (deep_cfr.py:394-397): the trained seat plays UNIFORM when any of its legal slots holds a NaN -- whatever
 * the other slots hold -- or when the legal slots' sum is not > 0; slots of cards not in hand are never read.  A negative entry is
 * outside the reference's domain (np.random.choice raises on it): it counts as 0 before the sum.  +-inf entries are not supported.
 * The action is the first q with u < c_q, c_q the running float64 sum of w_q / total in hand order (the last action if none), with
 * u = u53 of Philox counter (i, i >> 32, ply_tag, stream_id) under the key set by scopa_mccfr_seed. */
int32_t scopa_eval_init_states(scopa_ctx *ctx, scopa_state *d_states, int64_t n);
int32_t scopa_eval_step(scopa_ctx *ctx, scopa_state *d_states, int64_t n, const float *d_probs, const int32_t *d_trained_seat,
                        uint32_t stream_id, uint32_t ply_tag);

/* one ply of n lockstep evaluation episodes of a TABULAR policy d_policy[n_infosets][4] (float64, hand order) vs uniform
 * random: evaluate_agent (vanilla_cfr.py:157-216).  d_node_idx[n] tracks each episode's tree node (start at 0). */
/* the sampling thresholds of a tabular policy ([n_infosets][4] float64, device), computed once per evaluation: scopa_eval_tabular_step with d_policy = NULL then
 * samples the trained seat by integer compares against them -- the same actions, bit for bit, as the float64 divisions of np.random.choice it performs when
 * given the policy itself.  Invalidated by scopa_set_deal. */
int32_t scopa_eval_tabular_prepare(scopa_ctx *ctx, const double *d_policy);
int32_t scopa_eval_tabular_step(scopa_ctx *ctx, scopa_state *d_states, int32_t *d_node_idx, int64_t n, int32_t ply,
                                const double *d_policy, const int32_t *d_trained_seat, uint32_t stream_id);
/* the whole match of the PREPARED tabular policy vs uniform random in one launch (evaluate_agent's loop, vanilla_cfr.py:173-216): episodes i < n_seat0 have the
 * policy in seat 0, the rest in seat 1; the same Philox draws and thresholds as eight scopa_eval_tabular_step calls, hence the same episodes bit for bit, walked
 * as node indices of the deal's tree with no per-ply state traffic.  h_stats[seat][5] = episodes, sum of the trained side's rewards x2, sum of their squares,
 * sum of its scopas, sum of the opponent's (integers: every reward is a multiple of 0.5).  d_states_out[n] / d_node_idx_out[n]: the final states / terminal
 * indices as the per-ply form leaves them, or NULL.  Synchronous. */
int32_t scopa_eval_tabular_match(scopa_ctx *ctx, int64_t n, int64_t n_seat0, uint32_t stream_id, scopa_state *d_states_out, int32_t *d_node_idx_out,
                                 int64_t h_stats[10]);

/* ---- policy value / exploitability (build-defined; the reference only calls OpenSpiel's, vanilla_cfr.py:112-118) --
 * h_policy[n_infosets][4] or NULL = the average policy of the strategy table (InfoNode.policy, vanilla_cfr.py:32-39).
 * h_out4 = {exploitability = (BR0+BR1)/2, BR0, BR1, value of the policy for player 0}; h_policy_out (optional)
 * receives the policy that was evaluated. */
int32_t scopa_exploitability(scopa_ctx *ctx, const double *h_policy, double *h_out4, double *h_policy_out);

/* ---- policy against policy (build-defined; the host counterpart is algorithms.evaluation.head_to_head) -------------------------------
 * Tabular policies are [n_infosets][4] float64 DEVICE tables in hand order, n_pol of them back to back, used as given: rows are not normalised
 * and a non-finite entry propagates by IEEE rules.  n_pol outside [1, 256] or a NULL pointer (d_br excepted): SCOPA_EINVAL; no deal set:
 * SCOPA_ESTATE; tables that do not fit the LDS limit: SCOPA_ELIMIT (reachable through scopa_debug_lds_limit only).  Both calls launch on the
 * context's stream and do not synchronise; every float64 sum runs in a fixed order, so results are bit-identical from run to run.
 *
 * cross_play: d_out[a][b] = { E[reward of seat 0], E[reward of seat 0 squared], E[scopas of seat 0], E[scopas of seat 1] } of policy a in seat 0
 * against policy b in seat 1, exactly: one launch, one workgroup per ordered pair, eight bottom-up levels `v = 0.0; v += row[c] * child[c]`
 * (children left to right) over the terminals' 0.5 * p0, 0.25 * p0 * p0 and scopa counts.  d_out[a][a][0] is the policy value scopa_exploitability
 * reports, bit for bit.  LDS: 32 * n_infosets + 36 864 + 3 312 bytes -- 63 792 at 738 infosets, 93 072 at the 1 653 maximum -- so it fits
 * every deal, and under scopa_debug_lds_limit(64 KiB) it still runs, with the same bits, on deals of up to 792 infosets. */
int32_t scopa_cross_play(scopa_ctx *ctx, int32_t n_pol, const double *d_policies /*[n_pol][n_infosets][4]*/, double *d_out /*[n_pol][n_pol][4]*/);
/* best_response: one workgroup per (policy, responder), the procedure and summation order of scopa_exploitability (per (infoset, action) the ply's
 * nodes added in ascending order from 0.0; ties to the lowest action), plus a small launch for the mean.  d_out4[k] = {(BR0 + BR1) / 2, BR0, BR1,
 * value}, bit for bit what scopa_exploitability(ctx, policy k, ...) returns.  d_br (or NULL): d_br[k][p] is a complete policy table -- player p's
 * rows one-hot at the chosen action, the other player's rows policy k's -- fit to go back into scopa_cross_play or a match.  LDS as
 * scopa_exploitability: 68 * n_infosets + 35 664 + 3 312 bytes (89 160 at 738 infosets: SCOPA_ELIMIT under a 64 KiB limit). */
int32_t scopa_best_response(scopa_ctx *ctx, int32_t n_pol, const double *d_policies /*[n_pol][n_infosets][4]*/, double *d_br /*[n_pol][2][n_infosets][4] or NULL*/,
                            double *d_out4 /*[n_pol][4]*/);
/* The seat-swapped match of scopa_eval_tabular_match with a policy in BOTH seats: episodes i < n_seat0 have policy a in seat 0 and b in seat 1, the rest
 * the other way round.  Thresholds of both tables by scopa_eval_tabular_prepare's formula, in a buffer of this call's own (a prepared table is not
 * disturbed); the same Philox keying (episode, ply, stream_id; context seed) and, for every ply, the integer compares the trained seat uses there.
 * h_stats[seat half][5] as there, from a's point of view: episodes, sum of a's rewards x2, sum of their squares, sum of a's scopas, sum of b's.
 * d_node_idx_out[n] (or NULL): every episode's terminal index.  Synchronous. */
int32_t scopa_eval_pair_match(scopa_ctx *ctx, const double *d_policy_a, const double *d_policy_b, int64_t n, int64_t n_seat0, uint32_t stream_id,
                              int32_t *d_node_idx_out, int64_t h_stats[10]);

/* ---- many deals at once ("replicas": one workgroup per independent solve) -------------------------------------------------
 * The reference solves one deal (seed 42) but its env takes a seed (MiniScopaEnv(seed=...), mini_scopa_game.py:120-132).
 * A scopa_multi keeps n deals resident in HBM and runs the per-deal kernels with one workgroup per deal.
 *   deal_py_seeds : MiniDeck(seed) for every deal ON DEVICE (CPython seed + shuffle, one lane per deal)
 *   build         : game trees + zeroed tables; h_n_infosets[n] (optional) receives the infoset counts.  A second build (after new deals) starts the
 *                   handle over: tables, first-visit marks, the MCCFR iteration number and scopa_multi_counters are those of a fresh handle
 *   cfr_exact / cfr_sync_iterate, exploitability (h_out4[n][4]) : as the single-deal entry points, per deal
 *   tables_get    : [n_infosets(deal)][4] tables and keys of one deal */
typedef struct scopa_multi scopa_multi;
int32_t scopa_multi_create(scopa_ctx *ctx, int32_t n_deals, scopa_multi **out);
int32_t scopa_multi_destroy(scopa_multi *m);
int32_t scopa_multi_deal_py_seeds(scopa_multi *m, const int64_t *h_seeds);
int32_t scopa_multi_set_perms(scopa_multi *m, const uint8_t *h_perms /*[n][16]*/);
int32_t scopa_multi_perms_get(scopa_multi *m, uint8_t *h_perms);
int32_t scopa_multi_build(scopa_multi *m, int32_t *h_n_infosets);
/* one workgroup per deal; from 8192 deals on it takes the lane form below (same bits) when that form's precondition holds */
int32_t scopa_multi_cfr_exact_iterate(scopa_multi *m, int32_t n_iters);
/* the same exact solve with one LANE per deal (64 deals share an instruction stream: the tree shape is deal-independent),
 * tables gathered from HBM: the throughput form for thousands of deals; bit-identical results */
int32_t scopa_multi_cfr_exact_iterate_lanes(scopa_multi *m, int32_t n_iters);
int32_t scopa_multi_cfr_sync_iterate(scopa_multi *m, int32_t n_iters);
/* scopa_cfr_sync_iterate_weighted on every deal with the same weights; h_active[n_deals] (NULL = all): a deal whose byte is 0 is left untouched --
 * tables, first-visit marks and counters -- so a host loop can stop solving the deals that have converged */
int32_t scopa_multi_cfr_sync_iterate_weighted(scopa_multi *m, int32_t n_iters, const double *h_w, int32_t alternating,
                                              const uint8_t *h_active /*[n_deals] or NULL*/);
/* batched MCCFR on every deal at once, persistent: one workgroup per deal keeps the deal's regret table in LDS and runs all
 * n_iters iterations of `batch` traversal pairs without leaving the kernel; same definition (frozen tables per iteration,
 * Philox keyed by seed / traversal id / iteration) as scopa_mccfr_iterate on that deal */
int32_t scopa_multi_mccfr_iterate(scopa_multi *m, uint32_t batch, uint32_t n_iters, uint64_t seed);
int32_t scopa_multi_exploitability(scopa_multi *m, double *h_out4);
int32_t scopa_multi_tables_get(scopa_multi *m, int32_t deal, double *h_regret, double *h_strategy, double *h_local, uint64_t *h_keys);
/* the mirror of scopa_multi_tables_get: [n_infosets of the deal][4] float64 each, a NULL pointer leaves that table alone */
int32_t scopa_multi_tables_set(scopa_multi *m, int32_t deal, const double *h_regret, const double *h_strategy, const double *h_local);
int32_t scopa_multi_counters(scopa_multi *m, uint64_t *decision_visits, uint64_t *terminal_visits);

/* ---- a set of deals with the deal as a chance move ------------------------------------------------------------------------------
 * Chance picks one of a built scopa_multi's n deals uniformly; infosets are identified ACROSS deals by their 56-bit key (what a player who
 * cannot see the other hand knows), so every occurrence of a key shares one regret row and one strategy row.  The scopa_multi is borrowed: it
 * must outlive the handle and must not be dealt or built again while the handle lives; its own per-deal tables are not touched.  At most 65536
 * deals (SCOPA_ELIMIT beyond); an unbuilt multi gives SCOPA_ESTATE.
 *   global id     : rank of the key among the distinct keys of all deals, ascending unsigned
 *   counts        : deals, global infosets G, (deal, infoset) occurrences
 *   index_get     : h_keys[G]; h_map[n][1653] local id -> global id, -1 beyond the deal's infoset count (either may be NULL)
 *   tables        : [G][4] float64 regret and strategy sums (a NULL pointer leaves that table alone), zero after create and reset.  The common
 *                   factor 1/n is NOT applied to them (it cancels in regret matching and in the average policy), only to reported values
 *   cfr_iterate_weighted : scopa_cfr_sync_iterate_weighted's iteration on the shared tables, h_w[n_iters][3] = (pos, neg, strat) per iteration in
 *                   [0, 1] (NULL = all ones; else SCOPA_EINVAL): per (half-)iteration one sweep launch, one workgroup per deal, writes every deal's
 *                   increments, and one reduce launch adds a row's occurrences in ascending (deal, local id) order starting from the first, then
 *                   applies the weights and regret matching.  alternating = 1: two sweeps, sweep p updates player p's rows only, player 0 first.
 *                   No float64 atomics: two runs give the same bits, and one deal gives scopa_cfr_sync_iterate_weighted's.  n_iters = 0: no-op
 *   cfr_iterate_sampled : chance-sampled iterations.  The caller supplies the samples as it supplies the weights (no random numbers enter the
 *                   library): iteration t sweeps only the m deals h_deals[t][0..m), 1 <= m <= n, every id in [0, n) and none twice within an
 *                   iteration (else SCOPA_EINVAL; weights and `alternating` as above; everything is checked before the first launch).  Each listed
 *                   deal gets cfr_iterate_weighted's sweep against the current sigma rows, its increment rows going to slot s of a compact [m][1653][8]
 *                   image.  The reduce adds a row's cells over its SAMPLED occurrences only, in the same ascending (deal, local id) order starting
 *                   from the first sampled one -- the order of the ids within a list changes no bit -- and a row of the updated player(s) with no
 *                   sampled occurrence takes the increment +0.0 for both sums.  Every such row then gets the same update, so the weights discount
 *                   every row every iteration, and m = n gives cfr_iterate_weighted's bits.  alternating = 1: both half-sweeps use the iteration's
 *                   list.  Increments are NOT scaled by n / m: the factor is common and cancels like the 1/n left out above, so runs that mix
 *                   different m weight their iterations by m.  No host synchronisation between iterations; lists and weights are uploaded once
 *                   per call.  n_iters = 0: no-op
 *   mccfr_iterate : chance-sampled external-sampling MCCFR (plain regret matching, no weights, no discount) on the shared rows.  Iteration t of
 *                   a call works on the m distinct deals h_deals[t][0..m) (ids in [0, n), none twice within an iteration, else SCOPA_EINVAL), or on
 *                   all n deals when h_deals is NULL (m is then ignored).  For every listed deal d one workgroup freezes a strategy row (sigma and
 *                   choice thresholds, as scopa_multi_mccfr_iterate does) for each of the deal's infosets from the SHARED regret row of its key,
 *                   and walks `batch` traversal pairs in the deal's tree: global traversal ids d * batch + i, i = 0 .. batch - 1, the handle's
 *                   iteration number and `seed` -- the Philox keying of scopa_mccfr_traverse(iteration, d * batch, batch) on that deal.  Ids follow
 *                   the deal id, not its position in the list: list order and m do not change which random words a deal sees, and two copies of
 *                   one deal draw independent traversals.  The deal's regret increments dR and exact traverser-visit counts c go to its slot of the
 *                   increment image.  The reduce then takes every global row with at least one listed occurrence: R += the sum of dR over its
 *                   listed occurrences (ascending (deal, local id) order, starting from the first listed one); S[k] += (double)(sum of c) *
 *                   sigma_frozen(old R)[k] for k < the legal count, the count summed as an integer and multiplied once; the row's sigma is
 *                   refreshed as the CFR reduces leave it, so MCCFR and CFR iterations may be mixed on one handle.  A row with no listed
 *                   occurrence is not touched (MCCFR has no discount).  Increments are NOT scaled by n / m, as above.  The handle counts its MCCFR
 *                   iterations from 0 at create (tables_reset and tables_set leave the count alone): two calls of 5 and 3 iterations are one
 *                   run of 8.  Two launches per iteration, no host synchronisation in between, lists uploaded once per call.  No float64 atomics
 *                   reach HBM; within a workgroup the walks add into LDS in arrival order, so results are reproducible to rounding, not bit for
 *                   bit.  batch = 0, batch > 2^24, n_iters < 0 or > 2^20, n * batch > 2^32: SCOPA_EINVAL, checked before any launch; a deal whose
 *                   tables do not fit in LDS: SCOPA_ELIMIT.  n_iters = 0: no-op
 *   mccfr_counters : decision and terminal visits of all MCCFR walks of the handle (463 and 240 per traversal pair) and its MCCFR iteration
 *                   count; any pointer may be NULL
 *   exploitability : scopa_exploitability's procedure with every q summed over all deals; h_out4 = {(BR0 + BR1) / 2, BR0, BR1, value}, each
 *                   (v_deal0 + v_deal1 + ...) / n in deal order.  h_policy[G][4] or NULL = the average of the strategy table, uniform where its sum
 *                   is 0; h_policy_out[G][4] (or NULL) receives the evaluated policy
 *   policy_for_deal: scatters a DEVICE policy d_policy_G[G][4] into one deal's local order, d_policy_local[n_infosets(deal)][4] (device): what
 *                   scopa_cross_play, scopa_eval_pair_match and scopa_exploitability take on a context holding that deal */
typedef struct scopa_chance scopa_chance;
int32_t scopa_chance_create(scopa_multi *m, scopa_chance **out);
int32_t scopa_chance_destroy(scopa_chance *g);
int32_t scopa_chance_counts(scopa_chance *g, int32_t *n_deals, int64_t *n_global, int64_t *n_occurrences);
int32_t scopa_chance_index_get(scopa_chance *g, uint64_t *h_keys /*[G]*/, int32_t *h_map /*[n][1653]*/);
int32_t scopa_chance_tables_reset(scopa_chance *g);
int32_t scopa_chance_tables_get(scopa_chance *g, double *h_regret, double *h_strategy);
int32_t scopa_chance_tables_set(scopa_chance *g, const double *h_regret, const double *h_strategy);
int32_t scopa_chance_cfr_iterate_weighted(scopa_chance *g, int32_t n_iters, const double *h_w /*[n_iters][3]; NULL = all ones*/, int32_t alternating);
int32_t scopa_chance_cfr_iterate_sampled(scopa_chance *g, int32_t n_iters, int32_t m, const int32_t *h_deals /*[n_iters][m]*/,
                                         const double *h_w /*[n_iters][3]; NULL = all ones*/, int32_t alternating);
int32_t scopa_chance_mccfr_iterate(scopa_chance *g, int32_t n_iters, uint32_t batch, uint64_t seed,
                                   int32_t m, const int32_t *h_deals /*[n_iters][m]; NULL (m ignored) = all n deals*/);
int32_t scopa_chance_mccfr_counters(scopa_chance *g, uint64_t *decision_visits, uint64_t *terminal_visits, uint32_t *iteration);
int32_t scopa_chance_exploitability(scopa_chance *g, const double *h_policy /*[G][4] or NULL*/, double *h_out4, double *h_policy_out);
int32_t scopa_chance_policy_for_deal(scopa_chance *g, const double *d_policy_G, int32_t deal, double *d_policy_local /*[n_infosets(deal)][4]*/);
/* ---- policy against policy on the chance game: scopa_cross_play, scopa_best_response and scopa_eval_pair_match over the set of deals.  Policies are
 * [G][4] float64 DEVICE tables over global ids in hand order, n_pol of them back to back, used as given: rows are not normalised and a non-finite
 * entry propagates by IEEE rules.  All three launch on the handle's context's stream; cross_play and best_response do not synchronise it.  No float64
 * atomics: every sum has a fixed order, so results are bit-identical from run to run.  n_pol outside [1, 256] or a NULL pointer (d_per_deal, d_br,
 * d_deal_out and d_node_idx_out excepted): SCOPA_EINVAL; a scratch buffer that cannot be allocated: SCOPA_ENOMEM.
 *   cross_play    : d_out[a][b] = { E[reward of seat 0], E[its square], E[scopas of seat 0], E[scopas of seat 1] } of policy a in seat 0 against policy b
 *                   in seat 1, averaged over the deals.  Launch 1: one workgroup per (deal, a, b) gathers the combined table of the deal into LDS through
 *                   the deal's map row and runs scopa_cross_play's eight levels, `v = 0.0; v += row[c] * child[c]`, children left to right, into the
 *                   per-deal image -- d_per_deal[n][n_pol][n_pol][4], or (NULL) a scratch buffer of the handle that grows on demand.  Launch 2: one lane
 *                   per (a, b, quantity), s = img[0]; s += img[1]; ... in deal order, then s / (double)n.  d_per_deal[d] is bit for bit what
 *                   scopa_cross_play writes on a context holding deal d for the policy_for_deal tables; d_out[a][a][0] is the value
 *                   scopa_chance_exploitability reports for policy a; one deal gives scopa_cross_play's bits.  n * n_pol * n_pol >= 2^31: SCOPA_ELIMIT.
 *                   LDS: 32 * I_max + 36 864 + 3 312 bytes at the largest deal's infoset count I_max (76 720 at the 1 142 of the 495-deal
 *                   hidden-hand set); beyond the context's LDS limit: SCOPA_ELIMIT before anything is launched (scopa_debug_lds_limit only)
 *   best_response : scopa_chance_exploitability's procedure for n_pol policies at once, its kernels with a policy index in the grid: d_out4[k] =
 *                   {(BR0 + BR1) / 2, BR0, BR1, value}, bit for bit what scopa_chance_exploitability(g, policy k, ...) returns -- every q summed over a
 *                   ply's nodes ascending from 0.0, then over the key's occurrences in ascending (deal, local id) order from the first; a strict `>`,
 *                   ties to the lowest action.  d_br (or NULL): d_br[k][p] is a complete [G][4] table -- player p's rows one-hot at the chosen action,
 *                   the other player's rows policy k's -- fit to go back into cross_play or match.  Scratch per policy: n * (2 * 2 229 * 8 + 1 653 * 64)
 *                   + 4 G bytes (70 MB at 495 deals); the policies go through in chunks whose scratch stays below 1 GiB (one policy at least), and
 *                   chunking changes no bit.  No dynamic LDS, so no LDS refusal
 *   debug_scratch_budget : test hook: that budget in bytes (0 restores 1 GiB), so that the chunked route can be reached with a handful of policies
 *   match         : scopa_eval_pair_match with the deal drawn per episode.  Episode i draws deal = (x0 * n_deals) >> 32 from the first Philox word of
 *                   counter (i, i >> 32, 8, stream_id) under the context's seed (scopa_mccfr_seed; the plies use tags 0 to 5): a deal's probability
 *                   departs from 1 / n_deals by at most 2^-32, the uniform law's by at most n_deals / 2^32 in total.  The episode then walks that
 *                   deal's tree as scopa_eval_pair_match does: counters (i, i >> 32, ply, stream_id), the same 53-bit integer, the same three compares
 *                   against thresholds computed per global row by the same formula with the legal count of the global key; episodes i < n_seat0 have a
 *                   in seat 0.  An episode that drew deal d ends at the terminal index scopa_eval_pair_match(ctx_d, policy_for_deal(a, d),
 *                   policy_for_deal(b, d), n, n_seat0, stream_id, ...) writes at d_node_idx_out[i] on a context holding d under the same seed.
 *                   d_deal_out[n], d_node_idx_out[n] (int32, or NULL): every episode's deal and terminal index.  h_stats[half][5] = episodes, sum of
 *                   a's rewards x2, sum of their squares, a's scopas, b's scopas: exact integers.  One lane per episode gathers the node's infoset, its
 *                   global id and the threshold row from global memory (the set's tables do not fit in LDS).  Synchronous; n = 0 gives zeros and
 *                   launches nothing; n < 0 or n_seat0 outside [0, n]: SCOPA_EINVAL */
int32_t scopa_chance_cross_play(scopa_chance *g, int32_t n_pol, const double *d_policies /*[n_pol][G][4]*/, double *d_per_deal /*[n][n_pol][n_pol][4] or NULL*/,
                                double *d_out /*[n_pol][n_pol][4]*/);
int32_t scopa_chance_best_response(scopa_chance *g, int32_t n_pol, const double *d_policies /*[n_pol][G][4]*/, double *d_br /*[n_pol][2][G][4] or NULL*/,
                                   double *d_out4 /*[n_pol][4]*/);
int32_t scopa_chance_debug_scratch_budget(scopa_chance *g, int64_t bytes);
int32_t scopa_chance_match(scopa_chance *g, const double *d_policy_a, const double *d_policy_b, int64_t n, int64_t n_seat0, uint32_t stream_id,
                           int32_t *d_deal_out /*[n] or NULL*/, int32_t *d_node_idx_out /*[n] or NULL*/, int64_t h_stats[10]);
/* ---- Deep CFR over the set of deals: one advantage net per player serves every deal, because its 34 features are a function of the infoset key alone.
 * Both calls launch on the handle's context's stream and do not synchronise it.
 *   sdcfr_traverse : scopa_sdcfr_traverse_fused's default form (policy table + walks) for m deals in two launches.  The deals are h_deals[0..m), distinct ids
 *                   in [0, n), or all n deals (slot = deal) when h_deals is NULL and m is 0.  Launch 1 (grid: 105 tiles x m) evaluates the 1 653 decision
 *                   nodes of every listed deal under the frozen nets d_image (scopa_sdcfr_pack_weights) with k_sdcfr_policy's tile, from a node-info image
 *                   [n][1653] built once per handle, into [m][1653] policies and thresholds.  Launch 2 walks `batch` traversals per listed deal: a workgroup
 *                   serves one slot and a contiguous chunk of its traversals with k_sdcfr_walk's LDS carving (33 KB: the deal's compact tables and payoffs,
 *                   twelve wavefronts' scratch), per-wavefront task, Philox keying and row sweep; workgroups per deal = ceil(2 * compute units / m), at
 *                   most `batch`, at least 1.  Traversal i of deal d in slot s has global id b0 + d * batch + i -- keyed by the deal, as in mccfr_iterate, so
 *                   list order and m change no draw -- its 41 memory rows go to ring rows (write_base + 41 * (s * batch + i) + rank) % capacity and its
 *                   root value to d_root_values[s * batch + i].  Rows and root values are, bit for bit, those of m calls
 *                   scopa_sdcfr_traverse_fused(ctx_d, traverser, batch, ..., (write_base + 41 * s * batch) % capacity, ..., iteration, b0 + d * batch) on
 *                   contexts holding deal d under the same scopa_mccfr_seed.  d_mem_mask may be NULL, as there.  Refused with SCOPA_EINVAL and a message
 *                   in scopa_last_error, before anything is launched or written: a NULL pointer; traverser outside {0, 1}; batch < 0, or 0 with a list;
 *                   a list with m outside [1, n], an id outside [0, n) or an id twice; no list with m other than 0 or n; d_image / d_mem_regret /
 *                   d_mem_mask not 16-byte or d_mem_feat not 8-byte aligned; capacity < 41 or >= 2^30; write_base outside [0, capacity);
 *                   41 * m * batch > capacity; b0 + n * batch > 2^32.  An LDS limit below the walk's carving: SCOPA_ELIMIT.  batch = 0 without a list:
 *                   no-op.  Only this form is built: the forward-per-visit kernel (scopa_sdcfr_mode 1) and replayed uniforms stay single-deal.
 *                   Next lever, not attempted: policies are evaluated per listed deal, 1 653 x m nodes, not once per distinct key.
 *   sdcfr_visits  : decision visits of the handle's traversal calls, 105 / 82 per traversal of traverser 0 / 1, counted on the host
 *   sdcfr_average_policy : scopa_sdcfr_average_policy's definition evaluated once per distinct key of `player`: the FIFO float32 sum of
 *                   positive_regret_policy(net_s(x)) * d_coef[s], the float64 normalisation over the legal slots, uniform where the sum is 0 or not finite,
 *                   zeros beyond the legal count, a slot outside the store giving NaN and hence uniform; written to d_policy_G[G][4] (float64, device).
 *                   Rows of the other player are left untouched.  x comes from the key's representative node -- the first node of its first occurrence in
 *                   ascending (deal, local id) order -- listed once per handle, per player in ascending global id; the terms pass tiles that list sixteen
 *                   keys at a time with k_sdcfr_avg_terms's tile, the reduce takes one lane per row.  No atomics: bit-identical from run to run, and
 *                   d_policy_G[map[d][l]] is bit for bit the row scopa_sdcfr_average_policy writes for infoset l on a context holding deal d.  Arguments
 *                   and alignments as there (violations: SCOPA_EINVAL with a message). */
int32_t scopa_chance_sdcfr_traverse(scopa_chance *g, int32_t traverser, int32_t batch, int32_t m, const int32_t *h_deals /*[m]; NULL (m = 0) = all n deals*/,
                                    const float *d_image, float *d_mem_feat, float *d_mem_regret, float *d_mem_mask /*may be NULL*/, int64_t capacity,
                                    int64_t write_base, float *d_root_values /*[m * batch]*/, uint32_t iteration, uint32_t b0);
int32_t scopa_chance_sdcfr_visits(scopa_chance *g, uint64_t *decision_visits);
int32_t scopa_chance_sdcfr_average_policy(scopa_chance *g, int32_t player, int32_t n_snap, const float *d_w1, const float *d_b1, const float *d_w2,
                                          const float *d_b2, const float *d_w3, const float *d_b3, int32_t max_size, const int32_t *d_slots,
                                          const float *d_coef, double *d_policy_G /*[G][4]*/);

/* ---- FullScopa: the 40-card game (src/envs/full_scopa_game.py, src/envs/openspiel_full_scopa.py) -- state engine -------------
 * No reference solver uses it; provided: deal, the state protocol, and the batched device step.
 * Card id = action id = suit_idx*10 + rank-1 (denari, coppe, spade, bastoni).  A state refers to its deck (the deal order,
 * needed for the re-deals) by index `game` into a caller-supplied array of 40-byte decks. */
typedef struct scopa_full_state {   /* 64 bytes */
    uint64_t table[2];     /* ordered table, 20 six-bit slots (10 per word)                                   */
    uint64_t cap[2];       /* captured cards per player, 40-bit masks                                          */
    uint32_t hand[2];      /* ordered hands, 3 six-bit slots                                                   */
    uint32_t game;         /* deck index                                                                       */
    uint8_t  nh[2], nt, deck_pos, round, last_capture /* 0xFF = none */, scopas[2];
    uint16_t step;
    uint8_t  terminal;
    int8_t   r2_p0;        /* rewards x2 of player 0 once terminal (player 1 = negation)                       */
    uint8_t  flags;        /* bit 0: table capacity (20) exceeded                                              */
    uint8_t  pad[7];
} scopa_full_state;
int32_t scopa_full_deal_py_seed(int64_t seed, uint8_t perm40[40]);                              /* FullDeck.__init__ :29-32 */
int32_t scopa_full_state_init(const uint8_t deck40[40], uint32_t game, scopa_full_state *out);  /* FullScopaGame.reset :60-75 */
int32_t scopa_full_state_step(scopa_full_state *s, const uint8_t deck40[40], int32_t action);   /* FullScopaEnv.step :252-297 */
int32_t scopa_full_state_legal(const scopa_full_state *s, int32_t player, int32_t out[3], int32_t *n);
int32_t scopa_full_state_infoset_string(const scopa_full_state *s, int32_t player, char *buf, int32_t cap);
/* d_states[i] <- step(d_states[i], d_decks[d_states[i].game], d_actions[i]) */
int32_t scopa_full_step_batch(scopa_ctx *ctx, scopa_full_state *d_states, const uint8_t *d_actions, const uint8_t *d_decks, int64_t n);
int32_t scopa_full_step_batch_host(scopa_ctx *ctx, scopa_full_state *h_states, const uint8_t *h_actions, const uint8_t *h_decks,
                                   int64_t n_decks, int64_t n);
/* n_games uniform-random playouts to the end, one lane per game, decks dealt ON DEVICE from seeds[i] (CPython shuffle);
 * h_r2_p0[n] = rewards x2 of player 0, h_plies[n] = game length.  Philox stream (ctx seed, game, ply). */
int32_t scopa_full_random_playouts(scopa_ctx *ctx, const int64_t *h_seeds, int64_t n_games, int8_t *h_r2_p0, int16_t *h_plies);

/* ---- FullScopa: external-sampling MCCFR on a device hash table of infosets (build-defined: the reference's MCCFRTrainer cannot run on
 * FullScopaGame).  One deal has 36^6 histories, so rows are kept by KEY in an open-addressing store that grows as infosets are met.
 *   infoset_key   : host code, no GPU needed.  Over the decision nodes of one deck, two (state, player to move) pairs have equal keys exactly when
 *                   scopa_full_state_infoset_string gives equal strings; a key is never 0.  Packing: bit 63 set | player (bit 62) | round (3 bits) |
 *                   hand: which of the player's three cards of the round, deck40[4 + 6 round + 3 player + i], are still held (bit 56 + i) | table as a
 *                   40-bit card mask (bit 16 + card) | cards captured by the player (6 bits) | scopas of player 0, of player 1 (5 bits each).  The
 *                   opponent's capture count follows from the cards dealt so far.  Action slot a of a key is its a-th held card in deal order, which is
 *                   the state engine's hand order; the action count of a key is the number of hand bits.  A NULL pointer, a player outside {0, 1}, a
 *                   deck that is no permutation, or a state with round > 5, a hand above 3 or a table above 20: SCOPA_EINVAL
 *   create        : a store of 2^capacity_log2 slots of 128 bytes (key | regret[3] | strategy[3] | d_regret[3] | d_strategy[3] | visit count, uint32),
 *                   all zero, for the game of deck40 from root_state (NULL = the deal's initial state).  The root must be a non-terminal state at a
 *                   round boundary (step % 6 == 0) holding the deck's deal of its round; capacity_log2 in [4, 28]; else SCOPA_EINVAL.  SCOPA_ENOMEM
 *                   where the device cannot hold the store.  Destroy the handle before its context.  Counters start at 0
 *   slots         : a slot is claimed with one 64-bit compare-and-swap on its key word; probing is linear from a hash of the key over at most 64 slots,
 *                   and no loop anywhere waits for another lane, wavefront or workgroup.  An insert that finds the 64 slots taken by other keys adds
 *                   1 to `dropped`, skips that one update, and makes the call that launched it return SCOPA_ENOMEM (the calls that can claim slots --
 *                   traverse, iterate, tables_set -- synchronise once at their end to read the counter).  Rows that were updated are still right.
 *                   There is no resize in place: create a larger store and tables_set
 *   traverse      : traversals b0 .. b0 + nb - 1 of `traverser` from the root against the regrets as they are (frozen for the launch).  Writes only
 *                   d_regret, d_strategy and the visit counts, claiming slots where needed.  With q the mixed-radix number of the traverser's own
 *                   choices so far (0 at the root; q <- q n + a at a traverser node with n cards; q < 46 656): a terminal node returns r2_p0 / 2,
 *                   negated for traverser 1; a mover with one card plays it (no row, no draw, no count); otherwise sigma = regret matching
 *                   (InfoNode.current_strategy) of the regret row of the mover's key, an absent key being a zero row.  Opponent node:
 *                   d_strategy[a] += sigma[a], count += 1, then ONE action: the first slot whose running sum of sigma exceeds u (the last slot
 *                   as fallback), u = u53(x0, x1) of Philox4x32-10 under scopa_mccfr_seed's key of the handle's context at counter
 *                   (state.step << 16 | q, traversal id, iteration, 160 + traverser); the node's value is the child's.  Traverser node: cfv[a] = the
 *                   value of child a, in hand order; v = 0; v += sigma[a] cfv[a] left to right; d_regret[a] += cfv[a] - v; count += 1; the value
 *                   is v (no strategy term: a player's strategy sums grow while it is the opponent -- stochastically weighted averaging).  Draws are
 *                   named by node, not by lane, so the result does not depend on the cut (below) beyond the order of the float64 atomic adds:
 *                   counts, key set and counters are exact, rows met once per launch are bit-identical, the others reproducible to rounding.
 *                   traverser outside {0, 1}, nb > 1 << 24, b0 + nb above 2^32: SCOPA_EINVAL with nothing changed; nb = 0 is a no-op
 *   cut           : how a launch is decomposed.  0: a lane per traversal walks the whole tree depth-first (a stack of 12 frames of 128 bytes, at the
 *                   traverser's choice nodes).  K in 1..3: a workgroup per traversal; lane c < 6^K replays the first K rounds with the traverser's
 *                   choices set to the digits of c, reading sigma and writing nothing (frozen sigma and node-keyed draws make the replay exact), walks
 *                   the sub-tree below with updates and leaves its value in LDS; after one workgroup barrier lane 0 walks the first K rounds with
 *                   updates and takes sub-tree q's value where it reaches the cut.  -1 (the default): min(3, rounds from the root / 2).  A cut
 *                   above min(3, rounds from the root) or below -1: SCOPA_EINVAL
 *   apply         : one launch over the slots: regret += d_regret, strategy += d_strategy, d_* and the count to zero.  The iteration counter += 1
 *   iterate       : per iteration traverse(0), apply, traverse(1), apply, traversal ids 0 .. batch - 1, the iteration word of each traversal launch
 *                   being the handle's counter at that point (so it advances by 2 per iteration).  No host synchronisation between iterations;
 *                   one at the end of the call.  batch outside [1, 1 << 24] or n_iters > 1 << 20: SCOPA_EINVAL; n_iters = 0 is a no-op
 *   counters      : exact integers since create: choice visits (nodes whose mover holds 2 or 3 cards), terminal visits, rows occupied (zeroed by
 *                   reset and tables_set), dropped, the iteration counter (applies).  Any pointer may be NULL.  One traversal from a root at the start
 *                   of round r0, with S = (6^(6 - r0) - 1) / 5, makes 13 S choice visits as traverser 0, 8 S as traverser 1, and 6^(6 - r0) terminal
 *                   visits: 121 303, 74 648 and 46 656 from the deal's root
 *   tables_get    : the occupied rows in any order.  *n_rows holds the room of the arrays on entry and the number of rows on return; with every array
 *                   NULL only the number is returned; less room than rows: SCOPA_EINVAL (the number still returned).  n_act[i] is the key's action
 *                   count, regret and strategy are [n_rows][3] with the unused third slot 0.  delta_get: the same for d_regret, d_strategy and the
 *                   visit counts, as the traversals since the last apply left them.  Any array may be NULL
 *   tables_set    : clears the store (rows, increments, counts; the other counters stay) and inserts the given rows: checkpoints, planted tables.
 *                   n_rows outside [0, 2^capacity_log2], a NULL array with n_rows > 0, a key without bit 63, n_act[i] that is not the key's action
 *                   count or is below 2, a key twice: SCOPA_EINVAL with nothing changed.  reset: clears the store the same way
 *   match         : the seat-swapped match of evaluate_agent (mc_cfr.py:146-206) from the root: episodes i with 2 i < n_episodes have the agent in
 *                   seat 0.  The agent plays the average policy -- the strategy row of the mover's key over its sum; uniform where the key is absent
 *                   or the sum <= 1e-12 (ScopaLearnedPolicy) -- and the opponent uniformly: the first slot whose running sum of the probabilities
 *                   exceeds u, the last as fallback, u from Philox counter (i, i >> 32, stream_id << 8 | state.step, 176); a mover with one card
 *                   plays it.  One lane per episode; reads the store, never inserts.  h_sums[6] = sum of the agent's rewards x2 in seat 0, in
 *                   seat 1, the sums of their squares in seat 0, in seat 1, the agent's scopas, the opponent's scopas: exact integers summed on
 *                   the device.  h_r2_agent[n] (int8, or NULL): the agent's reward x2 of every episode.  Synchronous.  n_episodes < 0 or above
 *                   1 << 40 (1 << 31 with h_r2_agent), stream_id >= 1 << 24, h_sums NULL: SCOPA_EINVAL; n_episodes = 0 gives zeros
 *   exploitability: (scopa_amd/csrc/scopa_full_eval.hip) the exact value of the stored policy on the sub-game below `root`, and an exact pure response to it
 *                   for either player: h_out4 = {(BR0 + BR1) / 2, BR0, BR1, value}, value for player 0.  root (NULL = the handle's root) may be any
 *                   non-terminal round-boundary state (step % 6 == 0) of the handle's deck that holds the deck's deal of its round -- create's check -- so
 *                   a store trained from the deal's root can be measured on a later sub-game.  With R = 6 - root.round rounds left the sub-game has 36^R
 *                   histories (36, 1 296, 46 656, 1 679 616 for R = 1..4), movers alternating from player 0 with 3, 3, 2, 2, 1, 1 cards through a round;
 *                   it is swept whole, level by level.  R > 4: SCOPA_ELIMIT with nothing changed.  A NULL handle, NULL h_out4, which outside {0, 1}, a
 *                   bad root: SCOPA_EINVAL before any launch.  Synchronous; reads the store (fm_find, never claiming a slot) and leaves the counters,
 *                   the rows and the increments alone.  Every sum has ONE order -- no float64 atomics -- so the results are bit-identical from run to run
 *                   and to tests/full_exploit_ref.py, the float64 restatement of this procedure:
 *                     1 expand   level 0 is the root; node i of level d, whose mover holds n cards, has children i n + a at level d + 1, child a reached
 *                                by playing the a-th held card in hand order; 6 R levels of children
 *                     2 policy   at a node whose mover holds n >= 2 cards, prob[a] from the row of the mover's infoset_key.  which = 0, the average
 *                                policy: strategy[a] / total, total summed left to right over the n slots; uniform 1.0 / n where the key is absent or
 *                                total <= 1e-12 (match's rule).  which = 1: regret matching of the regret row as the traversal computes sigma, an absent
 *                                key being a zero row.  A one-card mover plays its card with probability 1.0
 *                     3 value    terminal: r2_p0 / 2.0; inner node: v = 0.0; v += prob[a] * child[a], left to right, bottom up; a one-card node takes its
 *                                child's value.  h_out4[3] is the root's
 *                     4 response of player p (0, then 1).  Reach: w[root] = 1.0, w[child a] = w[node] * prob[a] at the other player's choice nodes,
 *                                w[node] elsewhere.  Terminal: r2_p0 / 2.0, negated for p = 1.  Bottom up, level by level: the other player's nodes as in
 *                                3; at p's choice nodes Q[key][a] = 0.0; Q[key][a] += w[node] * V[child a] over the level's nodes holding that key in
 *                                ASCENDING node index, a*(key) = the first maximal slot among the key's n, V[node] = V[child a*(key)].  BR_p = V[root]
 *                   IMPERFECT RECALL: the key holds the round, the cards held, the table, the capture count and the scopas, and forgets the player's own
 *                   plays of earlier rounds.  Within a round recall is perfect, so for R = 1 step 4 gives THE best response.  For R > 1 it gives A pure
 *                   response whose value is computed exactly: BR_p is a value some responder really achieves, (BR0 + BR1) / 2 is a LOWER bound on the
 *                   true exploitability, and BR_p is not proved to be at least the policy's own value.
 *                   Scratch is allocated at the first call, kept in the handle, grown when a larger R comes and freed by destroy (SCOPA_ENOMEM where
 *                   the device cannot hold it): about 8 KB, 0.2 MB, 7.5 MB, 271 MB for R = 1..4, plus the sort's own
 *   response_get  : the rows of the last exploitability call for `player`, sorted by key: key, action count, chosen slot a*, Q[3] with the unused third
 *                   slot 0.0 (every key of the player that the sub-game holds, reached or not: Q is all 0.0 where no history of the key has w > 0).
 *                   *n_rows as in tables_get: room in, count out; every array NULL: the count only; too little room: SCOPA_EINVAL with the count
 *                   still returned.  SCOPA_ESTATE where no exploitability call has completed since create.  The rows stay valid until the next
 *                   exploitability call or destroy.  player outside {0, 1}: SCOPA_EINVAL
 * Every entry point but infoset_key returns SCOPA_EINVAL for a NULL handle before it touches the device. */
typedef struct scopa_full_mccfr scopa_full_mccfr;
int32_t scopa_full_infoset_key(const scopa_full_state *s, const uint8_t deck40[40], int32_t player, uint64_t *key);
int32_t scopa_full_mccfr_create(scopa_ctx *ctx, const uint8_t deck40[40], const scopa_full_state *root_state, int32_t capacity_log2, scopa_full_mccfr **out);
int32_t scopa_full_mccfr_destroy(scopa_full_mccfr *h);
int32_t scopa_full_mccfr_root(const scopa_full_mccfr *h, scopa_full_state *root, uint8_t deck40[40], int32_t *capacity_log2);   /* what create was given; any may be NULL */
int32_t scopa_full_mccfr_cut(scopa_full_mccfr *h, int32_t cut);
int32_t scopa_full_mccfr_reset(scopa_full_mccfr *h);
int32_t scopa_full_mccfr_traverse(scopa_full_mccfr *h, int32_t traverser, uint32_t iteration, uint32_t b0, uint32_t nb);
int32_t scopa_full_mccfr_apply(scopa_full_mccfr *h);
int32_t scopa_full_mccfr_iterate(scopa_full_mccfr *h, uint32_t batch, uint32_t n_iters);
int32_t scopa_full_mccfr_counters(scopa_full_mccfr *h, uint64_t *choice_visits, uint64_t *terminal_visits, uint64_t *rows, uint64_t *dropped, uint32_t *iterations);
int32_t scopa_full_mccfr_tables_get(scopa_full_mccfr *h, int64_t *n_rows, uint64_t *keys, int32_t *n_act, double *regret /*[n_rows][3]*/, double *strategy /*[n_rows][3]*/);
int32_t scopa_full_mccfr_delta_get(scopa_full_mccfr *h, int64_t *n_rows, uint64_t *keys, double *d_regret /*[n_rows][3]*/, double *d_strategy /*[n_rows][3]*/, uint32_t *counts);
int32_t scopa_full_mccfr_tables_set(scopa_full_mccfr *h, int64_t n_rows, const uint64_t *keys, const int32_t *n_act, const double *regret, const double *strategy);
int32_t scopa_full_mccfr_match(scopa_full_mccfr *h, int64_t n_episodes, uint32_t stream_id, int64_t h_sums[6], int8_t *h_r2_agent /*[n_episodes] or NULL*/);
int32_t scopa_full_mccfr_exploitability(scopa_full_mccfr *h, const scopa_full_state *root /*NULL = the handle's root*/,
                                        int32_t which /*0 = average policy, 1 = current regret-matching sigma*/, double h_out4[4]);
int32_t scopa_full_mccfr_response_get(scopa_full_mccfr *h, int32_t player, int64_t *n_rows, uint64_t *keys, int32_t *n_act, int32_t *action,
                                      double *q /*[n_rows][3]*/);

/* ---- FullScopa over a SET of decks, the deal as a chance move: deck-free two-word keys, deal-sampled external-sampling MCCFR (build-defined;
 * scopa_amd/csrc/scopa_full_chance.hip, scopa_full_wide.h).  The one-word key above names a hand by positions in ONE deck, so its rows mean nothing on
 * another deck.  Here a row is kept by what the mover sees, every traversal walks one deck of a set from a common root, all decks add into the rows they
 * share, and the average policy can be played on decks it was not trained on.  exploitability measures it exactly across a set of decks.
 *   infoset_key_wide: host code, no GPU needed.  key2[0] = A: bit 63 set | player (bit 62) | round (bits 59-61) | bits 56-58 zero | table as a 40-bit card
 *                   mask (bit 16 + card) | cards captured by the player (bits 10-15) | scopas of player 0 (bits 5-9), of player 1 (bits 0-4): the one-word
 *                   key with its hand field empty.  key2[1] = B: the player's hand as a 40-bit card mask, never 0 at a decision node.  Neither word reads
 *                   a deck.  Over the decision nodes of ANY decks two (state, player to move) pairs have equal (A, B) exactly when
 *                   scopa_full_state_infoset_string gives equal strings (the opponent's capture count follows from the cards dealt so far).  Action slot a
 *                   of a key is its a-th held card in ASCENDING CARD ID -- the a-th set bit of B -- not in hand order, which is deal order and differs
 *                   between decks that share the infoset; the action count is popcount(B).  A NULL pointer, a player outside {0, 1}, a state with
 *                   round > 5, a hand above 3 or a table above 20: SCOPA_EINVAL
 *   create        : a store of 2^capacity_log2 slots of 128 bytes (A | regret[3] | strategy[3] | d_regret[3] | d_strategy[3] | visit count | B), all zero,
 *                   for the n_decks decks [n_decks][40] below root_state (NULL = the initial state of decks[0]).  n_decks in [1, 1 << 20], capacity_log2 in
 *                   [4, 28].  The root must be a non-terminal state at a round boundary (step % 6 == 0, deck_pos == 10 + 6 round); its hands are IGNORED.
 *                   Every deck must be a permutation of 0..39 whose cards at positions >= 4 + 6 round are exactly the cards not on the root's table or in
 *                   its capture piles, and at round 0 must start with the root's four table cards in table order (the table is ordered and the capture
 *                   rule reads the order).  Anything else: SCOPA_EINVAL.  A traversal or episode on deck d starts from the root with the hands
 *                   d[4 + 6 round + 3 p + i].  SCOPA_ENOMEM where the device cannot hold the store.  Destroy the handle before its context
 *   slots         : home = hash(A ^ B * 0x9E3779B97F4A7C15) with the one-word store's hash, linear probing over at most 64 slots.  A slot is claimed by ONE
 *                   compare-and-swap of word A from 0 and then ONE of word B from 0, made by whoever sees its own A there; the lane that publishes B counts
 *                   the row; another B in the slot means another hand of the same A owns it for good and the probe goes on.  No loop anywhere waits for
 *                   another lane, wavefront or workgroup; a key pair occupies at most one slot; nothing is deleted between resets; a read-only probe
 *                   that meets word A with word B still 0 takes the row as absent (it was claimed in this launch: a zero row).  A full probe adds 1 to
 *                   `dropped`, skips that update and makes the call return SCOPA_ENOMEM, as above
 *   traverse      : traversals b0 .. b0 + nb - 1 of `traverser` on EACH listed deck (h_list[m] deck indices; NULL = every deck, m ignored), one launch.
 *                   The walk is scopa_full_mccfr_traverse's -- frozen regrets, regret matching, opponent nodes add sigma and the count and sample one
 *                   action, traverser nodes take every action and add cfv - v, a one-card mover adds no row, no draw and no count -- with three changes:
 *                   rows by (A, B); slot a is the a-th held card in ascending card id, and q is the mixed-radix number of the traverser's own SLOT
 *                   choices; the draw at Philox counter (state.step << 16 | q, traversal id, iteration, deck_index << 8 | 192 + traverser), deck_index
 *                   the index in the handle, not in the list, so the result does not depend on the list's order or length.  Listed decks must be
 *                   distinct and in range, traverser in {0, 1}, nb <= 1 << 24, b0 + nb <= 2^32, m x nb <= 1 << 30: else SCOPA_EINVAL with nothing
 *                   changed.  nb = 0 or m = 0 is a no-op
 *   cut           : as scopa_full_mccfr_cut; at K > 0 a workgroup per (listed deck, traversal), at 0 a lane
 *   apply, reset, counters: as above.  One traversal per listed deck makes the one-deck shape counts on each
 *   iterate       : per iteration traverse(0), apply, traverse(1), apply over that iteration's list h_lists[t][0..m) (NULL: every deck), traversal ids
 *                   0 .. batch - 1, the iteration word from the handle's counter.  The lists are uploaded once per call; no host synchronisation between
 *                   iterations, one at the end.  Nothing is scaled by n_decks / m; rows without a listed occurrence are untouched.  A bad list, batch
 *                   outside [1, 1 << 24], n_iters > 1 << 20, m x batch > 1 << 30: SCOPA_EINVAL with nothing changed
 *   tables_get, delta_get: as above with keys2 [n_rows][2] = (A, B) per row; n_act[i] = popcount(B)
 *   tables_set    : as above; validates bit 63 of A, B < 2^40, popcount(B) == n_act[i] in {2, 3}, no pair twice: else SCOPA_EINVAL with nothing changed
 *   match         : the seat-swapped match of the average policy against uniform play, as scopa_full_mccfr_match, on h_decks [k][40] (NULL: the handle's
 *                   decks).  Episode i has the agent in seat 0 where 2 i < n_episodes; with j = i in the first half and i - ceil(n_episodes / 2) in the
 *                   second it is played on deck j mod k, so both seats meet the same decks.  Draws at Philox counter (i, i >> 32, stream_id << 8 |
 *                   state.step, 208), slots in ascending card id.  Held-out decks must pass create's deck check against the handle's root, else
 *                   SCOPA_EINVAL: the policy is a function of the key alone, so it plays on any of them.  Reads the store, never inserts.  One launch, a lane
 *                   per episode: n_episodes above 1 << 36 (1 << 31 with h_r2_agent) or below 0, stream_id >= 1 << 24, h_sums NULL: SCOPA_EINVAL
 *   root          : what create was given: the root, the decks [n_decks][40], their number, capacity_log2; any pointer may be NULL
 *   exploitability: (scopa_amd/csrc/scopa_full_chance_eval.hip) the exact value of the stored policy on the sub-games below `root` on the k decks
 *                   h_decks [k][40] (NULL: the handle's decks, k ignored), the deal a uniform chance move over them, and an exact pure response to it
 *                   for either player ACROSS the decks: the responder plays ONE action at all histories that share the pair (A, B), on every deck.
 *                   h_out4 = {(BR0 + BR1) / 2, BR0, BR1, value}, value for player 0.  root (NULL = the handle's root) must be a non-terminal round
 *                   boundary as create asks; its hands are ignored.  Every evaluated deck must pass create's deck check against THAT root, so a store
 *                   can be measured on held-out decks and on a descendant round boundary that all the decks fit; a deck listed twice counts twice.
 *                   Checked in this order, each before any launch and with nothing changed: a NULL handle or h_out4, which outside {0, 1}, k < 1 with
 *                   h_decks given, a bad root: SCOPA_EINVAL; R = 6 - root.round > 4 or k x 36^R > 1 << 22 (3 236 decks at R = 2, 89 at R = 3, 2 at
 *                   R = 4): SCOPA_ELIMIT; a deck that does not fit: SCOPA_EINVAL.  Synchronous; reads the store (fw_find, never claiming a slot) and
 *                   leaves the counters, the rows and the increments alone.  It is scopa_full_mccfr_exploitability's procedure over a FOREST of one
 *                   tree per deck, and bit-identical to tests/full_chance_exploit_ref.py, its float64 restatement:
 *                     1 forest   with n decks and the one-deck level sizes size[k] (per round 1, 3, 9, 18 times 36^r: only levels whose mover has a
 *                                choice are numbered, the two one-card plies that end a round being played on the way), level k has n size[k] nodes;
 *                                node g = d size[k] + i is node i of deck d's tree, the roots are root_on(root, deck d) -- the root with the hands
 *                                deck[4 + 6 round + 3 p + i].  size[k + 1] = size[k] n_k, so child a of g is g n_k + a and the deck of a node is
 *                                g / size[k].  Child a is reached by the mover's a-th held card in ASCENDING CARD ID, not in hand order: slot a then
 *                                means the same card on every deck that shares the pair
 *                     2 policy   prob[a] from the row of the mover's pair (A, B), found by the read-only probe.  which = 0: match's rule,
 *                                strategy[a] / total with total summed left to right, uniform 1.0 / n where the pair is absent or total <= 1e-12.
 *                                which = 1: regret matching of the regret row; an absent pair, or a slot whose word B is unpublished, is a zero row
 *                     3 value    leaf: r2_p0 / 2.0; bottom up v = 0.0; v += prob[a] * child[a] in slot order.
 *                                h_out4[3] = (0.0 + V[root 0] + V[root 1] + ...) / n, added in deck order
 *                     4 response of player p (0, then 1).  w[root d] = 1.0 for every deck (the chance weight 1 / n is applied once, at the end);
 *                                w[child a] = w[node] * prob[a] at the other player's nodes, w[node] at p's.  Leaves negated for p = 1.  Bottom up: the
 *                                other player's levels as in 3; at p's levels Q[(A, B)][a] = 0.0; Q[(A, B)][a] += w[g] * V[child a] over ALL forest nodes
 *                                of the level that hold the pair, on every deck, in ASCENDING g; a* = the first maximal slot; V[g] = V[child a*].
 *                                BR_p = (0.0 + V[root 0] + V[root 1] + ...) / n, added in deck order
 *                     5 order    no float64 atomic anywhere: the same decks in the same order give the same bits.  A permuted deck list regroups
 *                                the adds of steps 3 and 4 and may change the last bits
 *                   IMPERFECT RECALL, as for one deck: the pair forgets the player's own plays of earlier rounds, so for R > 1 step 4 gives A pure
 *                   response whose value is exact -- BR_p is a value some responder really achieves, (BR0 + BR1) / 2 is a LOWER bound on the true
 *                   exploitability, and BR_p is not proved to be at least the policy's own value.  At R = 1 all six remaining cards are dealt, so a
 *                   player's hand fixes the opponent's: decks that share a pair are one game up to hand order, and BR_p is the mean of the per-deck
 *                   best responses.  Hidden hands begin to matter at R >= 2.
 *                   Scratch is one allocation kept in the handle, grown when a call needs more and freed by destroy (SCOPA_ENOMEM where the device
 *                   cannot hold it): with T = 31 n (36^R - 1) / 35 nodes about 168 T + 8 n 36^R + 57 x 18 n 36^(R-1) bytes plus the sorts' own --
 *                   0.8 GB at the cap
 *   response_get  : the rows of the last exploitability call for `player`, sorted by (A, B): keys2 = the pair, n_act = popcount(B), the chosen slot
 *                   a*, Q[3] with the unused third slot 0.0 (every pair of the player that the forest holds, reached or not).  *n_rows, the count
 *                   alone, too little room, SCOPA_ESTATE before a first completed call and a player outside {0, 1} as
 *                   scopa_full_mccfr_response_get.  A refused exploitability call leaves the rows of the call before it readable
 *   cfr_iterate   : (scopa_amd/csrc/scopa_full_chance_cfr.hip) n_iters exact, weighted CFR iterations on the sub-games below `root` on the handle's
 *                   OWN decks, the deal a uniform chance move: the bit-reproducible solver beside the sampled one, for the sub-games the
 *                   exploitability sweep measures.  root as for exploitability: a non-terminal round boundary that every handle deck fits (NULL =
 *                   the handle's root; its hands are ignored), R = 6 - root.round <= 4 and n_decks x 36^R <= 1 << 22.  h_w [n_iters][3] = (pos, neg,
 *                   strat) per iteration follows scopa_cfr_sync_iterate_weighted's contract literally: each weight finite and in [0, 1], the caller
 *                   owns t, the library computes no schedule; NULL = all 1.0 (vanilla CFR).  h_values [n_iters][2] (or NULL): the sweep values.
 *                   Checked in this order, each before any launch and with nothing changed: a NULL handle, n_iters outside [0, 1 << 20],
 *                   alternating outside {0, 1}, a weight that is not finite or lies outside [0, 1], a bad root: SCOPA_EINVAL; R > 4 or
 *                   n_decks x 36^R > 1 << 22: SCOPA_ELIMIT; a deck that does not fit the root: SCOPA_EINVAL.  n_iters = 0 is a no-op that claims
 *                   nothing.  The procedure defines the bits and tests/full_chance_cfr_ref.py restates it in float64:
 *                     1 forest   exactly step 1 of exploitability: deck-major, child a of g at g n_k + a, slot a the mover's a-th card in
 *                                ascending card id
 *                     2 claim    once per call every pair (A, B) of every choice level is claimed in the store (the claim of `slots` above).  A
 *                                claimed zero row reads as the absent row it replaces under every rule above; it counts in `rows` and appears in
 *                                tables_get.  If any claim is dropped the call returns SCOPA_ENOMEM with `dropped` raised and NOTHING computed: every
 *                                regret and strategy word of every row is unchanged, the zero rows already claimed stay.  A pair names its level
 *                                (player, round, popcount B), so a row belongs to exactly one level
 *                     3 sweep    with sigma frozen: prob[g][a] = regret matching of the pair's regret row (the which = 1 rule).  Two reaches top
 *                                down with w = 1.0 at every root: w1 multiplies by prob at player 1's choice levels only, w0 at player 0's only; for
 *                                traverser p, w_opp = w_(1-p) and w_own = w_p.  V bottom up as step 3 of exploitability: leaf r2_p0 / 2.0;
 *                                v = 0.0; v += prob[a] * child[a] in slot order.  The sweep's value is (0.0 + V[root 0] + V[root 1] + ...) / n in
 *                                deck order
 *                     4 update   of traverser p's rows, with x = V for p = 0 and -V for p = 1: for every pair K of p's levels and slot a < n,
 *                                dR[K][a] = 0.0; dR[K][a] += w_opp[g] * (x[child a of g] - x[g]) and dS[K][a] = 0.0; dS[K][a] += w_own[g] * prob[g][a]
 *                                over ALL forest nodes g of the level that hold K, on every deck, in ASCENDING g.  Then per cell R <- R + dR;
 *                                R <- !(R <= 0) ? R * pos : R * neg; S <- (S + dS) * strat.  Nothing is scaled by 1 / n.  One lane is a row's only
 *                                writer, with plain stores; no atomic touches a table word.  Slots at and above n stay 0.0
 *                     5 iteration alternating = 1: sweep + update of player 0's rows, then a fresh sweep (sigma from the new regrets) + update of
 *                                player 1's rows, h_values[t] = {value of sweep 0, value of sweep 1}.  alternating = 0: one sweep, both players'
 *                                rows updated from it, h_values[t] holds its value twice.  Iteration t uses h_w[t]
 *                     6 the rest rows whose pair is not in the forest are untouched (earlier rounds, other tables, other hands); d_regret,
 *                                d_strategy, the visit counts, choice_visits and terminal_visits are untouched.  The handle's iteration counter
 *                                advances by 2 per iteration, so MCCFR iterations that follow draw fresh Philox words.  iterate, traverse / apply,
 *                                match, exploitability, tables_get / _set and reset may precede or follow on the same handle in any order: the
 *                                set-up (forest, keys, the two sorts, the claim) is redone by every call and nothing of it is kept across calls
 *                     7 order    no float64 atomic anywhere: the same handle state gives the same bits.  One host synchronisation after the
 *                                claim (so that SCOPA_ENOMEM comes before anything is computed), none between iterations, one at the end, when
 *                                h_values is copied out and the rows are written back to their slots
 *                   IMPERFECT RECALL, as for exploitability: for R > 1 the pair forgets the player's own plays of earlier rounds, CFR has no
 *                   convergence proof on these rows, and the figure to watch is the lower bound (BR0 + BR1) / 2 of exploitability.  At R = 1 the
 *                   game below the root has perfect recall.
 *                   Scratch is one allocation kept in the handle, grown when a call needs more and freed by destroy (SCOPA_ENOMEM where the device
 *                   cannot hold it): with T = 31 n (36^R - 1) / 35 nodes about 192 T + 8 n 36^R + 80 x 18 n 36^(R-1) + 40 n_iters bytes plus the
 *                   sorts' own -- 0.9 GB at the cap
 *   cross_play    : (scopa_amd/csrc/scopa_full_chance_xplay.hip) store against store, exactly: for the K handles hs[0..K) -- a policy is a handle,
 *                   that is, its store -- h_out[a][b] holds, for hs[a] as player 0 against hs[b] as player 1, the expected reward of player 0
 *                   (r2_p0 / 2.0), the expected square of that reward, the expected terminal scopas[0] and the expected terminal scopas[1], on the
 *                   sub-games below `root` (NULL = hs[0]'s root) on the k decks h_decks (NULL = hs[0]'s decks, k ignored), the deal a uniform chance
 *                   move.  The policy of a store is a function of the pair (A, B) alone: the stores' own roots and decks do not matter and a handle
 *                   may appear more than once.  Synchronous; reads every store with the read-only probe only and leaves every handle's rows,
 *                   counters, increments, iteration counter, response rows and exploitability / cfr_iterate scratch alone.  Checked in this order,
 *                   each before any launch and with nothing changed (h_out included): hs or h_out NULL, K outside [1, 16], a NULL entry, handles
 *                   of different contexts, which outside {0, 1}, k < 1 with h_decks given, a bad root: SCOPA_EINVAL; R = 6 - root.round > 4,
 *                   k x 36^R > 1 << 22 or K x k x 36^R > 1 << 24: SCOPA_ELIMIT; a deck that fails create's check against that root: SCOPA_EINVAL.
 *                   The procedure defines the bits and tests/full_chance_xplay_ref.py restates it in float64:
 *                     1 forest   exactly step 1 of exploitability: deck-major, child a of g at g n_k + a, slot a the mover's a-th card in
 *                                ascending card id, the roots root_on(root, deck d).  A leaf carries r = r2_p0 / 2.0, r * r, (double)scopas[0] and
 *                                (double)scopas[1] of its terminal state
 *                     2 policy   for every handle j and every choice node prob_j[g][.] by step 2 of exploitability with `which`: uniform where the
 *                                pair is absent or the total is <= 1e-12 (which = 0), a slot whose word B is unpublished a zero row
 *                     3 value    for each ordered pair (a, b) and each quantity, bottom up v = 0.0; v += prob[g][s] * child[s] in slot order, prob =
 *                                prob_a at player 0's levels and prob_b at player 1's; a one-card node takes its child's value.
 *                                h_out[a][b][q] = (0.0 + V[root 0] + V[root 1] + ...) / n, added in deck order
 *                     4 order    no float64 atomic anywhere: the same handles, decks and order give the same bits
 *                   So h_out[a][a][0] is exploitability(hs[a], root, decks, which)'s value bit for bit, and h_out[a][b][0] is the value
 *                   exploitability reports on a store that holds hs[a]'s rows of player 0 and hs[b]'s of player 1 (bit 62 of A names the player).
 *                   Scratch is one allocation of its own kept in hs[0], grown when a call needs more and freed by destroy (SCOPA_ENOMEM where the
 *                   device cannot hold it): with E = k 36^R leaves and T = 31 k (36^R - 1) / 35 nodes about 24 K T + 52 E + max(16 K E,
 *                   (8 / 3) K^2 E) + 8 K^2 E bytes -- the K prob images of 24 bytes a node, two levels of states, the leaves packed in 4 bytes, and
 *                   V ([pair][quantity][node] doubles) for two levels at a time, the lowest level kept once per b -- 2.9 GB where K = 16 and
 *                   K E = 1 << 24
 *   pair_match    : (scopa_full_chance_xplay.hip) `match` with the opponent playing the average policy of h_b's store instead of uniform play: from
 *                   h_a's root (which may be the deal: the whole 36-ply game), the same seat rule, deck rule (j mod k), Philox counter
 *                   (i, i >> 32, stream_id << 8 | state.step, 208), fm_pick and probability rule (uniform where the pair is absent or the total is
 *                   <= 1e-12) for both players, the same six sums with "agent" = h_a and "opponent" = h_b.  One launch, a lane per episode, the one
 *                   episode body of `match` with the opponent's table as its parameter; reads both stores, never inserts.  Argument checks as for
 *                   match; h_b NULL or on another context: SCOPA_EINVAL.  With h_b holding none of the pairs met (an empty store) the sums and
 *                   h_r2_a equal match(h_a, ...)'s exactly.  h_a == h_b is allowed
 *   respond_traverse, respond_iterate, harden : (scopa_full_chance.hip) a SAMPLED BEST RESPONSE to a fixed store, from any root, the deal included.
 *                   h_resp is the responder's store and h_opp the fixed opponent's (NULL = uniform play).  What the hardened responder wins against
 *                   h_opp -- pair_match, or cross_play where the sub-game fits it -- is a LOWER BOUND on h_opp's exploitability that holds from any
 *                   root: the responder is a real key-pair policy, so the bound is achieved.  Checked before any launch, with nothing changed:
 *                   traverse's (iterate's) own checks with `responder` in traverser's place; h_opp on another context or h_opp == h_resp:
 *                   SCOPA_EINVAL; which outside {0, 1}: SCOPA_EINVAL.  h_opp's own root and decks do not matter (a store's policy is a function
 *                   of the pair): the walk runs on h_resp's root and decks.  h_opp's rows, increments, counters and iteration counter are left alone.
 *                     1 walk     traverse's walk (scopa_full_mccfr_walk.h, the same definition), launch geometry, cut and lists, with ONE
 *                                difference: at a node whose mover is not `responder` -- in the main walk and in the prefix replay of cut > 0 --
 *                                nothing of h_resp is claimed, written or counted.  The mover's pair is looked up in h_opp's table with the
 *                                read-only probe and its probabilities are, for which = 0, match's rule (strategy[a] / total where the pair is
 *                                held and total > 1e-12 over the n legal slots, else 1.0 / n) and, for which = 1, regret matching of h_opp's
 *                                regret row, an absent pair a zero row (so 1.0 / n); h_opp NULL: 1.0 / n.  Then fm_pick on the node's draw
 *                     2 rows     at the responder's nodes exactly traverse: the pair is claimed in h_resp, sigma is regret matching of its frozen
 *                                regrets, d_regret and the visit count take the atomics.  d_strategy is never written.  choice_visits and
 *                                terminal_visits of h_resp count every choice node and leaf walked, the opponent's included
 *                     3 draws    Philox counter (state.step << 16 | q, traversal id, iteration, deck_index << 8 | 144 + responder): traverse's
 *                                layout with a tag of its own, so list order, m and the cut change no draw
 *                     4 iterate  per iteration respond_traverse(0), apply, respond_traverse(1), apply at h_resp's iteration counter, b0 = 0,
 *                                nb = batch; the lists are uploaded once, no host synchronisation between iterations, one dropped check at the
 *                                end (SCOPA_ENOMEM where h_resp's store is full along a probe; the rows kept are right)
 *                     5 harden   a lane per slot: for every occupied slot strategy[a] = 1.0 where a is the FIRST maximal regret over the row's
 *                                popcount(B) slots and 0.0 at the other two; a slot whose word B is unpublished is skipped.  Regrets are untouched,
 *                                so training may go on and harden may be called again.  The response walk never adds into the strategy rows, so a
 *                                response store's strategy rows are only ever what harden left there; match, pair_match, cross_play and
 *                                exploitability then see the pure response unchanged.  Queued on the context's stream, no synchronisation
 *   respond_nets_traverse, respond_nets_iterate : (scopa_full_chance_sdcfr.hip) the SAMPLED BEST RESPONSE to the Deep CFR NETS' average policy, from
 *                   any round-boundary root (R = 1 .. 6, the deal included) on as many decks as h_resp holds -- where no store of the nets' policy
 *                   fits.  h_resp is the responder's store, as above; the fixed opponent is a snapshot set in sdcfr_match's form
 *                   (scopa_full_sdcfr_snapshots, below): traverse takes ONE, the set of player 1 - responder; iterate takes two, player 0's and
 *                   player 1's.  harden, match / pair_match / cross_play and sdcfr_match(opp_store = h_resp) then play the response.  Checked
 *                   before any launch, with nothing changed: respond_traverse's (respond_iterate's) own checks with `responder` in traverser's
 *                   place; responder outside {0, 1}; nb (batch) < 1; a list with a deck out of range or twice; traversal ids b0 + nb beyond 2^32;
 *                   a root that is no round boundary or a deck of h_resp that does not fit root_state; a NULL set or one that fails average_at's
 *                   checks; a scratch budget below one traversal's bytes: SCOPA_EINVAL.  An empty list (m = 0) is a no-op.
 *                     1 walk     it IS respond_traverse's walk at cut 0 with ONE substitution: at a node whose mover is not `responder` the
 *                                probabilities are the row of average_at at the node's key pair under match's rule (the total over the n legal
 *                                slots: row / total where total > 1e-12, else 1.0 / n) -- one rule, stated once (fw_row_probs), for a store's
 *                                row and the nets' --, then fm_pick on the node's draw.  No row of the opponent is claimed, written or counted;
 *                                the nets' tensors are only read.  n_snap = 0 is uniform play and equals respond_traverse(h_opp = NULL) at cut 0
 *                     2 rows     at the responder's nodes with n > 1 the pair is claimed in h_resp (a full probe: slot -1, dropped += 1, a zero
 *                                regret row, no write), sigma is regret matching of the row's frozen regrets, ALL n children are expanded (child a
 *                                of path p is path p n + a), on the way up v = sum of sigma[a] cfv[a] in slot order from 0.0 in float64, nothing
 *                                contracted, d_regret[a] += cfv[a] - v and count += 1 by the walk's float64 / uint32 atomics.  d_strategy is never
 *                                written.  A leaf is worth 0.5 r2_p0, negated for responder 1; the one-card plies are played through.
 *                                choice_visits and terminal_visits of h_resp count every choice node and leaf walked, the opponent's included: a
 *                                fixed function of R, the responder and the traversal count, added once per chunk
 *                     3 draws    Philox counter (state.step << 16 | q, b0 + i, iteration, deck_index << 8 | 144 + responder): respond_traverse's
 *                                draw, tag included, on purpose.  q is the path -- the responder's own slot choices in mixed radix -- and i the
 *                                traversal's index on its deck, so list order, m, chunking and launch geometry change no draw
 *                     4 iterate  per iteration respond_nets_traverse(0), apply, respond_nets_traverse(1), apply at h_resp's iteration counter and
 *                                h_resp's root, b0 = 0, nb = batch; the lists are uploaded once, no host synchronisation between iterations, one
 *                                dropped check at the end (SCOPA_ENOMEM where h_resp's store is full along a probe; the rows kept are right)
 *                     5 launches per chunk of C traversals (g = slot nb + i, as traverse_frontier numbers them), node (t, p) of level k at element
 *                                t W_k + p: the roots; per choice level going down, at a responder level a launch with a lane per node (claim,
 *                                sigma, (slot, sigma[3]) kept per row) and one with a lane per child, at a level of the other player average_at
 *                                over the level's C W_k contiguous pairs (skipped without snapshots) and a launch with a lane per node (draw, pick,
 *                                step, the child's state and pair); per responder level going up a launch with a lane per row.  Per path two
 *                                64-byte states, the pair, the 24-byte average row and two float64 values, per responder row the slot and sigma
 *                                (184 and 28 bytes), in traverse_frontier's block behind the slot lists; traversals pass through it in chunks of
 *                                at most 1 GiB (debug_sdcfr_scratch), and a chunk seam changes no draw and no row
 * Every entry point but infoset_key_wide returns SCOPA_EINVAL for a NULL handle before it touches the device. */
typedef struct scopa_full_chance scopa_full_chance;
int32_t scopa_full_infoset_key_wide(const scopa_full_state *s, int32_t player, uint64_t key2[2]);
int32_t scopa_full_chance_create(scopa_ctx *ctx, const uint8_t *decks /*[n_decks][40]*/, int32_t n_decks, const scopa_full_state *root_state /*NULL = the deal*/,
                                 int32_t capacity_log2, scopa_full_chance **out);
int32_t scopa_full_chance_destroy(scopa_full_chance *h);
int32_t scopa_full_chance_root(const scopa_full_chance *h, scopa_full_state *root, uint8_t *decks /*[n_decks][40]*/, int32_t *n_decks, int32_t *capacity_log2);
int32_t scopa_full_chance_cut(scopa_full_chance *h, int32_t cut);
int32_t scopa_full_chance_reset(scopa_full_chance *h);
int32_t scopa_full_chance_traverse(scopa_full_chance *h, int32_t traverser, uint32_t iteration, uint32_t b0, uint32_t nb, const int32_t *h_list /*[m] or NULL = all*/, int32_t m);
int32_t scopa_full_chance_apply(scopa_full_chance *h);
int32_t scopa_full_chance_iterate(scopa_full_chance *h, uint32_t batch, uint32_t n_iters, const int32_t *h_lists /*[n_iters][m] or NULL*/, int32_t m);
int32_t scopa_full_chance_counters(scopa_full_chance *h, uint64_t *choice_visits, uint64_t *terminal_visits, uint64_t *rows, uint64_t *dropped, uint32_t *iterations);
int32_t scopa_full_chance_tables_get(scopa_full_chance *h, int64_t *n_rows, uint64_t *keys2 /*[n_rows][2]*/, int32_t *n_act, double *regret /*[n_rows][3]*/, double *strategy /*[n_rows][3]*/);
int32_t scopa_full_chance_delta_get(scopa_full_chance *h, int64_t *n_rows, uint64_t *keys2 /*[n_rows][2]*/, double *d_regret /*[n_rows][3]*/, double *d_strategy /*[n_rows][3]*/, uint32_t *counts);
int32_t scopa_full_chance_tables_set(scopa_full_chance *h, int64_t n_rows, const uint64_t *keys2, const int32_t *n_act, const double *regret, const double *strategy);
int32_t scopa_full_chance_match(scopa_full_chance *h, int64_t n_episodes, uint32_t stream_id, const uint8_t *h_decks /*[k][40] or NULL = the handle's*/, int32_t k,
                                int64_t h_sums[6], int8_t *h_r2_agent /*[n_episodes] or NULL*/);
int32_t scopa_full_chance_exploitability(scopa_full_chance *h, const scopa_full_state *root /*NULL = the handle's root*/,
                                         const uint8_t *h_decks /*[k][40] or NULL = the handle's decks*/, int32_t k,
                                         int32_t which /*0 = average policy, 1 = current regret-matching sigma*/, double h_out4[4]);
int32_t scopa_full_chance_response_get(scopa_full_chance *h, int32_t player, int64_t *n_rows, uint64_t *keys2 /*[n_rows][2]*/,
                                       int32_t *n_act, int32_t *action, double *q /*[n_rows][3]*/);
int32_t scopa_full_chance_cfr_iterate(scopa_full_chance *h, const scopa_full_state *root /*NULL = the handle's root*/,
                                      int32_t n_iters, const double *h_w /*[n_iters][3] = (pos, neg, strat); NULL = all 1.0*/,
                                      int32_t alternating, double *h_values /*[n_iters][2] or NULL*/);
int32_t scopa_full_chance_cross_play(scopa_full_chance *const *hs, int32_t K, const scopa_full_state *root /*NULL = hs[0]'s root*/,
                                     const uint8_t *h_decks /*[k][40] or NULL = hs[0]'s decks*/, int32_t k,
                                     int32_t which /*0 = average policy, 1 = current regret-matching sigma*/, double *h_out /*[K][K][4]*/);
int32_t scopa_full_chance_pair_match(scopa_full_chance *h_a, scopa_full_chance *h_b, int64_t n_episodes, uint32_t stream_id,
                                     const uint8_t *h_decks /*[k][40] or NULL = h_a's decks*/, int32_t k, int64_t h_sums[6],
                                     int8_t *h_r2_a /*[n_episodes] or NULL*/);
int32_t scopa_full_chance_respond_traverse(scopa_full_chance *h_resp, scopa_full_chance *h_opp /*NULL = uniform play*/,
                                           int32_t which /*0 = h_opp's average policy, 1 = its current regret-matching sigma*/, int32_t responder,
                                           uint32_t iteration, uint32_t b0, uint32_t nb, const int32_t *h_list /*[m] or NULL = all*/, int32_t m);
int32_t scopa_full_chance_respond_iterate(scopa_full_chance *h_resp, scopa_full_chance *h_opp /*NULL = uniform play*/, int32_t which, uint32_t batch,
                                          uint32_t n_iters, const int32_t *h_lists /*[n_iters][m] or NULL*/, int32_t m);
int32_t scopa_full_chance_harden(scopa_full_chance *h);
typedef struct scopa_full_sdcfr_snapshots scopa_full_sdcfr_snapshots;   /* one player's snapshots, defined with the Deep CFR block below */
int32_t scopa_full_chance_respond_nets_traverse(scopa_full_chance *h_resp, const scopa_full_state *root_state /*NULL = h_resp's root*/, int32_t responder,
                                                uint32_t nb, const int32_t *h_list /*[m] or NULL = all*/, int32_t m,
                                                const scopa_full_sdcfr_snapshots *opponent /*ONE set: player 1 - responder's*/, uint32_t iteration, uint32_t b0);
int32_t scopa_full_chance_respond_nets_iterate(scopa_full_chance *h_resp, const scopa_full_sdcfr_snapshots *nets /*[2]: player 0's, player 1's*/, uint32_t batch,
                                               uint32_t n_iters, const int32_t *h_lists /*[n_iters][m] or NULL*/, int32_t m);

/* ---- Deep CFR on FullScopa over a set of decks (scopa_amd/csrc/scopa_full_chance_sdcfr.hip, scopa_full_sdcfr_tile.h; the counterparts are the
 * scopa_chance_sdcfr_* and scopa_team_chance_sdcfr_* blocks).  traverse and average_policy run on the sub-games the exact sweeps cover: a
 * round-boundary root with R = 6 - root.round <= 4 rounds to go and n_decks x 36^R <= 1 << 22; traverse_frontier has neither limit.  The advantage net's input is a function of the mover's key pair (A, B) alone, so one net per player
 * serves every deck and is defined at keys of decks it never trained on.
 *   features      96 float32, every value dyadic and so exact: [0, 40) the hand, one-hot by card id (word B) -- this IS the legal-action mask --,
 *                 [40, 80) the table, multi-hot by card id (A bits 16..55), [80, 86) the round, one-hot, 86 the mover's captured-card field / 64,
 *                 87 and 88 the mover's scopas / 32 and the opponent's scopas / 32, 89 = 1.0 if the player bit 62 is set, [90, 96) = 0.
 *                 sdcfr_features: host code, no GPU; n < 0 or a NULL array with n > 0: SCOPA_EINVAL
 *   net           one per player: an MLP 96-128-64-40 with ReLU, weights in torch layout W[out][in], float32; output c is the advantage of playing
 *                 card id c.  The traversal takes six device pointers, each to the two players' tensors one after the other: d_w1 [2][128][96],
 *                 d_b1 [2][128], d_w2 [2][64][128], d_b2 [2][64], d_w3 [2][40][64], d_b3 [2][40].  A unit's terms are accumulated in ONE fixed order
 *                 (scopa_full_sdcfr_tile.h: from the bias, inputs in ascending blocks of four on v_mfma_f32_16x16x4_f32; layer 1 never reads W1's
 *                 columns 92..95, whose inputs are 0 by definition), and a node's result depends on its own key and the weights alone, so one net
 *                 gives one set of bits whatever the grid, the list or the chunking
 *   policy        positive_regret_policy over the node's n <= 3 held cards in ASCENDING CARD ID, the slot order of the store: x[s] = adv[card s] where
 *                 that is > 0, else 0; z = (x[0] + x[1]) + x[2] in float32; policy[s] = x[s] / max(z, float32(1e-8)); zeros beyond n.  Thresholds
 *                 follow scopa_sdcfr's definition: sum = the float32 sum of the policy left to right; sum == 0: thr[0] = ~0; else with the float64
 *                 running sums cdf_k of (double)(policy[k] / sum), thr[k] = ceil(cdf_k / cdf_(n-1) * 2^53) for k < n - 1 and 2^53 for the rest of
 *                 thr[2].  A draw N = u53's 53-bit integer picks slot (thr[0] <= N) + (thr[1] <= N), at most n - 1; with thr[0] = ~0 it picks
 *                 (int)(N 2^-53 n) in float64
 *   set-up        once per (root, handle decks), kept in the handle until another root is asked for and freed by destroy: the deck-major forest of
 *                 `exploitability` step 1 over ALL the handle's decks; per choice node its key pair, the leaves as float32 r2_p0 / 2; no states are
 *                 kept.  With T = 31 n (36^R - 1) / 35 choice nodes: 16 T + 4 n 36^R bytes, and the tables 12 T + 16 T
 *   traverse      `batch` external-sampling traversals of `traverser` on each listed deck (h_list [m] deck indices, distinct and in range; NULL with
 *                 m = 0 or n_decks: every deck) below `root` (NULL = the handle's root), two launches, no atomics, no host synchronisation once the
 *                 forest is built.  First EVERY choice node of the listed decks' trees is evaluated under the net of its mover (policy and
 *                 thresholds, above).  Then each traversal walks the forest by index arithmetic: child a of node g of level k is g n_k + a; the
 *                 traverser's levels branch into every slot; at the other player's levels ONE slot is drawn with Philox4x32-10 under
 *                 scopa_mccfr_seed's key at counter (level << 24 | g, traversal id, iteration, 224 + traverser), g the node's index in its level of
 *                 the HANDLE's forest (deck-major over all handle decks); traversal i of deck d has id b0 + d * batch + i.  So list order, m and the
 *                 launch's geometry (how it cuts the batch across workgroups) change no draw and no row.  The id holds the call's `batch`: a
 *                 caller who splits a batch over two calls of a smaller `batch` gets other ids on every deck but deck 0, whatever b0 it passes.  A leaf is worth r2_p0 / 2, negated for traverser 1; a traverser node's
 *                 value is v = 0; v = v + policy[s] * cfv[s] in float32, slot order, every operation rounded; the other player's nodes hand their
 *                 child's value on; the root's value goes to d_root_values[slot * batch + i], slot the deck's position in the list.
 *                 Every traverser choice node writes one memory row, ROWS(R) = 4 (6^R - 1) / 5 per traversal (4, 28, 172, 1 036), at ring position
 *                 (write_base + ROWS * (slot * batch + i) + rank) % capacity; rank is level-major: the traverser's levels in ascending order, within
 *                 a level the nodes in ascending path (the mixed-radix number of the traverser's own slot choices so far).  A row is the node's 96
 *                 features into d_mem_feat [capacity][96] and 40 regrets into d_mem_regret [capacity][40]: with cfv[c] = 0 at cards not held,
 *                 d[c] = cfv[c] - v over all 40 cards, then d / (max|d| + float32(1e-8)) when the maximum is positive -- scopa_sdcfr_backward's
 *                 arithmetic over 16 slots and the reference's add_experience rule, carried to 40 cards.  The mask is feat[0..40) and is not stored.
 *                 ONE-CARD MOVERS leave no row and draw nothing: the forest numbers only choice levels, as the MCCFR walk does.  The reference's
 *                 traversal would have written a row at the traverser's one-card nodes too.
 *                 Refusals, each before any launch and with nothing written: a NULL handle, traverser outside {0, 1}, a bad root: SCOPA_EINVAL;
 *                 R > 4 or n_decks x 36^R > 1 << 22: SCOPA_ELIMIT; a handle deck that does not fit the root, a bad list, batch outside
 *                 [1, 1 << 24], a NULL device pointer, d_mem_feat or d_mem_regret not 16-byte aligned, capacity outside [ROWS, 2^30), write_base
 *                 outside [0, capacity), ROWS * m * batch > capacity, b0 + n_decks * batch > 2^32: SCOPA_EINVAL.
 *                 iterate, cfr_iterate, exploitability, cross_play, match and the tables calls are unaffected, may be interleaved and keep their bits:
 *                 nothing here reads or writes the store or the handle's counters
 *   visits        choice-node visits of all traversals since create, counted on the host from the fixed shape: with S = (6^R - 1) / 5 a traversal
 *                 makes 13 S as traverser 0 and 8 S as traverser 1
 *   policy_get    for tests: the tables of the forest at hand over ALL T choice nodes, level-major and deck-major within a level: policy [T][3],
 *                 thresholds [T][2], key pairs [T][2].  Entries of decks the last call did not list are those an earlier call left (zero before
 *                 any).  *n_nodes: room in, T out; every array NULL: T only; less room: SCOPA_EINVAL.  SCOPA_ESTATE before a first traversal call on
 *                 the forest at hand
 *   average_policy for `player`, the n_snap snapshots h_slots[0..n_snap) (FIFO order) of the six tensors [max_size][...] with the float32
 *                 coefficients d_coef[n_snap]: the policy launch once per snapshot in that order with acc[g][s] = acc[g][s] + coef * p[g][s] in float32,
 *                 then in float64 sum = (acc[0] + acc[1]) + acc[2] over the legal slots and acc[s] / sum, uniform 1 / n where the sum is 0 or not
 *                 finite -- scopa_chance_sdcfr_average_policy's definition; n_snap = 0 gives the uniform policy.  On the handle's decks (h_decks
 *                 NULL) or on h_decks [k][40] that fit the root, for which a forest of the call's own is built and freed.  Returns per choice node of
 *                 the player's levels, level-major and deck-major, the key pair h_keys2 [N][2] and h_policy [N][3]; nodes that share a pair carry
 *                 equal bits.  *n_rows: room in, N out; both arrays NULL: N only.  Synchronous.  Refusals as traverse's, in the same order
 *   debug_sdcfr   a benchmark hook on the context: launches = 0 (the default) both launches of a traverse call, 1 the policy launch alone (no row, no
 *                 visit), 2 the walk launch alone over the tables as an earlier call on the forest left them (SCOPA_ESTATE without one); anything
 *                 else: SCOPA_EINVAL
 *   policy_at     the policy launch on a caller's list: d_keys2 [n][2] key pairs (device, 16-byte aligned), all of mover `player`, under that player's
 *                 net of the six tensors [2][...]: policy [n][3] and thresholds [n][2] by the net, the K order, the regret matching and the threshold
 *                 rule above, the held cards counted from word B.  A pair's result depends on the pair and the weights alone: where the pair
 *                 occurs in a forest the bits are policy_get's, and list order, duplicates and n % 16 change no bit.  One launch on the context's
 *                 stream, no host synchronisation; n = 0: nothing is done.  A NULL context, player outside {0, 1}, n outside [0, 1 << 28], a NULL or
 *                 misaligned pointer with n > 0: SCOPA_EINVAL before any launch
 *   traverse_frontier  traverse's contract -- arguments, draws' 53-bit integer and slot rule, rows, ranks, ring positions, float32 arithmetic, root
 *                 values, visits -- WITHOUT a forest: any round-boundary root the handle's decks fit, R = 1 .. 6 (NULL: the handle's root, which may be
 *                 the deal), any deck count a handle holds; no SCOPA_ELIMIT.  ROWS(5) = 6 220, ROWS(6) = 37 324.  The handle's forest, where one
 *                 exists, is neither built, read nor freed.  A node of a traversal is (choice level k, path p), p the mixed-radix number of the
 *                 traverser's own slot choices so far (the root: 0); the traverser's levels send slot a to path p n_k + a, the other player's draw
 *                 ONE slot and keep p; the two one-card plies behind a round's last choice level are played through.  Level k of a traversal is a
 *                 dense array of W_k <= 6^R paths: children and parents are index arithmetic, no compaction, no atomics.  Draws: Philox4x32-10
 *                 under scopa_mccfr_seed's key at counter (k << 24 | p, traversal id, iteration, 240 + traverser), the id b0 + d * batch + i with d
 *                 the deck's index in the handle: named by the PATH, not by a forest's node, so the two forms draw differently and agree in
 *                 distribution only.  Per chunk of traversals: one small launch for the roots, then per choice level the policy_at launch over the
 *                 level's key pairs and an expand launch (a lane per child: the draw, the step, the child's state and key pair, or the leaf's value),
 *                 then per traverser level from the last to the first one launch that restates v and the regrets per 16-byte piece of the row and
 *                 writes features, regrets and the value handed up.  Level states (two buffers), one level's key pairs, policy and thresholds, two
 *                 value buffers and the rows' key pairs and policies live in ONE block owned by the handle, 180 x 6^R + 28 ROWS bytes a traversal,
 *                 reused across calls, grown where needed, freed by destroy; the call's m x batch traversals pass through it in chunks of at most
 *                 1 GiB (debug_sdcfr_scratch), which changes no bit.  No host synchronisation unless the block grows.  Refusals: traverse's
 *                 SCOPA_EINVAL list, and a budget below one traversal's bytes, each before any launch with nothing written
 *   debug_sdcfr_scratch  a test hook on the context: the bytes a chunk of traverse_frontier may take (0 = the default, 1 GiB), so that chunk seams
 *                 can be forced at small shapes; bytes < 0: SCOPA_EINVAL
 *   average_at    average_policy's rows on a caller's list: d_keys2 [n][2] key pairs (device, 16-byte aligned), all of mover `player`, and that
 *                 player's snapshots as average_policy takes them -> d_policy [n][3] float64 (device).  Row j carries the bits average_policy
 *                 writes for a forest node with pair j: acc = 0; per snapshot in FIFO order acc[s] = acc[s] + coef[i] * p_i[s] in float32, one
 *                 rounded product and one rounded sum (the forest route's two instructions), p_i the policy above under snapshot h_slots[i]; then in
 *                 float64 sum = (acc[0] + acc[1]) + acc[2] over the held cards, acc[s] / sum where the sum is positive and finite, else 1 / n_held;
 *                 0 beyond the held cards, which are counted from word B as policy_at counts them.  n_snap = 0: every row is 1 / n_held.
 *                 ONE launch whatever n_snap: a workgroup owns a fixed share of the list's 16-pair tiles, takes them 32 at a time and, per such
 *                 batch, loops over the snapshots in FIFO order -- the snapshot's register slices, then the batch's tiles under it -- with the
 *                 accumulators in LDS of its own (one writer each: no atomics, no order between workgroups).  The grid: a workgroup per tile until
 *                 every compute unit has one, up to four tiles each from there, then two workgroups per compute unit until each holds 32 tiles,
 *                 then more workgroups (eight per compute unit at most) -- a short list gets few workgroups and is cut for latency, a long one
 *                 amortises the reload.  List order, duplicates, n % 16 and the grid change no bit.  On the context's
 *                 stream, no host synchronisation unless the slot list outgrows the context's copy; n = 0: nothing is done.  A NULL context,
 *                 player outside {0, 1}, n outside [0, 1 << 28], n_snap outside [0, max_size], and with n_snap > 0 a NULL or misaligned tensor, a
 *                 NULL slot list or coefficients, a slot outside [0, max_size); with n > 0 a NULL or misaligned d_keys2 or d_policy: SCOPA_EINVAL
 *                 before any launch
 *   debug_sdcfr_average_grid  a test and benchmark hook on the context: the workgroups of every average_at launch, the match's included (at most one
 *                 per tile; 0 = the rule above), so that the work split -- several tiles a workgroup, ragged shares, more than one batch -- can be
 *                 forced at small lists and the rule's sweep recorded; it changes no bit.  A NULL context or workgroups < 0: SCOPA_EINVAL
 *   sdcfr_match   match's seat-swapped sampled episodes from the handle's root (which may be the deal) with the nets' AVERAGE POLICY in the
 *                 agent's seats: the agent plays agent[0] (player 0's snapshots) in seat 0 and agent[1] in seat 1.  Seat rule, deck rule (j mod k),
 *                 Philox counter (i, i >> 32, stream_id << 8 | state.step, 208), fm_pick and the six sums are match's.  At a choice node the
 *                 agent's probabilities are average_at's row under match's rule: total = the sum of its first n_held entries, row / total where
 *                 total > 1e-12, else uniform -- so on a sub-game the sweeps cover an episode equals, bit for bit, the same episode of match on a
 *                 store that holds average_policy's rows.  The opponent plays uniformly (opp_store and opp_nets NULL), a store's average policy as
 *                 pair_match reads it (opp_store, on the same context), or a second pair of snapshot sets (opp_nets[2]) under the agent's rule.
 *                 Episodes are level-synchronous: per chunk one launch for the roots, then per choice level of the 4 R -- mover k & 1 -- average_at
 *                 over the key pairs of the chunk's episodes whose mover is the agent (the episodes of seat k & 1, a contiguous part of the chunk:
 *                 no compaction), the same over the other part where the opponent is a set of nets, and ONE step launch with a lane per episode:
 *                 the probabilities, the draw, the pick, the step, the two one-card plies behind a round's last choice level, the child's state and
 *                 its mover's key pair; behind the last level the integer atomics of the sums.  At most 1 + 3 x 4 R launches a chunk, whatever
 *                 n_snap and n_episodes; no float atomics.  Two state buffers, key pairs, policy rows, a trace row and r2 per episode (200 bytes)
 *                 live in traverse_frontier's block behind the slot lists and the held-out decks; episodes pass through it in chunks of at most 1 GiB
 *                 (debug_sdcfr_scratch); episode ids are global, so chunking changes no bit.  h_trace[i][l] is the slot episode i chose at choice
 *                 level l of the WHOLE game (l = 4 round + level in the round), -1 at levels above the root.  Synchronous.  Refusals, each with
 *                 h_sums untouched and nothing launched: a NULL handle (before the device is touched), match's argument checks and its held-out-deck
 *                 check against the root, a NULL agent, both kinds of opponent at once, an opponent store of another context, a snapshot set that
 *                 fails average_at's checks (NULL weights with n_snap > 0 among them), a budget below one episode's bytes: SCOPA_EINVAL */
#define SCOPA_FULL_SDCFR_FEATURES 96
#define SCOPA_FULL_SDCFR_ACTIONS 40
int32_t scopa_full_chance_sdcfr_features(const uint64_t *keys2 /*[n][2]*/, int64_t n, float *feat /*[n][96]*/);
int32_t scopa_full_chance_sdcfr_traverse(scopa_full_chance *h, const scopa_full_state *root /*NULL = the handle's root*/, int32_t traverser, int32_t batch,
                                         int32_t m, const int32_t *h_list /*[m]; NULL (m = 0) = all decks*/, const float *d_w1, const float *d_b1,
                                         const float *d_w2, const float *d_b2, const float *d_w3, const float *d_b3, float *d_mem_feat /*[capacity][96]*/,
                                         float *d_mem_regret /*[capacity][40]*/, int64_t capacity, int64_t write_base, float *d_root_values /*[m * batch]*/,
                                         uint32_t iteration, uint32_t b0);
int32_t scopa_full_chance_sdcfr_traverse_frontier(scopa_full_chance *h, const scopa_full_state *root /*NULL = the handle's root*/, int32_t traverser,
                                                  int32_t batch, int32_t m, const int32_t *h_list /*[m]; NULL (m = 0) = all decks*/, const float *d_w1,
                                                  const float *d_b1, const float *d_w2, const float *d_b2, const float *d_w3, const float *d_b3,
                                                  float *d_mem_feat /*[capacity][96]*/, float *d_mem_regret /*[capacity][40]*/, int64_t capacity,
                                                  int64_t write_base, float *d_root_values /*[m * batch]*/, uint32_t iteration, uint32_t b0);
int32_t scopa_full_chance_sdcfr_policy_at(scopa_ctx *ctx, int32_t player, const uint64_t *d_keys2 /*[n][2]*/, int64_t n, const float *d_w1, const float *d_b1,
                                          const float *d_w2, const float *d_b2, const float *d_w3, const float *d_b3, float *d_policy /*[n][3]*/,
                                          uint64_t *d_thr /*[n][2]*/);
int32_t scopa_full_chance_sdcfr_visits(scopa_full_chance *h, uint64_t *choice_visits);
int32_t scopa_full_chance_debug_sdcfr(scopa_ctx *ctx, int32_t launches);
int32_t scopa_full_chance_debug_sdcfr_scratch(scopa_ctx *ctx, int64_t bytes);
int32_t scopa_full_chance_sdcfr_policy_get(scopa_full_chance *h, int64_t *n_nodes, float *h_policy /*[T][3] or NULL*/, uint64_t *h_thr /*[T][2] or NULL*/,
                                           uint64_t *h_keys2 /*[T][2] or NULL*/);
int32_t scopa_full_chance_sdcfr_average_policy(scopa_full_chance *h, const scopa_full_state *root /*NULL = the handle's root*/,
                                               const uint8_t *h_decks /*[k][40] or NULL = the handle's decks*/, int32_t k, int32_t player, int32_t n_snap,
                                               const float *d_w1, const float *d_b1, const float *d_w2, const float *d_b2, const float *d_w3, const float *d_b3,
                                               const int32_t *h_slots /*[n_snap]*/, int32_t max_size, const float *d_coef /*[n_snap]*/, int64_t *n_rows,
                                               uint64_t *h_keys2 /*[N][2]*/, double *h_policy /*[N][3]*/);
typedef struct scopa_full_sdcfr_snapshots {   /* one player's snapshots, as average_policy takes them */
    int32_t n_snap, max_size;
    const float *d_w1, *d_b1, *d_w2, *d_b2, *d_w3, *d_b3;   /* device, [max_size][...] each */
    const int32_t *h_slots;                                  /* host, [n_snap], FIFO order */
    const float *d_coef;                                     /* device, [n_snap] */
} scopa_full_sdcfr_snapshots;
int32_t scopa_full_chance_sdcfr_average_at(scopa_ctx *ctx, int32_t player, const uint64_t *d_keys2 /*[n][2]*/, int64_t n, int32_t n_snap, const float *d_w1,
                                           const float *d_b1, const float *d_w2, const float *d_b2, const float *d_w3, const float *d_b3,
                                           const int32_t *h_slots /*[n_snap]*/, int32_t max_size, const float *d_coef /*[n_snap]*/, double *d_policy /*[n][3]*/);
int32_t scopa_full_chance_debug_sdcfr_average_grid(scopa_ctx *ctx, int32_t workgroups);
int32_t scopa_full_chance_sdcfr_match(scopa_full_chance *h, int64_t n_episodes, uint32_t stream_id, const uint8_t *h_decks /*[k][40] or NULL = the handle's*/,
                                      int32_t k, const scopa_full_sdcfr_snapshots *agent /*[2]: player 0's, player 1's*/, scopa_full_chance *opp_store /*or NULL*/,
                                      const scopa_full_sdcfr_snapshots *opp_nets /*[2] or NULL*/, int64_t h_sums[6], int8_t *h_r2_agent /*[n_episodes] or NULL*/,
                                      int8_t *h_trace /*[n_episodes][24] or NULL*/);

/* ---- Team MiniScopa TPI: 2 teams x 2 seats on the 16-card deck, 16 plies (src/envs/team_mini_scopa_game.py,
 * src/envs/openspiel_team_mini_scopa.py) -- state engine ------------------------------------------------------------------
 * The reference trains nothing on it, but registers it as a two-player zero-sum game, so its generic CFRTrainer runs on it unmodified
 * (SURVEY §8f-4); provided: the state protocol, the batched device step, device playouts, and -- below -- that solver for one fixed deal.
 * The "player" of the TPI game is the TEAM (coordinator) of the seat to move; seats 0,1 = team 0, seats 2,3 = team 1. */
typedef struct scopa_team_state {   /* 40 bytes */
    uint64_t history;      /* nibble i = action of ply i (TPIMiniScopaState.action_history)                    */
    uint32_t table;        /* ordered table, nibble list (at most 8: table ranks are always distinct)          */
    uint16_t hand[4];      /* ordered hands                                                                    */
    uint16_t cap[4];       /* captured cards per seat, 16-bit masks                                            */
    uint8_t  nh[4];
    uint8_t  scopas[4];
    uint8_t  nt, step, last_capture_team /* 0xFF = None */, flags /* bit 0 terminal, bit 1 table overflow */;
} scopa_team_state;
int32_t scopa_team_state_init(const uint8_t perm16[16], scopa_team_state *out);               /* TeamMiniScopaGame.reset :68-78 */
int32_t scopa_team_state_step(scopa_team_state *s, int32_t action);                           /* apply_action / env.step :173-201 */
int32_t scopa_team_state_legal(const scopa_team_state *s, int32_t out[4], int32_t *n);        /* legal_actions, openspiel_team…:52-86 */
int32_t scopa_team_state_rewards_x2(const scopa_team_state *s, int32_t r2_seat[4]);           /* evaluate_game :125-155, x2 */
int32_t scopa_team_state_infoset_string(const scopa_team_state *s, int32_t team, char *buf, int32_t cap); /* :119-146 */
/* d_states[i] <- step(d_states[i], d_actions[i]) */
int32_t scopa_team_step_batch(scopa_ctx *ctx, scopa_team_state *d_states, const uint8_t *d_actions, int64_t n);
int32_t scopa_team_step_batch_host(scopa_ctx *ctx, scopa_team_state *h_states, const uint8_t *h_actions, int64_t n);
/* n_games uniform-random playouts to the end, one lane per game, dealt ON DEVICE from seeds[i] (CPython shuffle);
 * h_r2_team0[n] = reward x2 of team 0 (team 1 = negation), h_scopas[n][4] per seat.  Philox stream (ctx seed, game, ply). */
int32_t scopa_team_random_playouts(scopa_ctx *ctx, const int64_t *h_seeds, int64_t n_games, int8_t *h_r2_team0, uint8_t *h_scopas);

/* ---- Team MiniScopa TPI solved for one fixed deal: exact CFR, best response, minimax ------------------------------------------
 * stands behind CFRTrainer(TPIMiniScopaGame()) : src/algorithms/vanilla_cfr.py:41-120 run on src/envs/openspiel_team_mini_scopa.py.
 * The tree is regular: ply k is played by seat k & 3 from a hand of 4 - (k >> 2) cards (legal_actions :52-95), always 16 plies.  Depths 0..11 hold
 * SCOPA_TEAM_N_CHOICE nodes with a real choice; depths 12..15 are forced (one card left), so each of the SCOPA_TEAM_N_LEAVES depth-12 nodes stands
 * for its forced tail and its terminal.  The information-state string ends in the whole action history (:138-168): for a fixed deal every node is
 * its own infoset, SCOPA_TEAM_N_INFOSETS = choice nodes + 4 x depth-12 nodes.
 *   rows          : level-major, row = level offset + mixed-radix path of legal-action INDICES (hand positions), first ply most significant; the
 *                   children of node j of depth d are j * b + c, b = 4 - (d >> 2).  Level offsets 0, 1, 5, 21, 85, 341, 1 109, 3 413, 10 325,
 *                   31 061, 72 533, 155 477; depth-12 node = the same path, 0 .. 331 775
 *   tables        : [SCOPA_TEAM_N_CHOICE][4] float64 regret_sum, strategy_sum and local_strategy (InfoNode, vanilla_cfr.py:8-21), rows padded
 *                   with 0; reset state: sums 0, local_strategy uniform.  leaf_reach_sum [2][SCOPA_TEAM_N_LEAVES]: a forced node of team p keeps
 *                   regret_sum [0.] and local_strategy [1.], and its strategy_sum is the sum over team p's traversals of p's reach at its
 *                   depth-12 ancestor -- that one number per (team, depth-12 node) stands for all 1 327 104 forced InfoNodes.  Any pointer of
 *                   tables_get / tables_set may be NULL
 *   set_deal      : builds the payoffs on the device (one lane per depth-12 node: 16 steps from the root, the path's digits taken from the index)
 *                   and puts the tables in their reset state.  The team state lives in the context next to the MiniScopa deal: scopa_set_deal
 *                   does not touch it, scopa_team_set_deal does not touch the MiniScopa deal, scopa_ctx_destroy frees it
 *   tree_leaves   : h_r2[SCOPA_TEAM_N_LEAVES] int8, reward x2 of team 0 (evaluate_game, team_mini_scopa_game.py:125-155; team 1 = negation)
 *   cfr_iterate   : n_iters iterations of "for p in (0, 1): _cfr_recursive(root, p, 1.0, 1.0)" (vanilla_cfr.py:56-99, :108-110).  Every infoset has one
 *                   node, so the recursion with its mid-traversal local_strategy refresh (:97) is a level-synchronous sweep: reaches down as
 *                   running products from the root (:83-85), values up as np.sum(local_strategy * action_utils) left to right (:87), the
 *                   traverser's rows regret_sum += opp_reach * (action_utils - value), strategy_sum += reach * local_strategy (:93-95), then
 *                   every row's local_strategy <- get_strategy() (:23-30).  h_w NULL: the reference bit for bit.  Else h_w[n_iters][3] = (pos, neg,
 *                   strat), scopa_cfr_sync_iterate_weighted's contract with alternating = 1, applied to the traverser's rows and (strat only) to
 *                   its leaf_reach_sum: R <- R + dR; R <- !(R <= 0) ? R * pos : R * neg; S <- (S + dS) * strat.  Every weight finite and in
 *                   [0, 1], n_iters <= 1 << 20 (else SCOPA_EINVAL, nothing launched or changed); 0 is a no-op; (1, 1, 1) gives the NULL path's bits.
 *                   The caller owns t.  h_root_values[n_iters][2] (or NULL): the two traversals' root values.  Two launches per traversal:
 *                   256 workgroups sweep the depth-4 subtrees through LDS (80 648 bytes), one workgroup finishes depths 3..0.  No float64
 *                   atomics, one writer per row: bit-identical from run to run
 *   value passes  : one upward sweep with a mode per team -- follow a table (rows used as given, v = 0.0; v += row[c] * child[c], children left
 *                   to right) or maximise (the child best for the mover's own team by a strict `>`, ties to the lowest action; with one node per
 *                   infoset the per-node maximum is the best response everywhere, reachable or not) -- in the same two-launch cut.  Policy
 *                   tables are [SCOPA_TEAM_N_CHOICE][4] float64 DEVICE tables, 32-byte aligned (else SCOPA_EINVAL)
 *   exploitability: d_policy or NULL = the average policy (InfoNode.policy, vanilla_cfr.py:32-39: strategy_sum normalised, uniform where its
 *                   sum is not > 0).  h_out4 = {(BR0 + BR1) / 2, BR0, BR1, value for team 0}; d_br[2][SCOPA_TEAM_N_CHOICE][4] (or NULL): d_br[p] is a
 *                   complete table, team p's rows one-hot at the chosen action, the other team's rows the policy's (scopa_best_response's form)
 *   minimax       : backward induction, both teams maximise: *h_value = the game value for team 0, d_policy_out (or NULL) a one-hot table of both teams
 *   policy_value  : *h_out = the exact expected reward of team 0 playing table a against team 1 playing table b; NULL = uniform
 * SCOPA_ESTATE before scopa_team_set_deal.  Everything launches on the context's stream; only the calls that return host values synchronise it. */
#define SCOPA_TEAM_N_CHOICE 321365
#define SCOPA_TEAM_N_LEAVES 331776
#define SCOPA_TEAM_N_INFOSETS 1648469
int32_t scopa_team_set_deal(scopa_ctx *ctx, const uint8_t perm16[16]);
int32_t scopa_team_tree_counts(scopa_ctx *ctx, int32_t *n_choice, int32_t *n_leaves, int32_t *n_infosets);
int32_t scopa_team_tree_leaves(scopa_ctx *ctx, int8_t *h_r2);
int32_t scopa_team_tables_reset(scopa_ctx *ctx);
int32_t scopa_team_tables_get(scopa_ctx *ctx, double *h_regret, double *h_strategy, double *h_local, double *h_leaf_reach_sum);
int32_t scopa_team_tables_set(scopa_ctx *ctx, const double *h_regret, const double *h_strategy, const double *h_local, const double *h_leaf_reach_sum);
int32_t scopa_team_cfr_iterate(scopa_ctx *ctx, int32_t n_iters, const double *h_w /*[n_iters][3] or NULL*/, double *h_root_values /*[n_iters][2] or NULL*/);
int32_t scopa_team_cfr_traverse(scopa_ctx *ctx, int32_t traverser, double *h_value);   /* one unweighted traversal: _cfr_recursive(root, traverser, 1.0, 1.0) -> value */
/* one launch of an unweighted traversal, for timing: part 0 = the 256 subtrees, 1 = depths 3..0; (0, 1) in order is scopa_team_cfr_traverse without the host value */
int32_t scopa_team_cfr_launch(scopa_ctx *ctx, int32_t traverser, int32_t part);
int32_t scopa_team_exploitability(scopa_ctx *ctx, const double *d_policy /*or NULL = average policy*/, double *h_out4, double *d_br /*[2][N_CHOICE][4] or NULL*/);
int32_t scopa_team_minimax(scopa_ctx *ctx, double *h_value, double *d_policy_out /*[N_CHOICE][4] or NULL*/);
int32_t scopa_team_policy_value(scopa_ctx *ctx, const double *d_policy_a, const double *d_policy_b, double *h_out);

/* ---- Team MiniScopa TPI over a SET of deals with the deal as a chance move: shared infosets, weighted CFR, best response across deals --------
 * On one deal (above) every node is its own infoset and the game is one of perfect information.  Here chance picks one of n deals uniformly and a
 * team's rows are shared between all deals the acting seat cannot tell apart: one regret, strategy and sigma row per distinct key.  The handle
 * borrows the context (its device and stream) and nothing else: the context's own team deal is neither read nor touched.
 *   key           : 64 bits of a choice node (depths 0..11): bits 60-63 the depth; bits 44-59 the acting seat's INITIAL hand as scopa_team_state.hand
 *                   holds it (nibble i = hand position i); bits 0-43 the card ids played so far, nibble i = ply i.  The table is empty at the deal, so
 *                   the table and everyone's remaining cards follow from that history: the partition of the reference's information_state_string
 *                   (openspiel_team_mini_scopa.py:138-168: acting seat, own hand, table, action history) with ONE refinement, the one MiniScopa's
 *                   ordered key makes: the hand is kept in hand order, not sorted.  Two occurrences of a key therefore have the same legal slots in
 *                   the same order, and a row's slot c means the same card everywhere.  A deal set whose seats' hands are stored ascending makes
 *                   equal hand sets share rows.  The depth d fixes the team, (d & 3) >> 1, and the legal count, 4 - (d >> 2).  Forced plies (depths
 *                   12..15) have one action and get no row; the chance game keeps no leaf_reach_sum
 *   create        : n >= 1 deals, h_perms[n][16], each a perm16 as scopa_team_set_deal takes it (else SCOPA_EINVAL).  Keys are computed on the device,
 *                   one lane per (deal, row) walking the row's path digits from the deal's root, and sorted on the host: global id = rank among the
 *                   distinct keys ascending, so the ids of one depth are contiguous.  Also built: map[n][SCOPA_TEAM_N_CHOICE] local row -> global id,
 *                   the occurrences deal * SCOPA_TEAM_N_CHOICE + row of every global id in ascending order, the depth-12 payoffs r2[n][SCOPA_TEAM_N_LEAVES].
 *                   Limits: n * SCOPA_TEAM_N_CHOICE < 2^31, and the increment image, n * SCOPA_TEAM_N_CHOICE * 64 bytes, within its byte budget (32 GiB:
 *                   1 670 deals) -- else SCOPA_ELIMIT before anything is allocated.  Destroy the handle before its context
 *   debug_image_budget : test hook on the CONTEXT: that budget in bytes for later creates (0 restores 32 GiB)
 *   counts        : deals, global rows G, (deal, row) occurrences = n * SCOPA_TEAM_N_CHOICE; any pointer may be NULL
 *   index_get     : h_keys[G] ascending; h_map[n][SCOPA_TEAM_N_CHOICE] (either may be NULL)
 *   tables        : [G][4] float64 regret and strategy sums, rows padded with 0 (a NULL pointer leaves that table alone), zero after create and reset.
 *                   The common factor 1/n is NOT applied to them (it cancels in regret matching and in the average policy), only to reported values.
 *                   The sigma rows are refreshed from the regrets on reset and on a tables_set that brings regrets; sigma_get copies them out:
 *                   regret matching of the regret rows over the legal slots, uniform where the positive parts do not sum to > 0
 *   cfr_iterate   : n_iters iterations of "for p in (0, 1)" as scopa_team_cfr_iterate, its weight contract and checks (h_w[n_iters][3] = (pos, neg,
 *                   strat), each finite and in [0, 1], NULL = all ones; n_iters <= 1 << 20; else SCOPA_EINVAL with nothing launched; 0 is a no-op).
 *                   Three launches per traversal, no host synchronisation between iterations.  (1) grid 256 x n: scopa_team_cfr_iterate's cut, one
 *                   workgroup per (deal, depth-4 subtree) gathers the subtree's 1 255 sigma rows into LDS (80 648 bytes) through the deal's map row,
 *                   rebuilds the reaches from the four ancestor rows and sweeps values up, v = ls[0] * u[0]; v += ls[c] * u[c] left to right; it updates
 *                   nothing: a traverser's node writes the 64-byte row {opp * (u[c] - v), reach * ls[c]} into the deal's slot of the increment image
 *                   [n][SCOPA_TEAM_N_CHOICE][8].  (2) grid n: depths 3..0 of each deal from its 256 subtree values, the same increments, the deal's root
 *                   value.  (3) one lane per global row of the traverser's team adds the row's cells over its occurrences in ascending (deal, row)
 *                   order STARTING FROM THE FIRST occurrence's value, then R <- R + dR; R <- !(R <= 0) ? R * pos : R * neg; S <- (S + dS) * strat and
 *                   the row's sigma by regret matching.  h_root_values[n_iters][2] (or NULL): (v_deal0 + v_deal1 + ...) / n in deal order per traversal.
 *                   No float64 atomics, one writer per row: bit-identical from run to run; one deal gives scopa_team_cfr_iterate's regret and strategy
 *                   tables and root values bit for bit; two copies of one deal give exactly twice its tables
 *   cfr_launch    : one launch of an unweighted traversal, for timing: part 0 = the subtrees, 1 = the tops, 2 = the reduce; (0, 1, 2) in order is one
 *                   traversal of cfr_iterate with weights (1, 1, 1)
 *   cfr_iterate_sampled : deal-sampled iterations.  Iteration t works on the m distinct deals h_deals[t][0..m) only; h_deals NULL (m ignored) = all n
 *                   deals.  Checked before the first launch, SCOPA_EINVAL with nothing changed otherwise: 0 <= n_iters <= 1 << 20 (0 is a no-op),
 *                   alternating 0 or 1, cfr_iterate's weight contract (finite, in [0, 1], NULL = all ones) and, with a list, 1 <= m <= n, every id in
 *                   [0, n), no id twice within an iteration.  The lists are uploaded once per call into a buffer of n_iters * m ids (never n_iters * n)
 *                   and the weights are launch arguments: no host synchronisation between iterations.  Per iteration a one-workgroup launch marks the
 *                   listed deals in a table [n]; each listed deal then gets cfr_iterate's launches (1) and (2) against the current sigma rows, grids
 *                   256 x m and m with the deal taken from the list, its increment rows going to its own slot of the image (create, its limits and its
 *                   byte budget are unchanged; unlisted slots are not read).  The reduce is (3) over the LISTED occurrences only: one lane per global
 *                   row of the updated team(s) asks the table for each occurrence's deal (occurrence / SCOPA_TEAM_N_CHOICE), loads the image rows of
 *                   listed occurrences alone and adds them in ascending (deal, row) order starting from the first listed one's value, so the order of
 *                   ids within a list changes no bit; a row with no listed occurrence takes +0.0 for both sums (a regret of -0.0 becomes +0.0).  EVERY
 *                   row of an updated team then gets cfr_iterate's update, so the weights discount every row every iteration.  The reduce's image
 *                   traffic falls with m; its launch still has a lane per global row and walks every occurrence id, as the MCCFR apply launch's cost
 *                   follows G.  alternating = 1: traverser 0's sweep and reduce, then traverser 1's sweep against the refreshed sigma and its reduce,
 *                   both on the iteration's list; with h_deals NULL, or a list naming all n deals in any order, tables, sigma and root values are
 *                   cfr_iterate's bit for bit.  alternating = 0: both traversers' sweeps run against the sigma rows of the iteration's start (their
 *                   image rows are disjoint) and one reduce launch updates the rows of both teams: the bits of two independent sweeps followed by the
 *                   two reduces.  h_root_values[n_iters][2] (or NULL): per traverser's sweep the listed deals' root values added in ascending deal id
 *                   from the first, divided by m.  Increments are NOT scaled by n / m -- a common factor, like the 1/n left out of the tables -- so a
 *                   run that mixes different m weights its iterations by m.  The sigma rows are left as cfr_iterate's reduce leaves them: cfr_iterate,
 *                   mccfr_iterate and exploitability may follow on the same handle in any order.  No float64 atomics, one writer per row:
 *                   bit-identical from run to run.  Synchronises only to return root values
 *   exploitability: the best response ACROSS deals.  The per-node maximum of the one-deal solver is no best response here, because a responder's row
 *                   is shared by nodes in several deals.  Per responder p, level by level from depth 11 to 0: on a level p plays, a lane per (deal,
 *                   node) writes q[c] = opp_reach(node) * val(child c) into the image -- opp_reach the running product from the root of the policy's
 *                   probabilities of the OTHER team along the path -- a lane per global row of that depth adds q over the row's occurrences in the
 *                   fixed order from the first and takes the first slot that is best by a strict `>` (ties to the lowest slot, an all-zero row slot 0),
 *                   and the level's values are val(child[choice]); on the other team's levels v = 0.0; v += row[c] * val(child c), left to right, rows
 *                   used as given; terminals 0.5 * r2, negated for team 1.  h_out4 = {(BR0 + BR1) / 2, BR0, BR1, value of the policy for team 0}, each
 *                   entry (v_deal0 + v_deal1 + ...) / n in deal order; per deal the value is bit for bit scopa_team_policy_value of the policy_for_deal
 *                   table.  d_policy[G][4] DEVICE table or NULL = the average of the strategy table, uniform where its sum is not > 0; d_policy_out[G][4]
 *                   (or NULL) receives the evaluated policy; d_br[2][G][4] (or NULL): d_br[p] is a complete table, team p's rows one-hot at the choice,
 *                   the other team's rows the policy's.  Tables 32-byte aligned (else SCOPA_EINVAL).  Scratch, allocated at first use: 2 x
 *                   [n][SCOPA_TEAM_N_CHOICE + SCOPA_TEAM_N_LEAVES] float64 for reach and values.  A sequence of launches, one lane per node, no host round
 *                   trip between levels; synchronises at the end
 *   policy_for_deal: scatters a DEVICE table d_policy_G[G][4] into one deal's local row order, d_policy_local[SCOPA_TEAM_N_CHOICE][4] (device): what
 *                   scopa_team_policy_value and scopa_team_exploitability take on a context holding that deal.  Does not synchronise */
typedef struct scopa_team_chance scopa_team_chance;
int32_t scopa_team_chance_create(scopa_ctx *ctx, int32_t n, const uint8_t *h_perms /*[n][16]*/, scopa_team_chance **out);
int32_t scopa_team_chance_destroy(scopa_team_chance *g);
int32_t scopa_team_chance_debug_image_budget(scopa_ctx *ctx, int64_t bytes);
int32_t scopa_team_chance_counts(scopa_team_chance *g, int32_t *n_deals, int64_t *n_global, int64_t *n_occurrences);
int32_t scopa_team_chance_index_get(scopa_team_chance *g, uint64_t *h_keys /*[G]*/, int32_t *h_map /*[n][SCOPA_TEAM_N_CHOICE]*/);
int32_t scopa_team_chance_tables_reset(scopa_team_chance *g);
int32_t scopa_team_chance_tables_get(scopa_team_chance *g, double *h_regret, double *h_strategy);
int32_t scopa_team_chance_tables_set(scopa_team_chance *g, const double *h_regret, const double *h_strategy);
int32_t scopa_team_chance_sigma_get(scopa_team_chance *g, double *h_sigma /*[G][4]*/);
int32_t scopa_team_chance_cfr_iterate(scopa_team_chance *g, int32_t n_iters, const double *h_w /*[n_iters][3] or NULL*/, double *h_root_values /*[n_iters][2] or NULL*/);
int32_t scopa_team_chance_cfr_iterate_sampled(scopa_team_chance *g, int32_t n_iters, int32_t m,
                                              const int32_t *h_deals /*[n_iters][m]; NULL (m ignored) = all n deals*/, const double *h_w /*[n_iters][3] or NULL*/,
                                              int32_t alternating, double *h_root_values /*[n_iters][2] or NULL*/);
int32_t scopa_team_chance_cfr_launch(scopa_team_chance *g, int32_t traverser, int32_t part);
int32_t scopa_team_chance_exploitability(scopa_team_chance *g, const double *d_policy /*[G][4] or NULL*/, double *h_out4, double *d_policy_out /*[G][4] or NULL*/,
                                         double *d_br /*[2][G][4] or NULL*/);
int32_t scopa_team_chance_policy_for_deal(scopa_team_chance *g, const double *d_policy_G, int32_t deal, double *d_policy_local /*[SCOPA_TEAM_N_CHOICE][4]*/);

/* ---- Team MiniScopa TPI, external-sampling MCCFR: MCCFRTrainer(TPIMiniScopaGame()) : src/algorithms/mc_cfr.py:27-99 run on
 * src/envs/openspiel_team_mini_scopa.py, over the regret_sum, strategy_sum and local_strategy tables above (tables_get / tables_set serve both solvers).
 * _sample draws one np.random.choice at EVERY decision visit, the forced ones included (mc_cfr.py:55), recurses into the sampled child (:67) and, at a
 * traverser's node with b cards, into every child in order (:72-78).  The recursion's shape does not depend on the draws: 49 381 visits (draws) per
 * traversal of team 0, 20 583 of team 1, 69 964 per iteration(); 14 400 terminals per traversal; down to depth 11 there are 9 781 (2 583) visit
 * instances, 1 731 of them the traverser's, and 3 600 arrivals at depth-12 nodes.  reach_probs[traverser] is never updated (:61-65): every traverser visit
 * adds sigma to strategy_sum (:84).  A forced node of the traverser's keeps regret_sum [0.] and its strategy_sum is its visit count: per arrival at its
 * depth-12 ancestor the team's first forced ply is visited once and its second twice.
 *   state         : seen[SCOPA_TEAM_N_CHOICE] uint8, 1 where a decision visit reached the row (the reference's dict holds its key, mc_cfr.py:32-35);
 *                   leaf_visits[2][SCOPA_TEAM_N_LEAVES] uint64, arrivals at each depth-12 node per traverser (all four forced nodes below it then exist;
 *                   strategy_sum of team p's first / second forced node = 1 x / 2 x leaf_visits[p]); the delta buffer [SCOPA_TEAM_N_CHOICE][5] float64,
 *                   4 regret increments + traverser-visit count (scopa_mccfr_delta_buffer's layout); an iteration counter.  Allocated at the first
 *                   call below; scopa_team_set_deal and scopa_team_tables_reset return all of it, and the counters, to zero
 *   replay        : MCCFRTrainer.iteration() (:88-92) n_iters times in the reference's visit order on live tables, driven by h_uniforms -- what
 *                   np.random.choice draws, one float64 per decision visit; a forced tail's 11 (5) draws are skipped in the stream.  Tables, seen and
 *                   leaf_visits come out bit-identical to the reference under the same np.random.seed (np.dot, :79, is the fma chain v = fma(sigma[i],
 *                   cfv[i], v) from 0.0); local_strategy of every updated row is refreshed as in scopa_team_cfr_iterate.  *consumed = n_iters x 69 964.
 *                   n_uniforms < n_iters x 69 964 is SCOPA_EINVAL with nothing changed; n_iters <= 1 << 20.  The form shipped walks on ONE lane
 *   traverse      : the throughput path, scopa_mccfr_traverse's contract: traversals with global ids [b0, b0 + nb) of `iteration`, one per traverser each,
 *                   against the regrets as they are (frozen: walks read the regret table and write only the delta buffer, seen and leaf_visits).  The
 *                   draw of a visit is u53(x0, x1) of Philox4x32-10 under scopa_mccfr_seed's key with counter
 *                       (index of the visit instance in the traversal's fixed-shape recursion, global traversal id, iteration, 64 + traverser)
 *                   the index being level-major over the instance tree: instance j of depth d has index (instances above depth d) + j, its child
 *                   instances are j * m + slot with m = b + 1 at the traverser's plies (slot 0 the sampled child, slot 1 + c child c) and m = 1
 *                   elsewhere.  Forced plies draw nothing.  The action follows np.random.choice's rule as in the replay; value = reward of the leaf
 *                   the sampled descent ends in; increment = weight * (cfv_all - v), weight = opponent reach / traverser's sampling probability, 0
 *                   where that probability is 0 (:79-83).  Results do not depend on how [b0, b0 + nb) is split over calls, up to the order of the
 *                   float64 additions into a row.  nb <= 1 << 24
 *   apply         : one launch over all rows; a row with count > 0: regret += delta[:4]; strategy += count * sigma, sigma = regret matching
 *                   (InfoNode.current_strategy, :20-24) of the regrets BEFORE the add; local_strategy = get_strategy() (vanilla_cfr.py:23-30) of the new
 *                   regrets, so scopa_team_cfr_iterate may follow; delta <- 0.  The iteration counter += 1
 *   iterate       : n_iters x { traverse(counter, 0, batch); apply }
 *   counters      : decision visits (forced ones included, on either path: 69 964 per pair of traversals), terminal visits (28 800 per pair) and the
 *                   iteration counter (applies).  Exact integers that follow from the shape; the replay adds to the first two
 *   delta_get     : host copy of the delta buffer, h_delta[SCOPA_TEAM_N_CHOICE][5];  visits_get: h_seen[SCOPA_TEAM_N_CHOICE], h_leaf_visits[2][SCOPA_TEAM_N_LEAVES],
 *                   either may be NULL */
int32_t scopa_team_mccfr_replay(scopa_ctx *ctx, int32_t n_iters, const double *h_uniforms, int64_t n_uniforms, int64_t *consumed);
int32_t scopa_team_mccfr_traverse(scopa_ctx *ctx, uint32_t iteration, uint32_t b0, uint32_t nb);
int32_t scopa_team_mccfr_apply(scopa_ctx *ctx);
int32_t scopa_team_mccfr_iterate(scopa_ctx *ctx, uint32_t batch, uint32_t n_iters);
int32_t scopa_team_mccfr_counters(scopa_ctx *ctx, uint64_t *decision_visits, uint64_t *terminal_visits, uint32_t *iterations);
int32_t scopa_team_mccfr_delta_get(scopa_ctx *ctx, double *h_delta);
int32_t scopa_team_mccfr_visits_get(scopa_ctx *ctx, uint8_t *h_seen, uint64_t *h_leaf_visits);

/* ---- Team MiniScopa over a set of deals, external-sampling MCCFR with the deal sampled too: the sampling solver above on the rows the deals share by
 * key (scopa_team_chance_* tables; tables_get / tables_set / sigma_get / exploitability serve both solvers).  Within one deal the map from local row to
 * global row is injective, so a traversal on one deal is scopa_team_mccfr_traverse's walk with every table address sent through the deal's map row.
 *   state         : the delta buffer [G][5] float64, 4 regret increments + traverser-visit count over the global ids (scopa_team_mccfr_delta_get's layout),
 *                   allocated at the first call below (SCOPA_ENOMEM leaves nothing allocated), zeroed by tables_reset, freed by destroy; two visit
 *                   counters and an iteration counter that counts applies from 0 at create -- tables_reset and tables_set leave the counters alone, as on
 *                   scopa_chance.  No seen marks and no leaf_visits: the chance game keeps no leaf_reach_sum either.  create is unchanged
 *   traverse      : traversals with global ids [b0, b0 + nb) of `iteration`, one per traverser each, on deal `deal` against the shared regrets as they
 *                   are; sigma = regret matching (InfoNode.current_strategy) of the shared regret row of the node's key; the draws are exactly those of
 *                   scopa_team_mccfr_traverse(iteration, b0, nb) on a context holding that deal: Philox counter (instance index, traversal id, iteration,
 *                   64 + traverser) under scopa_mccfr_seed's key of the handle's context.  Writes only the delta buffer.  nb <= 1 << 24, b0 + nb must not
 *                   overflow, deal in [0, n): else SCOPA_EINVAL with nothing changed; nb = 0 is a no-op
 *   apply         : one launch, a lane per global row; a row with count > 0: regret += delta[:4]; strategy[c] += count * sigma[c] for the legal slots,
 *                   sigma of the regrets BEFORE the add; the row's sigma refreshed as cfr_iterate's reduce leaves it, so cfr_iterate may follow on the
 *                   same handle; delta <- 0.  A row with count 0 is not written.  No discount.  The iteration counter += 1
 *   walk          : the walk launch of ONE iteration alone, for timing: iterate is { walk(counter, batch, m, list); apply } per iteration
 *   iterate       : iteration t of the call works on the m distinct deals h_deals[t][0..m), or on all n when h_deals is NULL (m is then ignored): ONE walk
 *                   launch, then apply.  The launch covers, for every listed deal d, the traversals d * batch + i, i < batch, of the handle's iteration
 *                   counter: ids follow the deal id and not its list position, so neither list order nor m changes the random words a deal sees, and two
 *                   copies of one deal draw independent traversals.  Increments are NOT scaled by n / m.  The lists are uploaded once per call; no host
 *                   synchronisation between iterations.  A workgroup serves one deal for the whole launch (its LDS accumulator of the rows of depths
 *                   0..4 is flushed once through the deal's map row); deeper rows are float64 atomics into shared rows, so the arrival order spans deals:
 *                   counts and strategy sums are exact, regrets reproducible to rounding.  SCOPA_EINVAL, checked before any launch and with nothing
 *                   changed: batch = 0 or > 1 << 24; n_iters < 0 or > 1 << 20; n * batch > 2^32; with a list m < 1, m > n, an id outside [0, n) or an id
 *                   twice within one iteration.  n_iters = 0 is a no-op
 *   counters      : decision visits (69 964 per pair of traversals, forced plies included), terminal visits (28 800 per pair), the iteration counter
 *   delta_get     : host copy of the delta buffer, h_delta[G][5] */
int32_t scopa_team_chance_mccfr_traverse(scopa_team_chance *g, uint32_t iteration, int32_t deal, uint32_t b0, uint32_t nb);
int32_t scopa_team_chance_mccfr_apply(scopa_team_chance *g);
int32_t scopa_team_chance_mccfr_walk(scopa_team_chance *g, uint32_t iteration, uint32_t batch, int32_t m, const int32_t *h_deals /*[m] or NULL = all n deals*/);
int32_t scopa_team_chance_mccfr_iterate(scopa_team_chance *g, int32_t n_iters, uint32_t batch, int32_t m, const int32_t *h_deals /*[n_iters][m]; NULL (m ignored) = all n deals*/);
int32_t scopa_team_chance_mccfr_counters(scopa_team_chance *g, uint64_t *decision_visits, uint64_t *terminal_visits, uint32_t *iterations);
int32_t scopa_team_chance_mccfr_delta_get(scopa_team_chance *g, double *h_delta /*[G][5]*/);

/* ---- Team MiniScopa, policy against policy on one deal (build-defined; the two-player counterparts are scopa_cross_play and
 * scopa_eval_pair_match): the exact cross-play matrix of K tables and the sampled seat-swapped match.  Tables are [SCOPA_TEAM_N_CHOICE][4] float64
 * DEVICE tables, 32-byte aligned, used as given: rows are not normalised, the padding slots c >= b are never read into a sum, a non-finite entry
 * propagates by IEEE rules.  Policy a plays team 0's depths and policy b team 1's (the teams of scopa_team_set_deal's tree: (d & 3) >> 1).
 *   leaf scopas   : a uint8 per depth-12 node, after its four forced plies: scopas of team 0's two seats summed in the low nibble, of team 1's in the
 *                   high nibble.  Built at the first call below, not by scopa_team_set_deal, which only invalidates them; freed by scopa_ctx_destroy
 *   cross_play    : d_out[a][b] = { E[reward of team 0], E[its square], E[scopas of team 0], E[scopas of team 1] } with table a as team 0 against table
 *                   b as team 1.  At a depth-12 node the four quantities are 0.5 * r2, 0.25 * r2 * r2 and the two nibbles; per node and quantity
 *                   v = 0.0; v += row[c] * child[c], children left to right (scopa_team_policy_value's arithmetic: d_out[a][b][0] is its value bit for
 *                   bit).  Two launches in scopa_team_cfr_iterate's cut.  (1) grid (n_pol * n_pol, 256), one workgroup per (a, b, depth-4 subtree): one
 *                   upward pass, every row loaded once as a 32-byte vector straight from its team's table; only the values live in LDS (1 255 x 4
 *                   float64, 40 160 bytes static: four workgroups per compute unit).  (2) grid n_pol * n_pol: depths 3..0 from the 256 x 4 subtree
 *                   values.  No float64 atomics, every sum in a fixed order: bit-identical from run to run.  Does not synchronise, except that a call
 *                   which has to grow the scratch waits for the stream first (an earlier call's launches may still read the old one).  The subtree
 *                   image [n_pol * n_pol][256][4] belongs to the context and grows on demand; the leaf scopas are built before it, so SCOPA_ENOMEM
 *                   leaves no scratch image allocated (leaf scopas already built stay: they are the deal's, like its payoffs).  The grid is
 *                   three-dimensional (pairs, subtrees, deals) because no dimension may reach 2^32 lanes: n_pol = 256, 2^24 workgroups, launches.
 *                   n_pol outside [1, 256], a NULL pointer or a misaligned table: SCOPA_EINVAL; 256 * n_pol * n_pol workgroups at or above the
 *                   limit (2^31: not reachable on one deal): SCOPA_ELIMIT before anything is allocated or launched
 *   match         : episode i draws ply d = 0..11 at Philox counter (i, i >> 32, 32 + d, stream_id) under scopa_mccfr_seed's key (tags 32..44 stay
 *                   clear of scopa_eval_pair_match's 0..8 under one stream id); N = the 53-bit integer of u53(x0, x1); the action is
 *                   #{k < b - 1 : thr[k] <= N} with thr the thresholds of scopa_eval_pair_match's formula computed on the fly from the acting team's
 *                   table row and b = 4 - (d >> 2), so a row that sums to 0 or NaN plays slot 0; the child is j * b + action.  Episodes i < n_team0 have
 *                   a as team 0 and b as team 1, the rest the other way round.  d_leaf_out[n] (int32, or NULL): the depth-12 index every episode ends
 *                   at.  h_stats[half][5] = episodes, sum of a's rewards x2, sum of their squares, a's team's scopas, b's team's scopas, from a's
 *                   side: exact integers summed on the device.  One lane per episode.  Synchronous; n = 0 gives zeros and launches nothing; n < 0,
 *                   n_team0 outside [0, n], a NULL table or h_stats, a misaligned table: SCOPA_EINVAL
 *   debug_xplay_group_limit : test hook on the CONTEXT: the workgroup limit of cross_play and of scopa_team_chance_cross_play (0 restores 2^31)
 * SCOPA_ESTATE before scopa_team_set_deal. */
int32_t scopa_team_cross_play(scopa_ctx *ctx, int32_t n_pol, const double *d_policies /*[n_pol][SCOPA_TEAM_N_CHOICE][4]*/, double *d_out /*[n_pol][n_pol][4]*/);
int32_t scopa_team_match(scopa_ctx *ctx, const double *d_policy_a, const double *d_policy_b, int64_t n, int64_t n_team0, uint32_t stream_id,
                         int32_t *d_leaf_out /*[n] or NULL*/, int64_t h_stats[10]);
int32_t scopa_team_debug_xplay_group_limit(scopa_ctx *ctx, int64_t groups);

/* ---- Team MiniScopa over a set of deals, policy against policy (build-defined; the two-player counterparts are scopa_chance_cross_play and
 * scopa_chance_match).  Tables are [G][4] float64 DEVICE tables over the handle's global rows, 32-byte aligned, used as given.  The kernels are the
 * one-deal ones above with every row address sent through the deal's map row.
 *   leaf scopas   : [n][SCOPA_TEAM_N_LEAVES] uint8 as above, built at the first call below (scopa_team_chance_create is unchanged), freed by destroy
 *   cross_play    : (1) grid (n_pol * n_pol, 256, n), one workgroup per (a, b, depth-4 subtree, deal), the pair index fastest; the same 40 160 bytes
 *                   of LDS.  (2) grid (n_pol * n_pol, n): the per-deal image [n][n_pol][n_pol][4], into d_per_deal or, where that is NULL, into scratch.
 *                   (3) one lane per (a, b, quantity): s = img[0]; s += img[1]; ... in deal order, then s / (double)n -> d_out.  d_per_deal[d] is bit
 *                   for bit what scopa_team_cross_play writes on a context holding deal d for the policy_for_deal tables; d_out[a][a][0] is the value
 *                   entry of scopa_team_chance_exploitability for policy a, and d_out[br0][a][0] its BR0 entry where br0 is d_br[0] of that call; one
 *                   deal gives scopa_team_cross_play's bits.  The subtree image [n][n_pol * n_pol][256][4] and the scratch per-deal image belong to the
 *                   handle and grow on demand, after the leaf scopas (SCOPA_ENOMEM leaves neither image allocated).  Does not synchronise, except
 *                   in the handle's first call, which waits for the leaf scopas, and in a call that has to grow the scratch.  Errors as above;
 *                   SCOPA_ELIMIT where 256 * n * n_pol * n_pol reaches 2^31 (128 deals at n_pol = 256), before anything is allocated or launched
 *   match         : scopa_team_match with the deal drawn per episode, as scopa_chance_match draws it: deal = (x0 * n_deals) >> 32 from the first Philox
 *                   word of counter (i, i >> 32, 44, stream_id).  An episode that drew deal d ends at the index scopa_team_match(ctx_d,
 *                   policy_for_deal(a, d), policy_for_deal(b, d), ...) writes at d_leaf_out[i] on a context holding d under the same seed.  d_deal_out[n],
 *                   d_leaf_out[n] (int32, or NULL).  h_stats as above.  Synchronous; the same refusals */
int32_t scopa_team_chance_cross_play(scopa_team_chance *g, int32_t n_pol, const double *d_policies /*[n_pol][G][4]*/, double *d_per_deal /*[n][n_pol][n_pol][4] or NULL*/,
                                     double *d_out /*[n_pol][n_pol][4]*/);
int32_t scopa_team_chance_match(scopa_team_chance *g, const double *d_policy_a, const double *d_policy_b, int64_t n, int64_t n_team0, uint32_t stream_id,
                                int32_t *d_deal_out /*[n] or NULL*/, int32_t *d_leaf_out /*[n] or NULL*/, int64_t h_stats[10]);

/* ---- Deep CFR on Team MiniScopa over a set of deals (scopa_team_chance_sdcfr.hip; the two-player counterpart is the scopa_chance_sdcfr_* block).
 * DeepCFR._external_sampling_cfr (deep_cfr.py:284-365) on TPIMiniScopaGame: the "player" is the team of the seat to move, and the reference's feature
 * encoder reads the mover's hand and the table only, so MiniScopa's 34 features, its 34-128-64-16 advantage net and scopa_sdcfr_pack_weights apply
 * unchanged with player = team.  A handle over one deal is the one-deal solver.  All calls launch on the handle's context's stream.
 *   sdcfr_traverse : `batch` traversals of `traverser` (a team) in each of the m listed deals (h_deals[0..m), distinct ids in [0, n); NULL with m = 0:
 *                   all n, slot = deal), in two launches without a host synchronisation.  Node-info images are built on the device once per handle, at
 *                   the first call: [n][321365] feature bits | hand nibbles of the choice rows, [n][4][331776] feature bits of the forced nodes.
 *                   Launch 1 (the matrix cores; grid cut by slot, team and chunk, a workgroup loads one team's weight slices into registers once and
 *                   loops over that team's 16-node tiles) writes, for every listed deal, every choice row's regret-matching policy [4] (float32, hand
 *                   order, zeros beyond the legal count) under the net of the row's team and its sampling thresholds [3] (uint64; scopa_sdcfr's
 *                   definition: thr[k] = ceil(cdf_k / cdf_last * 2^53), 2^53 beyond the legal count, thr[0] = ~0 where the sum is 0) -- and the
 *                   policy of the traverser's forced nodes (depths 12, 13 for team 0, 14, 15 for team 1), which the reference evaluates like any
 *                   other: relu(adv) / max(relu(adv), 1e-8) of the one legal card, 1 or 0 but for advantages below 1e-8.  Every accumulator keeps
 *                   scopa_sdcfr's K order: equal features give the MiniScopa kernels' bits.  Launch 2 walks the traversals, a workgroup per traversal
 *                   and one slot per workgroup for the whole launch: the traverser's plies branch into every legal card in hand order, the other
 *                   team's plies compare N (u = N * 2^-53, N from x0, x1 of the draw) with the node's thresholds as integers -- a zero sum keeps numpy's
 *                   (int)(u * legal) --, the terminal is worth 0.5 * r2 of the traverser's team, values come back up in float32 in hand order
 *                   (scopa_sdcfr_backward's arithmetic: value = sum policy * child, regrets = cfv - value over all 16 slots, / (max|.| + 1e-8)) and
 *                   every node of the traverser, forced ones included, leaves a row: SCOPA_TEAM_SDCFR_ROWS = 1 653 rows per traversal (501 choice
 *                   + 2 x 576 forced; not MiniScopa's 1 653 decision nodes), in depth-first post-order.  Traversal i of deal d in slot s has global
 *                   id b0 + d * batch + i; a draw is Philox4x32-10 under scopa_mccfr_seed's key at counter (local row of the node, traversal id,
 *                   iteration, 96 + traverser) -- tags 0, 1 (MCCFR), 4, 5 (MiniScopa Deep CFR), 8 and 32..44 (matches, playouts), 48 (team playouts),
 *                   64, 65 (team MCCFR) are taken -- so list order, m, batch chunking and launch geometry change no draw.  Rows go to ring rows
 *                   (write_base + 1653 * (s * batch + i) + rank) % capacity, the root value to d_root_values[s * batch + i].  No atomics: runs are
 *                   bit-identical, and a deal's rows do not depend on the list.  d_mem_mask may be NULL (a row's mask is features[0..16)).
 *                   Refused with SCOPA_EINVAL and a message, before anything is launched or written: a NULL pointer; traverser outside {0, 1};
 *                   batch < 0, or 0 with a list; a list with m outside [1, n], an id outside [0, n) or an id twice; no list with m other than 0 or
 *                   n; d_image / d_mem_regret / d_mem_mask not 16-byte or d_mem_feat not 8-byte aligned; capacity < 1653 or >= 2^30; write_base
 *                   outside [0, capacity); 1653 * m * batch > capacity; b0 + n * batch > 2^32.  batch = 0 without a list: no-op.
 *   sdcfr_visits  : non-terminal visits of the handle's traversal calls, SCOPA_TEAM_SDCFR_VISITS0 / 1 per traversal, counted on the host
 *   sdcfr_policy_get : for tests: the policies [321365][4] and thresholds [321365][3] of slot `slot` of the last traversal call (either may be NULL).
 *                   Synchronises.  SCOPA_ESTATE before the first traversal call, SCOPA_EINVAL for a slot outside the last call's m
 *   sdcfr_forced_get : for tests, beside it: the policy of the one legal card at the last call's traverser's forced nodes, [2][331776] float32 by
 *                   depth-12 node: [0] its first forced depth (12 or 14), [1] the second.  Same refusals
 *   sdcfr_average_policy : scopa_chance_sdcfr_average_policy's definition over the handle's keys of `team`: per distinct key the FIFO float32 sum of
 *                   positive_regret_policy(net_s(x)) * d_coef[s], the float64 normalisation over the legal slots, uniform where the sum is 0 or not
 *                   finite, zeros beyond the legal count, a slot outside the store giving NaN and hence uniform; the other team's rows are left
 *                   untouched.  x comes from the key's representative node, its first occurrence in ascending (deal, row) order.  The terms pass
 *                   and the reduce are scopa_chance_sdcfr_average_policy's kernels, run over chunks of keys (multiples of sixteen) whose terms
 *                   [n_snap][chunk] float4 stay within 1 GiB.  No atomics.
 *   debug_sdcfr   : test hooks on the CONTEXT: the bytes those terms may take, and the workgroups a slot of the walk launch may have, so that small cases
 *                   reach the chunked pass and a workgroup that walks several traversals (0 restores a default); launches: 1 = a traversal call makes
 *                   its policy launch alone, 2 = its walk launch alone over the tables of the call before (SCOPA_ESTATE without them), for
 *                   benchmarks that time the two apart; 0 = both
 * Everything is allocated at first use and freed by scopa_team_chance_destroy; the other calls on the handle are unaffected and may be interleaved. */
#define SCOPA_TEAM_SDCFR_ROWS 1653
#define SCOPA_TEAM_SDCFR_VISITS0 4277
#define SCOPA_TEAM_SDCFR_VISITS1 3127
int32_t scopa_team_chance_sdcfr_traverse(scopa_team_chance *g, int32_t traverser, int32_t batch, int32_t m, const int32_t *h_deals /*[m]; NULL (m = 0) = all n deals*/,
                                         const float *d_image, float *d_mem_feat, float *d_mem_regret, float *d_mem_mask /*may be NULL*/, int64_t capacity,
                                         int64_t write_base, float *d_root_values /*[m * batch]*/, uint32_t iteration, uint32_t b0);
int32_t scopa_team_chance_sdcfr_visits(scopa_team_chance *g, uint64_t *decision_visits);
int32_t scopa_team_chance_sdcfr_policy_get(scopa_team_chance *g, int32_t slot, float *h_policy /*[321365][4] or NULL*/, uint64_t *h_thr /*[321365][3] or NULL*/);
int32_t scopa_team_chance_sdcfr_forced_get(scopa_team_chance *g, int32_t slot, float *h_forced /*[2][331776]*/);
int32_t scopa_team_chance_sdcfr_average_policy(scopa_team_chance *g, int32_t team, int32_t n_snap, const float *d_w1, const float *d_b1, const float *d_w2,
                                               const float *d_b2, const float *d_w3, const float *d_b3, int32_t max_size, const int32_t *d_slots,
                                               const float *d_coef, double *d_policy_G /*[G][4]*/);
int32_t scopa_team_chance_debug_sdcfr(scopa_ctx *ctx, int64_t terms_bytes, int32_t walk_groups, int32_t launches);

/* ---- N > 1: one-shot all-reduce of the delta buffer over peer (xGMI) memory -------------------------------------------------
 * One process per GPU on one node.  create: allocates this rank's inbox (fine-grained device memory) and returns its 64-byte
 * hipIpc handle; the caller all-gathers the handles (torch.distributed) and passes all `world` of them to connect.
 * allreduce_delta (on the context's stream): the delta buffer of every rank becomes the sum over ranks, added in rank order on
 * every rank (bit-identical replicas).  Waits are bounded (5 s, scopa_p2p_set_budget): a wait that gives up is counted, makes
 * every later wait fall through (a dead peer cannot hang a GPU) and makes allreduce_delta / iterate_sharded -- which synchronise
 * the stream before they return -- fail with SCOPA_ETIMEOUT, on that call and on every later one until the exchange is
 * re-created; status returns the count (0 = healthy) and the exchanges issued.  Replaces torch.distributed.all_reduce(delta)
 * between scopa_mccfr_traverse and scopa_mccfr_apply.
 * set_form: 0 (default) = plain stores + system-scope release fence / acquire fence (the textbook protocol); 1 = every access to an
 * inbox line is a system-scope (sc0 sc1) access ordered by s_waitcnt alone: 4.5 us less per iteration, no cache maintenance; use
 * it only after it has been validated against a collective on the topology at hand (scopa_amd/distributed.py does that). */
int32_t scopa_p2p_create(scopa_ctx *ctx, int32_t rank, int32_t world, uint8_t handle_out[64]);
int32_t scopa_p2p_connect(scopa_ctx *ctx, const uint8_t *handles /*[world][64]*/);
int32_t scopa_p2p_allreduce_delta(scopa_ctx *ctx);
int32_t scopa_p2p_set_form(scopa_ctx *ctx, int32_t light);
int32_t scopa_p2p_set_budget(scopa_ctx *ctx, double seconds);   /* wait budget of later exchanges, 1 ms .. 60 s */
/* n_iters whole iterations of this rank's slice [b0, b0+nb) of the global traversal ids, the exchange fused into the
 * reduce+apply kernel (two launches per iteration, as on one GPU); all ranks call it with the same n_iters */
int32_t scopa_mccfr_iterate_sharded(scopa_ctx *ctx, uint32_t b0, uint32_t nb, uint32_t n_iters);
int32_t scopa_p2p_status(scopa_ctx *ctx, int32_t *timeouts, uint64_t *exchanges);
int32_t scopa_p2p_destroy(scopa_ctx *ctx);

/* ---- counters / profiling -------------------------------------------------------------------------------
 * exact integer counts of decision-node visits ("infoset-traversals") and terminal visits since creation */
int32_t scopa_counters(scopa_ctx *ctx, uint64_t *decision_visits, uint64_t *terminal_visits);
/* stride > 0: every stride-th launch of the dominant traversal kernel carries a (start, stop) HIP event pair attached to
 * the dispatch itself (hipExtLaunchKernelGGL) on the context's stream (stride 1 = every launch); 0 = off.  scopa_prof_read
 * synchronises and returns the number of sampled launches and their summed kernel milliseconds since enable. */
int32_t scopa_prof_enable(scopa_ctx *ctx, int32_t stride);
int32_t scopa_prof_read(scopa_ctx *ctx, int64_t *launches, double *kernel_ms);
/* the same kernel timed by ITSELF: per sampled launch (the ones scopa_prof_enable's stride selects), first workgroup start ->
 * last workgroup end on the 100 MHz device-wide clock, summed over the samples held (the last 2048 at most) since scopa_prof_enable;
 * no events, no dispatch latency: launch ramp and end-of-kernel write-back are outside it */
int32_t scopa_prof_device(scopa_ctx *ctx, int64_t *launches, double *kernel_ms);
/* after scopa_prof_device: mean microseconds a workgroup of the sampled launches spent in (prologue, traversal walks, epilogue) */
int32_t scopa_prof_phases(scopa_ctx *ctx, double out_us[3]);
/* beside the phases: { mean start of a workgroup behind the first workgroup of its launch, the LAST workgroup's start behind the first, the longest
 * workgroup of a launch } in microseconds, means over the sampled launches -- what a launch's time is made of beside its workgroups' own phases */
int32_t scopa_prof_spread(scopa_ctx *ctx, double out_us[3]);

#ifdef __cplusplus
}
#endif
#endif /* SCOPA_H */
