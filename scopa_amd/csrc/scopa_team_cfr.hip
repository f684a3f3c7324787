// scopa_team_cfr.hip -- Team MiniScopa TPI solved on the device for one fixed deal: the reference's vanilla CFR (CFRTrainer._cfr_recursive,
// src/algorithms/vanilla_cfr.py:56-99, run on TPIMiniScopaGame, src/envs/openspiel_team_mini_scopa.py) with per-iteration weights, and the exact
// value passes (best response, minimax, policy against policy).
//
// The tree is regular: ply k is played by seat k & 3 (team (k & 3) >> 1) from a hand of 4 - (k >> 2) cards, always for 16 plies.  Depths 0..11 hold
// the 321 365 nodes with a real choice, level-major, node id = level offset + mixed-radix path (first ply most significant), child = j * b + c;
// depths 12..15 are forced (one card left), so a depth-12 node stands for its whole forced tail and carries the terminal's payoff.  The infoset
// string ends in the full action history: for a fixed deal every node is its own infoset, every table row has exactly one node.  The reference's
// order-dependent recursion therefore equals a level-synchronous sweep: reaches down with the stored sigma, values up, the traverser's rows updated,
// every row's sigma refreshed (vanilla_cfr.py:97).  A forced node of team p keeps regret 0 and sigma 1 and its strategy_sum is the sum, over team
// p's traversals, of p's reach at its depth-12 ancestor: one number per (team, depth-12 node), leaf_reach_sum.
//
// The cut is by the first round of play.  Launch 1: one workgroup per depth-4 node (256) rebuilds its reaches from its four ancestor rows and sweeps
// its subtree (1 255 rows, 1 296 leaves) through LDS.  Launch 2: one workgroup finishes depths 3..0 from the 256 subtree values.  Stream order
// between the two also means the top rows' sigma is replaced only after every subtree workgroup has read it.  Every row has one writer and every
// float64 sum a fixed order: no atomics, runs are bit-identical.
#include <string.h>

#include <new>

#include "scopa_team_passes.h"

using scopa::fail;

namespace {

// One node of the sweep (vanilla_cfr.py:87-97) with B legal actions: value = np.sum(local_strategy * action_utils); on the traverser's rows
// regret_sum += opponent_reach * (action_utils - value), strategy_sum += reach * local_strategy, then the iteration's weights; the row's sigma is
// refreshed from its regrets whoever moves.  `row` is the node's table row; returns the value.
template <int B>
__device__ __forceinline__ double cfr_node(const double *u, const double *ls, double r0, double r1, bool mine, int trav, size_t row, double *g_R, double *g_S,
                                           double *g_L, double wpos, double wneg, double wstrat) {
    const double v = cfr_value<B>(u, ls);
    Row4 R = load_row(g_R + row * 4);
    if (mine) {
        Row4 S = load_row(g_S + row * 4);
        double dR[B], dS[B];
        cfr_increments<B>(u, ls, v, trav == 0 ? r0 : r1, trav == 0 ? r1 : r0, dR, dS);
        cfr_apply<B>(R, S, dR, dS, wpos, wneg, wstrat);
        store_row(g_R + row * 4, R);
        store_row(g_S + row * 4, S);
    }
    Row4 L = {{0.0, 0.0, 0.0, 0.0}};
    scopa::regret_match<B>(R.x, L.x);
    store_row(g_L + row * 4, L);
    return v;
}

// ---- launch 1 of a traversal: the 256 depth-4 subtrees ---------------------------------------------------------------------------------
// LDS: kSubLds (scopa_team_passes.h).  Regret and strategy rows are touched once, on the way up, and stream between HBM and registers.
template <int D>
__device__ __forceinline__ void sub_update_level(int g, int trav, const double *s_sig, const double *s_r0, const double *s_r1, double *s_val, double *g_R, double *g_S,
                                                 double *g_L, double wpos, double wneg, double wstrat, int tid) {
    constexpr int b = t_branch(D), w = s_width(D), lo = s_offset(D), lo1 = s_offset(D + 1);
    for (int j = tid; j < w; j += kSubThreads) {
        double u[b], ls[b];
#pragma unroll
        for (int c = 0; c < b; c++) { u[c] = s_val[lo1 + j * b + c]; ls[c] = s_sig[(lo + j) * 4 + c]; }
        s_val[lo + j] = cfr_node<b>(u, ls, s_r0[lo + j], s_r1[lo + j], t_team(D) == trav, trav, (size_t)t_offset(D) + (size_t)g * w + j, g_R, g_S, g_L, wpos, wneg, wstrat);
    }
    __syncthreads();
}

__global__ void __launch_bounds__(kSubThreads)
k_team_cfr_sub(double *g_R, double *g_S, double *g_L, const int8_t *__restrict__ g_r2, double *g_lrs /* the traverser's [331776] */, double *__restrict__ g_sub /*[256]*/,
               int trav, double wpos, double wneg, double wstrat) {
    extern __shared__ double s_team[];
    double *s_sig = s_team, *s_r0 = s_sig + kSubRows * 4, *s_r1 = s_r0 + kSubRows, *s_val = s_r1 + kSubRows;
    const int g = blockIdx.x, tid = threadIdx.x;
    // the subtree's rows of level d are consecutive in the level-major table
#pragma unroll
    for (int d = kCutDepth; d < 12; d++) {
        const double *src = g_L + ((size_t)t_offset(d) + (size_t)g * s_width(d)) * 4;
        for (int k = tid; k < s_width(d) * 4; k += kSubThreads) s_sig[s_offset(d) * 4 + k] = src[k];
    }
    if (tid == 0) sub_root_reaches(g, g_L, [](int row) { return row; }, s_r0[0], s_r1[0]);
    __syncthreads();
    sub_reach_pass(s_sig, s_r0, s_r1, tid);
    // depth 11 -> the depth-12 nodes: the traverser's reach there is its reach at all four forced plies below (sigma = 1), hence what every forced node of the
    // traverser's adds to its strategy_sum; the terminal's reward for the traverser (0.5 * r2 of its team, exact)
    for (int j = tid; j < kSubLeaves; j += kSubThreads) {
        constexpr int lo = s_offset(11);
        const int par = j >> 1, a = j & 1;
        const double sg = s_sig[(lo + par) * 4 + a];
        const double reach = trav == 0 ? s_r0[lo + par] : s_r1[lo + par] * sg;   // team 1 moves at depth 11
        const size_t leaf = (size_t)g * kSubLeaves + j;
        g_lrs[leaf] = (g_lrs[leaf] + reach) * wstrat;
        s_val[kSubRows + j] = leaf_value(g_r2[leaf], trav);
    }
    __syncthreads();
#define SC_TEAM_UP(D) sub_update_level<D>(g, trav, s_sig, s_r0, s_r1, s_val, g_R, g_S, g_L, wpos, wneg, wstrat, tid)
    SC_TEAM_UP(11); SC_TEAM_UP(10); SC_TEAM_UP(9); SC_TEAM_UP(8); SC_TEAM_UP(7); SC_TEAM_UP(6); SC_TEAM_UP(5); SC_TEAM_UP(4);
#undef SC_TEAM_UP
    if (tid == 0) g_sub[g] = s_val[0];
}

// ---- launch 2: depths 3..0 from the 256 subtree values -----------------------------------------------------------------------------------
template <int D>
__device__ __forceinline__ void top_update_level(int trav, const double *s_sig, const double *s_r0, const double *s_r1, double *s_val, double *g_R, double *g_S, double *g_L,
                                                 double wpos, double wneg, double wstrat, int tid) {
    constexpr int w = t_width(D), lo = t_offset(D), lo1 = t_offset(D + 1);
    for (int j = tid; j < w; j += kSubThreads) {
        double u[4], ls[4];
#pragma unroll
        for (int c = 0; c < 4; c++) { u[c] = s_val[lo1 + j * 4 + c]; ls[c] = s_sig[(lo + j) * 4 + c]; }
        s_val[lo + j] = cfr_node<4>(u, ls, s_r0[lo + j], s_r1[lo + j], t_team(D) == trav, trav, (size_t)(lo + j), g_R, g_S, g_L, wpos, wneg, wstrat);
    }
    __syncthreads();
}

__global__ void __launch_bounds__(kSubThreads)
k_team_cfr_top(double *g_R, double *g_S, double *g_L, const double *__restrict__ g_sub, double *__restrict__ g_root /* one value, or NULL */, int trav, double wpos, double wneg,
               double wstrat) {
    __shared__ double s_sig[kTopRows * 4], s_r0[kTopRows], s_r1[kTopRows], s_val[kTopRows + kSubtrees];
    const int tid = threadIdx.x;
    for (int k = tid; k < kTopRows * 4; k += kSubThreads) s_sig[k] = g_L[k];
    for (int k = tid; k < kSubtrees; k += kSubThreads) s_val[kTopRows + k] = g_sub[k];
    if (tid == 0) { s_r0[0] = 1.0; s_r1[0] = 1.0; }
    __syncthreads();
    top_reach_pass(s_sig, s_r0, s_r1, tid);
#define SC_TEAM_UP(D) top_update_level<D>(trav, s_sig, s_r0, s_r1, s_val, g_R, g_S, g_L, wpos, wneg, wstrat, tid)
    SC_TEAM_UP(3); SC_TEAM_UP(2); SC_TEAM_UP(1); SC_TEAM_UP(0);
#undef SC_TEAM_UP
    if (tid == 0 && g_root) g_root[0] = s_val[0];
}

// ---- the value pass (value_node and its modes: scopa_team_passes.h) ---------------------------------------------------------------------------
template <int D>
__device__ __forceinline__ void sub_value_level(int g, const TeamPlay &pl, double *s_val, double *g_out, int tid) {
    constexpr int b = t_branch(D), w = s_width(D), lo = s_offset(D), lo1 = s_offset(D + 1);
    for (int j = tid; j < w; j += kSubThreads) {
        double u[b];
#pragma unroll
        for (int c = 0; c < b; c++) u[c] = s_val[lo1 + j * b + c];
        s_val[lo + j] = value_node<b>(u, t_team(D), pl, (size_t)t_offset(D) + (size_t)g * w + j, g_out);
    }
    __syncthreads();
}

__global__ void __launch_bounds__(kSubThreads)
k_team_value_sub(const int8_t *__restrict__ g_r2, TeamPlay pl, double *g_out, double *__restrict__ g_sub) {
    __shared__ double s_val[kSubRows + kSubLeaves];
    const int g = blockIdx.x, tid = threadIdx.x;
    for (int j = tid; j < kSubLeaves; j += kSubThreads) {
        s_val[kSubRows + j] = leaf_value(g_r2[(size_t)g * kSubLeaves + j], pl.persp);
    }
    __syncthreads();
    sub_value_level<11>(g, pl, s_val, g_out, tid); sub_value_level<10>(g, pl, s_val, g_out, tid); sub_value_level<9>(g, pl, s_val, g_out, tid);
    sub_value_level<8>(g, pl, s_val, g_out, tid); sub_value_level<7>(g, pl, s_val, g_out, tid); sub_value_level<6>(g, pl, s_val, g_out, tid);
    sub_value_level<5>(g, pl, s_val, g_out, tid); sub_value_level<4>(g, pl, s_val, g_out, tid);
    if (tid == 0) g_sub[g] = s_val[0];
}

__global__ void __launch_bounds__(kSubThreads)
k_team_value_top(TeamPlay pl, double *g_out, const double *__restrict__ g_sub, double *__restrict__ g_value /* one value */) {
    __shared__ double s_val[kTopRows + kSubtrees];
    const int tid = threadIdx.x;
    for (int k = tid; k < kSubtrees; k += kSubThreads) s_val[kTopRows + k] = g_sub[k];
    __syncthreads();
#pragma unroll
    for (int d = kCutDepth - 1; d >= 0; d--) {
        for (int j = tid; j < t_width(d); j += kSubThreads) {
            double u[4];
#pragma unroll
            for (int c = 0; c < 4; c++) u[c] = s_val[t_offset(d + 1) + j * 4 + c];
            s_val[t_offset(d) + j] = value_node<4>(u, t_team(d), pl, (size_t)(t_offset(d) + j), g_out);
        }
        __syncthreads();
    }
    if (tid == 0) g_value[0] = s_val[0];
}

// ---- small kernels: a lane per depth-12 node or per row -----------------------------------------------------------------------------------
// The payoff of every depth-12 node: 16 steps from the root, the path's digits taken from the index (first ply most significant), the forced plies
// play the one card left.
__global__ void __launch_bounds__(256)
k_team_leaves(scopa_team_state root, int8_t *__restrict__ g_r2) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= kTLeaves) return;
    g_r2[i] = (int8_t)team_leaf_r2(root, i);
}

// the reset state of the tables: regret and strategy sums 0, sigma uniform over the legal slots (InfoNode.__post_init__, vanilla_cfr.py:15-21)
__global__ void __launch_bounds__(256)
k_team_sigma_uniform(double *__restrict__ g_L) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= kTChoice) return;
    const int b = t_branch(depth_of_row(row));
    Row4 r;
#pragma unroll
    for (int c = 0; c < 4; c++) r.x[c] = c < b ? 1.0 / (double)b : 0.0;
    store_row(g_L + (size_t)row * 4, r);
}

// InfoNode.policy (vanilla_cfr.py:32-39): the strategy sums normalised, np.sum left to right; uniform where the sum is not > 0
__global__ void __launch_bounds__(256)
k_team_average_policy(const double *__restrict__ g_S, double *__restrict__ g_pol) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= kTChoice) return;
    store_row(g_pol + (size_t)row * 4, average_row(load_row(g_S + (size_t)row * 4), t_branch(depth_of_row(row))));
}

}  // namespace

namespace scopa {
void team_release(scopa_ctx *ctx) {
    scopa_team_solver *t = ctx->team;
    if (!t) return;
    void *bufs[] = {t->d_r2, t->d_R, t->d_S, t->d_L, t->d_lrs, t->d_sub, t->d_avg, t->d_root};
    for (void *b : bufs) if (b) (void)hipFree(b);
    team_mccfr_release(t);
    team_xplay_release(&t->xp);
    delete t;
    ctx->team = nullptr;
}
}  // namespace scopa

namespace {

constexpr size_t kTableBytes = sizeof(double) * 4 * (size_t)kTChoice, kLrsBytes = sizeof(double) * 2 * (size_t)kTLeaves;

int32_t team_reset_tables(scopa_ctx *ctx, scopa_team_solver *t) {
    SC_HIP(ctx, hipMemsetAsync(t->d_R, 0, kTableBytes, ctx->stream));
    SC_HIP(ctx, hipMemsetAsync(t->d_S, 0, kTableBytes, ctx->stream));
    SC_HIP(ctx, hipMemsetAsync(t->d_lrs, 0, kLrsBytes, ctx->stream));
    hipLaunchKernelGGL(k_team_sigma_uniform, dim3((kTChoice + 255) / 256), dim3(256), 0, ctx->stream, t->d_L);
    SC_HIP(ctx, hipGetLastError());
    return scopa::team_mccfr_reset(ctx, t);
}

// one value pass = the two launches; the root value goes to t->d_sub[kSubtrees + slot]
int32_t team_value_pass(scopa_ctx *ctx, scopa_team_solver *t, const TeamPlay &pl, double *d_out, int slot) {
    hipLaunchKernelGGL(k_team_value_sub, dim3(kSubtrees), dim3(kSubThreads), 0, ctx->stream, (const int8_t *)t->d_r2, pl, d_out, t->d_sub);
    SC_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_team_value_top, dim3(1), dim3(kSubThreads), 0, ctx->stream, pl, d_out, (const double *)t->d_sub, t->d_sub + kSubtrees + slot);
    SC_HIP(ctx, hipGetLastError());
    return SCOPA_OK;
}

// the two launches of one traversal (part 0: the subtrees, 1: the top, which leaves the root value at d_root if that is not NULL)
int32_t team_cfr_launch(scopa_ctx *ctx, scopa_team_solver *t, int part, int trav, double wpos, double wneg, double wstrat, double *d_root) {
    if (part == 0) {
        SC_LDS_ATTR(ctx, scopa::kLdsTeamCfr, k_team_cfr_sub, (int)kSubLds);
        hipLaunchKernelGGL(k_team_cfr_sub, dim3(kSubtrees), dim3(kSubThreads), kSubLds, ctx->stream, t->d_R, t->d_S, t->d_L, (const int8_t *)t->d_r2,
                           t->d_lrs + (size_t)trav * kTLeaves, t->d_sub, trav, wpos, wneg, wstrat);
    } else {
        hipLaunchKernelGGL(k_team_cfr_top, dim3(1), dim3(kSubThreads), 0, ctx->stream, t->d_R, t->d_S, t->d_L, (const double *)t->d_sub, d_root, trav, wpos, wneg, wstrat);
    }
    SC_HIP(ctx, hipGetLastError());
    return SCOPA_OK;
}

int32_t team_values_to_host(scopa_ctx *ctx, scopa_team_solver *t, double *h, int n) {
    SC_HIP(ctx, hipMemcpyAsync(h, t->d_sub + kSubtrees, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SCOPA_OK;
}

}  // namespace

extern "C" {

int32_t scopa_team_set_deal(scopa_ctx *ctx, const uint8_t perm16[16]) {
    if (!ctx || !perm16) return SCOPA_EINVAL;
    scopa_team_state root;
    const int32_t rc0 = scopa_team_state_init(perm16, &root);
    SC_REQUIRE(ctx, rc0 == SCOPA_OK, SCOPA_EINVAL, "scopa_team_set_deal: perm16 is not a permutation of 0..15");
    SC_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->team) {
        scopa_team_solver *n = new (std::nothrow) scopa_team_solver();
        if (!n) return fail(ctx, SCOPA_ENOMEM, "scopa_team_set_deal: out of host memory");
        ctx->team = n;
        const bool ok = hipMalloc(&n->d_r2, kTLeaves) == hipSuccess && hipMalloc(&n->d_R, kTableBytes) == hipSuccess && hipMalloc(&n->d_S, kTableBytes) == hipSuccess &&
                        hipMalloc(&n->d_L, kTableBytes) == hipSuccess && hipMalloc(&n->d_lrs, kLrsBytes) == hipSuccess &&
                        hipMalloc(&n->d_sub, sizeof(double) * (kSubtrees + 8)) == hipSuccess;
        if (!ok) { scopa::team_release(ctx); return fail(ctx, SCOPA_ENOMEM, "scopa_team_set_deal: out of device memory"); }
    }
    scopa_team_solver *t = ctx->team;
    t->has_deal = false;
    t->root = root;
    t->xp.leaf_sc_valid = false;   // rebuilt by the next cross-play or match (scopa_team_xplay.hip)
    hipLaunchKernelGGL(k_team_leaves, dim3((kTLeaves + 255) / 256), dim3(256), 0, ctx->stream, root, t->d_r2);
    SC_HIP(ctx, hipGetLastError());
    const int32_t rc = team_reset_tables(ctx, t);
    if (rc != SCOPA_OK) return rc;
    t->has_deal = true;
    return SCOPA_OK;
}

int32_t scopa_team_tree_counts(scopa_ctx *ctx, int32_t *n_choice, int32_t *n_leaves, int32_t *n_infosets) {
    if (!ctx) return SCOPA_EINVAL;
    SC_TEAM_READY(ctx, "scopa_team_tree_counts");
    (void)t;
    if (n_choice) *n_choice = kTChoice;
    if (n_leaves) *n_leaves = kTLeaves;
    if (n_infosets) *n_infosets = kTInfosets;
    return SCOPA_OK;
}

int32_t scopa_team_tree_leaves(scopa_ctx *ctx, int8_t *h_r2) {
    if (!ctx || !h_r2) return SCOPA_EINVAL;
    SC_TEAM_READY(ctx, "scopa_team_tree_leaves");
    SC_HIP(ctx, hipMemcpyAsync(h_r2, t->d_r2, kTLeaves, hipMemcpyDeviceToHost, ctx->stream));
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SCOPA_OK;
}

int32_t scopa_team_tables_reset(scopa_ctx *ctx) {
    if (!ctx) return SCOPA_EINVAL;
    SC_TEAM_READY(ctx, "scopa_team_tables_reset");
    return team_reset_tables(ctx, t);
}

int32_t scopa_team_tables_get(scopa_ctx *ctx, double *h_regret, double *h_strategy, double *h_local, double *h_leaf_reach_sum) {
    if (!ctx) return SCOPA_EINVAL;
    SC_TEAM_READY(ctx, "scopa_team_tables_get");
    if (h_regret) SC_HIP(ctx, hipMemcpyAsync(h_regret, t->d_R, kTableBytes, hipMemcpyDeviceToHost, ctx->stream));
    if (h_strategy) SC_HIP(ctx, hipMemcpyAsync(h_strategy, t->d_S, kTableBytes, hipMemcpyDeviceToHost, ctx->stream));
    if (h_local) SC_HIP(ctx, hipMemcpyAsync(h_local, t->d_L, kTableBytes, hipMemcpyDeviceToHost, ctx->stream));
    if (h_leaf_reach_sum) SC_HIP(ctx, hipMemcpyAsync(h_leaf_reach_sum, t->d_lrs, kLrsBytes, hipMemcpyDeviceToHost, ctx->stream));
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SCOPA_OK;
}

int32_t scopa_team_tables_set(scopa_ctx *ctx, const double *h_regret, const double *h_strategy, const double *h_local, const double *h_leaf_reach_sum) {
    if (!ctx) return SCOPA_EINVAL;
    SC_TEAM_READY(ctx, "scopa_team_tables_set");
    if (h_regret) SC_HIP(ctx, hipMemcpyAsync(t->d_R, h_regret, kTableBytes, hipMemcpyHostToDevice, ctx->stream));
    if (h_strategy) SC_HIP(ctx, hipMemcpyAsync(t->d_S, h_strategy, kTableBytes, hipMemcpyHostToDevice, ctx->stream));
    if (h_local) SC_HIP(ctx, hipMemcpyAsync(t->d_L, h_local, kTableBytes, hipMemcpyHostToDevice, ctx->stream));
    if (h_leaf_reach_sum) SC_HIP(ctx, hipMemcpyAsync(t->d_lrs, h_leaf_reach_sum, kLrsBytes, hipMemcpyHostToDevice, ctx->stream));
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the host buffers are only borrowed for the call
    return SCOPA_OK;
}

int32_t scopa_team_cfr_iterate(scopa_ctx *ctx, int32_t n_iters, const double *h_w, double *h_root_values) {
    if (!ctx || n_iters < 0 || n_iters > (1 << 20)) return SCOPA_EINVAL;
    SC_TEAM_READY(ctx, "scopa_team_cfr_iterate");
    if (n_iters == 0) return SCOPA_OK;
    SC_REQUIRE(ctx, !h_w || scopa::cfr_weights_ok(h_w, n_iters), SCOPA_EINVAL, "scopa_team_cfr_iterate: every weight must be finite and in [0, 1]");
    if (h_root_values && t->root_cap < (size_t)n_iters * 2) {
        if (t->d_root) SC_HIP(ctx, hipFree(t->d_root));
        t->d_root = nullptr; t->root_cap = 0;
        SC_HIP(ctx, hipMalloc(&t->d_root, sizeof(double) * 2 * (size_t)n_iters));
        t->root_cap = (size_t)n_iters * 2;
    }
    for (int32_t it = 0; it < n_iters; it++) {
        // the weights are launch arguments: (1, 1, 1) multiplies every cell by 1.0, which changes no bit
        const double wpos = h_w ? h_w[it * 3 + 0] : 1.0, wneg = h_w ? h_w[it * 3 + 1] : 1.0, wstrat = h_w ? h_w[it * 3 + 2] : 1.0;
        for (int p = 0; p < 2; p++)   // for i in range(num_players): _cfr_recursive(root, i, 1.0, 1.0)  (vanilla_cfr.py:108-110)
            for (int part = 0; part < 2; part++) {
                const int32_t rc = team_cfr_launch(ctx, t, part, p, wpos, wneg, wstrat, h_root_values ? t->d_root + (size_t)it * 2 + p : nullptr);
                if (rc != SCOPA_OK) return rc;
            }
    }
    if (h_root_values) {
        SC_HIP(ctx, hipMemcpyAsync(h_root_values, t->d_root, sizeof(double) * 2 * (size_t)n_iters, hipMemcpyDeviceToHost, ctx->stream));
        SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return SCOPA_OK;
}

int32_t scopa_team_cfr_traverse(scopa_ctx *ctx, int32_t traverser, double *h_value) {
    if (!ctx || !h_value || traverser < 0 || traverser > 1) return SCOPA_EINVAL;
    SC_TEAM_READY(ctx, "scopa_team_cfr_traverse");
    for (int part = 0; part < 2; part++) {
        const int32_t rc = team_cfr_launch(ctx, t, part, traverser, 1.0, 1.0, 1.0, t->d_sub + kSubtrees);
        if (rc != SCOPA_OK) return rc;
    }
    return team_values_to_host(ctx, t, h_value, 1);
}

int32_t scopa_team_cfr_launch(scopa_ctx *ctx, int32_t traverser, int32_t part) {
    if (!ctx || traverser < 0 || traverser > 1 || part < 0 || part > 1) return SCOPA_EINVAL;
    SC_TEAM_READY(ctx, "scopa_team_cfr_launch");
    return team_cfr_launch(ctx, t, part, traverser, 1.0, 1.0, 1.0, nullptr);
}

int32_t scopa_team_exploitability(scopa_ctx *ctx, const double *d_policy, double *h_out4, double *d_br) {
    if (!ctx || !h_out4) return SCOPA_EINVAL;
    SC_TEAM_READY(ctx, "scopa_team_exploitability");
    SC_REQUIRE(ctx, (((uintptr_t)d_policy | (uintptr_t)d_br) & 31) == 0, SCOPA_EINVAL, "scopa_team_exploitability: tables must be 32-byte aligned");
    if (!d_policy) {
        if (!t->d_avg) SC_HIP(ctx, hipMalloc(&t->d_avg, kTableBytes));
        hipLaunchKernelGGL(k_team_average_policy, dim3((kTChoice + 255) / 256), dim3(256), 0, ctx->stream, (const double *)t->d_S, t->d_avg);
        SC_HIP(ctx, hipGetLastError());
        d_policy = t->d_avg;
    }
    for (int br = 0; br < 3; br++) {   // 0 / 1: that team responds, valued for itself; 2: nobody does, valued for team 0
        TeamPlay pl;
        pl.tab[0] = pl.tab[1] = d_policy;
        pl.mode[0] = br == 0 ? kMaximise : kFollow;
        pl.mode[1] = br == 1 ? kMaximise : kFollow;
        pl.persp = br == 1 ? 1 : 0;
        const int32_t rc = team_value_pass(ctx, t, pl, br < 2 && d_br ? d_br + (size_t)br * 4 * kTChoice : nullptr, br);
        if (rc != SCOPA_OK) return rc;
    }
    double v[3];
    const int32_t rc = team_values_to_host(ctx, t, v, 3);
    if (rc != SCOPA_OK) return rc;
    h_out4[0] = (v[0] + v[1]) / 2.0; h_out4[1] = v[0]; h_out4[2] = v[1]; h_out4[3] = v[2];
    return SCOPA_OK;
}

int32_t scopa_team_minimax(scopa_ctx *ctx, double *h_value, double *d_policy_out) {
    if (!ctx || !h_value) return SCOPA_EINVAL;
    SC_TEAM_READY(ctx, "scopa_team_minimax");
    SC_REQUIRE(ctx, ((uintptr_t)d_policy_out & 31) == 0, SCOPA_EINVAL, "scopa_team_minimax: the table must be 32-byte aligned");
    TeamPlay pl;
    pl.tab[0] = pl.tab[1] = nullptr;
    pl.mode[0] = pl.mode[1] = kMaximise;
    pl.persp = 0;
    const int32_t rc = team_value_pass(ctx, t, pl, d_policy_out, 0);
    if (rc != SCOPA_OK) return rc;
    return team_values_to_host(ctx, t, h_value, 1);
}

int32_t scopa_team_policy_value(scopa_ctx *ctx, const double *d_policy_a, const double *d_policy_b, double *h_out) {
    if (!ctx || !h_out) return SCOPA_EINVAL;
    SC_TEAM_READY(ctx, "scopa_team_policy_value");
    SC_REQUIRE(ctx, (((uintptr_t)d_policy_a | (uintptr_t)d_policy_b) & 31) == 0, SCOPA_EINVAL, "scopa_team_policy_value: tables must be 32-byte aligned");
    TeamPlay pl;
    pl.tab[0] = d_policy_a; pl.tab[1] = d_policy_b;
    pl.mode[0] = d_policy_a ? kFollow : kUniform;
    pl.mode[1] = d_policy_b ? kFollow : kUniform;
    pl.persp = 0;
    const int32_t rc = team_value_pass(ctx, t, pl, nullptr, 0);
    if (rc != SCOPA_OK) return rc;
    return team_values_to_host(ctx, t, h_out, 1);
}

}  // extern "C"
