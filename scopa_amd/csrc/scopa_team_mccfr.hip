// scopa_team_mccfr.hip -- external-sampling MCCFR on Team MiniScopa TPI for one fixed deal: the reference's MCCFRTrainer._sample / .iteration
// (src/algorithms/mc_cfr.py:37-92) run on TPIMiniScopaGame (src/envs/openspiel_team_mini_scopa.py), in two forms over the tables of scopa_team_cfr.hip.
//
// The recursion's shape is fixed.  _sample draws one np.random.choice at every decision visit (:55), recurses once into the sampled child (:67) and,
// at a traverser's node with b cards, b more times, into every child in order (:72-78): a visit instance of a traverser ply has b + 1 child instances
// (slot 0 the sampled child, slot 1 + c child c), one of any other ply has one.  Level d of the instance tree therefore holds the product of these
// multipliers above it, whatever is drawn: 9 781 instances down to depth 11 for traverser 0 (2 583 for traverser 1), of which 1 731 are the traverser's,
// and 3 600 arrivals at depth-12 nodes.  The forced tail below a depth-12 node is 11 (5) more visits with sigma = [1.]: the team's first forced ply
// once, its second twice, four terminals; a forced traverser node adds 0 to its regret and 1.0 to its strategy_sum per visit.  An instance's return
// value is the payoff of the leaf its sampled descent ends in (:86), an integer reward x2.
//
//   k_team_mccfr_replay   the reference's own order on one lane, live tables, uniforms from the host: the bit-exactness anchor
//   k_team_mccfr_walk     the throughput path: a workgroup expands a traversal level by level through LDS against frozen regrets
//   k_team_mccfr_apply    a lane per row: regrets, strategy sums and local_strategy of the rows the walks touched; the delta buffer back to zero
//
// The walk keeps one record per TRAVERSER instance (row, sampled action, opponent reach, own sampling probability: 20 bytes x 1 731); the plies of
// the other team between two traverser plies are a chain of single children, walked in registers by the lane that creates the next record.  Values
// come back up as int8 (reward x2).  A row's regret increment is weight * (cfv - v), weight = opponent reach / sampling probability or 0 (:79-83).
// The root row receives one increment per traversal: rows of depths 0..4 (341 rows) accumulate in LDS per workgroup (ds_add_f64) and are flushed once,
// deeper rows go straight to the delta buffer as float64 atomics.
#include <string.h>

#include "scopa_team_mccfr_walk.h"
#include "scopa_tree_passes.h"

using scopa::fail;

namespace {

// ---- the replay: MCCFRTrainer._sample in the reference's visit order, one lane, live tables --------------------------------------------------
struct Replay {
    double *R, *S, *L;
    uint8_t *seen;
    unsigned long long *lv;
    const int8_t *r2;
    const double *u;
    long long upos;
};

// A row is its own infoset and is revisited only through the sample-then-loop pair at its parent, so the row read on entry is still the row at the
// update.  One call site per level (slot 0 = the sampled child, then the loop): twelve bodies per traverser, all frames in registers.
template <int D, int TRAV>
__device__ __forceinline__ double replay_rec(Replay &w, int idx, double reach_opp, double samp_trav) {
    if constexpr (D == 12) {   // the forced tail: its draws are skipped in the stream, its terminal's reward returned (:38-39)
        w.lv[(size_t)TRAV * kTLeaves + idx] += 1ull;
        w.upos += TRAV == 0 ? 11 : 5;
        const int p0 = w.r2[idx];
        return 0.5 * (double)(TRAV == 0 ? p0 : -p0);
    } else {
        constexpr int n = t_branch(D);
        const size_t row = (size_t)t_offset(D) + idx;
        w.seen[row] = 1;   // _get_node (:32-35)
        Row4 R = load_row(w.R + row * 4);
        double sigma[4];
        scopa::mc_sigma(R.x, n, sigma);
        const int a = choice<n>(sigma, w.u[w.upos]);
        w.upos++;
        if constexpr (t_team(D) != TRAV) {
            return replay_rec<D + 1, TRAV>(w, idx * n + a, reach_opp * pick<n>(sigma, a), samp_trav);
        } else {
            double util = 0.0, cfv[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
            for (int k = 0; k <= n; k++) {   // :67, then :72-78
                const int c = k == 0 ? a : k - 1;
                const double val = replay_rec<D + 1, TRAV>(w, idx * n + c, reach_opp, samp_trav * pick<n>(sigma, c));
                util = k == 0 ? val : util;
#pragma unroll
                for (int i = 0; i < n; i++) cfv[i] = k == i + 1 ? val : cfv[i];
            }
            const double v = dot<n>(sigma, cfv);
            const double wt = samp_trav > 0.0 ? reach_opp / samp_trav : 0.0;   // :81-82
            Row4 S = load_row(w.S + row * 4), L = {{0.0, 0.0, 0.0, 0.0}};
#pragma unroll
            for (int i = 0; i < n; i++) {
                R.x[i] += wt * (cfv[i] - v);
                S.x[i] += sigma[i];   // reach_probs[traverser] stays 1.0 (:61-65, :84)
            }
            scopa::regret_match<n>(R.x, L.x);   // what scopa_team_cfr_iterate plays from
            store_row(w.R + row * 4, R);
            store_row(w.S + row * 4, S);
            store_row(w.L + row * 4, L);
            return util;
        }
    }
}

__global__ void __launch_bounds__(64)
k_team_mccfr_replay(double *g_R, double *g_S, double *g_L, uint8_t *g_seen, unsigned long long *g_lv, const int8_t *__restrict__ g_r2, const double *__restrict__ g_u,
                    int n_iters, long long *g_consumed) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    Replay w{g_R, g_S, g_L, g_seen, g_lv, g_r2, g_u, 0};
#pragma unroll 1
    for (int it = 0; it < n_iters; it++) {   // iteration(), :88-92
        replay_rec<0, 0>(w, 0, 1.0, 1.0);
        replay_rec<0, 1>(w, 0, 1.0, 1.0);
    }
    *g_consumed = w.upos;
}

// ---- the walk: scopa_team_mccfr_walk.h, here on the context's own rows ---------------------------------------------------------------------------
// tasks [0, 2 nb): task k is traverser k & 1 of global traversal b0 + (k >> 1); a workgroup takes tasks blockIdx.x, + gridDim.x, ...
__global__ void __launch_bounds__(kWalkThreads)
k_team_mccfr_walk(const double *__restrict__ g_R, uint8_t *g_seen, unsigned long long *g_lv, const int8_t *__restrict__ g_r2, double *g_delta, uint32_t iteration, uint32_t b0,
                  uint32_t nb, uint32_t seed_lo, uint32_t seed_hi) {
    __shared__ WalkLds s;
    const int tid = threadIdx.x;
    for (int k = tid; k < kShallowRows * 5; k += kWalkThreads) s.delta[k] = 0.0;
    __syncthreads();
    for (uint32_t task = blockIdx.x; task < 2u * nb; task += gridDim.x) {
        const Walk<OwnRows> w{g_R, g_seen, g_lv, g_r2, g_delta, b0 + (task >> 1), iteration, seed_lo, seed_hi, OwnRows{}};
        if ((task & 1u) == 0u) walk_one<0>(w, s, tid); else walk_one<1>(w, s, tid);
    }
    for (int k = tid; k < kShallowRows * 5; k += kWalkThreads) {
        const double d = s.delta[k];
        if (d != 0.0) atomicAdd(g_delta + k, d);
    }
}

// regret += delta[:4]; strategy += count * sigma of the regrets before the add; local_strategy = regret matching of the new regrets; delta <- 0.
// A row no traverser instance visited (count 0) received nothing and is left as it is.
__global__ void __launch_bounds__(256)
k_team_mccfr_apply(double *g_R, double *g_S, double *g_L, double *g_delta) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= kTChoice) return;
    double *d = g_delta + (size_t)row * 5;
    const double count = d[4];
    if (count == 0.0) return;
    const int b = t_branch(depth_of_row(row));
    Row4 R = load_row(g_R + (size_t)row * 4), S = load_row(g_S + (size_t)row * 4), L = {{0.0, 0.0, 0.0, 0.0}};
    double sigma[4];
    scopa::mc_sigma(R.x, b, sigma);
#pragma unroll
    for (int c = 0; c < 4; c++) {
        if (c < b) {
            R.x[c] += d[c];
            S.x[c] += count * sigma[c];
        }
        d[c] = 0.0;
    }
    d[4] = 0.0;
    scopa::regret_match_n(b, R.x, L.x);
    store_row(g_R + (size_t)row * 4, R);
    store_row(g_S + (size_t)row * 4, S);
    store_row(g_L + (size_t)row * 4, L);
}

constexpr size_t kSeenBytes = (size_t)kTChoice, kVisitBytes = sizeof(unsigned long long) * 2 * (size_t)kTLeaves, kDeltaBytes = sizeof(double) * 5 * (size_t)kTChoice;

// the sampling solver's buffers, at its first call on the context
int32_t ensure_state(scopa_ctx *ctx, scopa_team_solver *t) {
    if (t->d_delta) return SCOPA_OK;
    const bool ok = hipMalloc(&t->d_seen, kSeenBytes) == hipSuccess && hipMalloc(&t->d_leaf_visits, kVisitBytes) == hipSuccess && hipMalloc(&t->d_consumed, sizeof(long long)) == hipSuccess &&
                    hipMalloc(&t->d_delta, kDeltaBytes) == hipSuccess;
    if (!ok) {
        scopa::team_mccfr_release(t);
        return fail(ctx, SCOPA_ENOMEM, "scopa_team_mccfr: out of device memory");
    }
    return scopa::team_mccfr_reset(ctx, t);
}

int32_t walk_launch(scopa_ctx *ctx, scopa_team_solver *t, uint32_t iteration, uint32_t b0, uint32_t nb) {
    const uint32_t tasks = 2u * nb, resident = 2u * (uint32_t)ctx->n_cus;   // two workgroups per compute unit hold their LDS accumulators for the whole launch
    hipLaunchKernelGGL(k_team_mccfr_walk, dim3(tasks < resident ? tasks : resident), dim3(kWalkThreads), 0, ctx->stream, (const double *)t->d_R, t->d_seen, t->d_leaf_visits,
                       (const int8_t *)t->d_r2, t->d_delta, iteration, b0, nb, (uint32_t)ctx->seed, (uint32_t)(ctx->seed >> 32));
    SC_HIP(ctx, hipGetLastError());
    t->mccfr_decision += (unsigned long long)nb * (kDraws0 + kDraws1);
    t->mccfr_terminal += (unsigned long long)nb * 2ull * kTerminals;
    return SCOPA_OK;
}

int32_t apply_launch(scopa_ctx *ctx, scopa_team_solver *t) {
    hipLaunchKernelGGL(k_team_mccfr_apply, dim3((kTChoice + 255) / 256), dim3(256), 0, ctx->stream, t->d_R, t->d_S, t->d_L, t->d_delta);
    SC_HIP(ctx, hipGetLastError());
    t->mccfr_iteration++;
    return SCOPA_OK;
}

}  // namespace

namespace scopa {

int32_t team_mccfr_reset(scopa_ctx *ctx, scopa_team_solver *t) {
    t->mccfr_iteration = 0;
    t->mccfr_decision = t->mccfr_terminal = 0;
    if (!t->d_delta) return SCOPA_OK;
    SC_HIP(ctx, hipMemsetAsync(t->d_seen, 0, kSeenBytes, ctx->stream));
    SC_HIP(ctx, hipMemsetAsync(t->d_leaf_visits, 0, kVisitBytes, ctx->stream));
    SC_HIP(ctx, hipMemsetAsync(t->d_delta, 0, kDeltaBytes, ctx->stream));
    return SCOPA_OK;
}

void team_mccfr_release(scopa_team_solver *t) {
    void *bufs[] = {t->d_seen, t->d_leaf_visits, t->d_delta, t->d_uniforms, t->d_consumed};
    for (void *b : bufs) if (b) (void)hipFree(b);
    t->d_seen = nullptr; t->d_leaf_visits = nullptr; t->d_delta = nullptr; t->d_uniforms = nullptr; t->d_consumed = nullptr;
    t->uniforms_cap = 0;
}

}  // namespace scopa

extern "C" {

int32_t scopa_team_mccfr_replay(scopa_ctx *ctx, int32_t n_iters, const double *h_uniforms, int64_t n_uniforms, int64_t *consumed) {
    if (!ctx || n_iters < 0 || n_iters > (1 << 20) || n_uniforms < 0 || (n_uniforms > 0 && !h_uniforms)) return SCOPA_EINVAL;
    SC_TEAM_READY(ctx, "scopa_team_mccfr_replay");
    const int64_t need = (int64_t)n_iters * (int64_t)(kDraws0 + kDraws1);
    SC_REQUIRE(ctx, n_uniforms >= need, SCOPA_EINVAL, "scopa_team_mccfr_replay: the uniform stream is shorter than 69 964 per iteration");
    if (consumed) *consumed = 0;
    if (n_iters == 0) return SCOPA_OK;
    const int32_t rc = ensure_state(ctx, t);
    if (rc != SCOPA_OK) return rc;
    if (t->uniforms_cap < (size_t)need) {
        if (t->d_uniforms) SC_HIP(ctx, hipFree(t->d_uniforms));
        t->d_uniforms = nullptr; t->uniforms_cap = 0;
        SC_HIP(ctx, hipMalloc(&t->d_uniforms, sizeof(double) * (size_t)need));
        t->uniforms_cap = (size_t)need;
    }
    SC_HIP(ctx, hipMemcpyAsync(t->d_uniforms, h_uniforms, sizeof(double) * (size_t)need, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_team_mccfr_replay, dim3(1), dim3(64), 0, ctx->stream, t->d_R, t->d_S, t->d_L, t->d_seen, t->d_leaf_visits, (const int8_t *)t->d_r2, (const double *)t->d_uniforms,
                       n_iters, t->d_consumed);
    SC_HIP(ctx, hipGetLastError());
    long long used = 0;
    SC_HIP(ctx, hipMemcpyAsync(&used, t->d_consumed, sizeof used, hipMemcpyDeviceToHost, ctx->stream));
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the host stream is only borrowed for the call
    t->mccfr_decision += (unsigned long long)need;
    t->mccfr_terminal += (unsigned long long)n_iters * 2ull * kTerminals;
    if (consumed) *consumed = used;
    SC_REQUIRE(ctx, used == need, SCOPA_ESTATE, "scopa_team_mccfr_replay: the walk did not read 69 964 uniforms per iteration");
    return SCOPA_OK;
}

int32_t scopa_team_mccfr_traverse(scopa_ctx *ctx, uint32_t iteration, uint32_t b0, uint32_t nb) {
    if (!ctx || nb > (1u << 24) || b0 > 0xFFFFFFFFu - nb) return SCOPA_EINVAL;
    SC_TEAM_READY(ctx, "scopa_team_mccfr_traverse");
    const int32_t rc = ensure_state(ctx, t);
    if (rc != SCOPA_OK || nb == 0) return rc;
    return walk_launch(ctx, t, iteration, b0, nb);
}

int32_t scopa_team_mccfr_apply(scopa_ctx *ctx) {
    if (!ctx) return SCOPA_EINVAL;
    SC_TEAM_READY(ctx, "scopa_team_mccfr_apply");
    const int32_t rc = ensure_state(ctx, t);
    if (rc != SCOPA_OK) return rc;
    return apply_launch(ctx, t);
}

int32_t scopa_team_mccfr_iterate(scopa_ctx *ctx, uint32_t batch, uint32_t n_iters) {
    if (!ctx || batch == 0 || batch > (1u << 24)) return SCOPA_EINVAL;
    SC_TEAM_READY(ctx, "scopa_team_mccfr_iterate");
    int32_t rc = ensure_state(ctx, t);
    for (uint32_t it = 0; it < n_iters && rc == SCOPA_OK; it++) {
        rc = walk_launch(ctx, t, t->mccfr_iteration, 0, batch);
        if (rc == SCOPA_OK) rc = apply_launch(ctx, t);
    }
    return rc;
}

int32_t scopa_team_mccfr_counters(scopa_ctx *ctx, uint64_t *decision_visits, uint64_t *terminal_visits, uint32_t *iterations) {
    if (!ctx) return SCOPA_EINVAL;
    SC_TEAM_READY(ctx, "scopa_team_mccfr_counters");
    if (decision_visits) *decision_visits = t->mccfr_decision;
    if (terminal_visits) *terminal_visits = t->mccfr_terminal;
    if (iterations) *iterations = t->mccfr_iteration;
    return SCOPA_OK;
}

int32_t scopa_team_mccfr_delta_get(scopa_ctx *ctx, double *h_delta) {
    if (!ctx || !h_delta) return SCOPA_EINVAL;
    SC_TEAM_READY(ctx, "scopa_team_mccfr_delta_get");
    const int32_t rc = ensure_state(ctx, t);
    if (rc != SCOPA_OK) return rc;
    SC_HIP(ctx, hipMemcpyAsync(h_delta, t->d_delta, kDeltaBytes, hipMemcpyDeviceToHost, ctx->stream));
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SCOPA_OK;
}

int32_t scopa_team_mccfr_visits_get(scopa_ctx *ctx, uint8_t *h_seen, uint64_t *h_leaf_visits) {
    if (!ctx) return SCOPA_EINVAL;
    SC_TEAM_READY(ctx, "scopa_team_mccfr_visits_get");
    const int32_t rc = ensure_state(ctx, t);
    if (rc != SCOPA_OK) return rc;
    if (h_seen) SC_HIP(ctx, hipMemcpyAsync(h_seen, t->d_seen, kSeenBytes, hipMemcpyDeviceToHost, ctx->stream));
    if (h_leaf_visits) SC_HIP(ctx, hipMemcpyAsync(h_leaf_visits, t->d_leaf_visits, kVisitBytes, hipMemcpyDeviceToHost, ctx->stream));
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SCOPA_OK;
}

}  // extern "C"
