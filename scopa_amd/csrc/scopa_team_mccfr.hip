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

#include "scopa_mccfr_sigma.h"
#include "scopa_philox.h"
#include "scopa_team_solver.h"
#include "scopa_tree_passes.h"

using scopa::fail;

namespace {

// ---- the instance tree ---------------------------------------------------------------------------------------------------------------------
template <int TRAV> __host__ __device__ constexpr int i_mult(int d) { return t_team(d) == TRAV ? t_branch(d) + 1 : 1; }
template <int TRAV> __host__ __device__ constexpr int i_width(int d) { int w = 1; for (int k = 0; k < d; k++) w *= i_mult<TRAV>(k); return w; }
template <int TRAV> __host__ __device__ constexpr int i_offset(int d) { int o = 0; for (int k = 0; k < d; k++) o += i_width<TRAV>(k); return o; }
// the traverser's K-th ply (0..5), the cards it plays from, and its instances: 1, 5, 25, 100, 400, 1 200 for either traverser
template <int TRAV> __host__ __device__ constexpr int s_depth(int k) { return 4 * (k >> 1) + (k & 1) + 2 * TRAV; }
__host__ __device__ constexpr int s_cards(int k) { return 4 - (k >> 1); }
__host__ __device__ constexpr int s_count(int k) { int w = 1; for (int j = 0; j < k; j++) w *= s_cards(j) + 1; return w; }
__host__ __device__ constexpr int s_first(int k) { int o = 0; for (int j = 0; j < k; j++) o += s_count(j); return o; }
constexpr int kStages = 6, kStageRecs = s_first(kStages), kArrivals = s_count(kStages);
constexpr int kShallowRows = t_offset(5);   // rows of depths 0..4, accumulated in LDS
constexpr unsigned long long kDraws0 = 49381, kDraws1 = 20583, kTerminals = 4ull * kArrivals;   // per traversal, forced tails included
static_assert(kStageRecs == 1731 && kArrivals == 3600 && kShallowRows == 341, "instance tree");
static_assert(i_offset<0>(12) == 9781 && i_offset<1>(12) == 2583 && i_width<0>(12) == kArrivals && i_width<1>(12) == kArrivals, "instance tree");
static_assert(i_offset<0>(12) + 11 * kArrivals == kDraws0 && i_offset<1>(12) + 5 * kArrivals == kDraws1, "draws per traversal");
static_assert(s_depth<0>(5) == 9 && s_depth<1>(5) == 11 && s_depth<1>(0) == 2, "traverser plies");
constexpr uint32_t kPhiloxTag = 64u;   // counter word 3 = 64 + traverser (0, 1: k_mccfr_traverse; 4, 5: SDCFR; 32: full-game playouts; 48: team playouts)

// np.random.choice(legal, p=sigma) (mc_cfr.py:55): cdf = cumsum(p); cdf /= cdf[-1]; searchsorted(cdf, u, side="right") -- the rule of k_mccfr_replay
template <int N>
__device__ __forceinline__ int choice(const double *sigma, double u) {
    double cdf[N];
    double c = sigma[0];
    cdf[0] = c;
#pragma unroll
    for (int i = 1; i < N; i++) { c += sigma[i]; cdf[i] = c; }
    const double last = cdf[N - 1];
    int a = 0;
#pragma unroll
    for (int i = 0; i < N; i++) a += cdf[i] / last <= u ? 1 : 0;
    return a < N - 1 ? a : N - 1;
}
// x[a] by compares: the values are passed one by one, so that no run-time index ever addresses the array (that would put it in scratch memory)
__device__ __forceinline__ double pick4(double x0, double x1, double x2, double x3, int a) {
    double r = x0;
    r = a == 1 ? x1 : r;
    r = a == 2 ? x2 : r;
    r = a == 3 ? x3 : r;
    return r;
}
template <int N>
__device__ __forceinline__ double pick(const double *x, int a) { return pick4(x[0], N > 1 ? x[1] : 0.0, N > 2 ? x[2] : 0.0, N > 3 ? x[3] : 0.0, a); }
// np.dot(sigma, cfv_all) (:79) as k_mccfr_replay writes it
template <int N>
__device__ __forceinline__ double dot(const double *sigma, const double *cfv) {
    double v = 0.0;
#pragma unroll
    for (int i = 0; i < N; i++) v = fma(sigma[i], cfv[i], v);
    return v;
}

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

// ---- the walk --------------------------------------------------------------------------------------------------------------------------------
constexpr int kWalkThreads = 256;
struct WalkLds {
    double reach[kStageRecs], samp[kStageRecs];   // opponent reach and traverser sampling probability of a traverser instance, as running products
    double delta[kShallowRows * 5];               // the workgroup's increments into rows of depths 0..4
    uint32_t node[kStageRecs];                    // its node within its level | sampled action << 30
    int8_t val[kStageRecs + 5], leaf[kArrivals];  // return values, reward x2
};
static_assert(sizeof(WalkLds) == 53600, "LDS per workgroup");   // three would fit a compute unit; the kernel's 180 VGPRs allow two (a wavefront of each per SIMD)

struct Walk {
    const double *R;
    uint8_t *seen;
    unsigned long long *lv;
    const int8_t *r2;
    double *delta;
    uint32_t trav_id, iteration, seed_lo, seed_hi;
};

// one decision visit: the row's frozen sigma and the action its draw picks.  Philox counter (instance index in the traversal's recursion, global
// traversal id, iteration, 64 + traverser) under the context's seed; u = u53(x0, x1)
template <int D, int TRAV>
__device__ __forceinline__ int visit(const Walk &w, int node, int inst, double *sigma) {
    constexpr int n = t_branch(D);
    const size_t row = (size_t)t_offset(D) + node;
    w.seen[row] = 1;
    const Row4 R = load_row(w.R + row * 4);
    scopa::mc_sigma(R.x, n, sigma);
    const scopa::philox_out x = scopa::philox4x32_10((uint32_t)(i_offset<TRAV>(D) + inst), w.trav_id, w.iteration, kPhiloxTag + TRAV, w.seed_lo, w.seed_hi);
    return choice<n>(sigma, scopa::u53(x.x0, x.x1));
}

// the other team's plies from depth D down to the traverser's next ply or depth 12: single children, the instance index carries over
template <int D, int TRAV>
__device__ __forceinline__ void descend(const Walk &w, int &node, int inst, double &reach) {
    if constexpr (D < 12 && t_team(D) != TRAV) {
        double sigma[4];
        const int a = visit<D, TRAV>(w, node, inst, sigma);
        reach = reach * pick<t_branch(D)>(sigma, a);
        node = node * t_branch(D) + a;
        descend<D + 1, TRAV>(w, node, inst, reach);
    }
}

template <int K, int TRAV>
__device__ __forceinline__ void make_record(const Walk &w, WalkLds &s, int node, int inst, double reach, double samp) {
    double sigma[4];
    const int a = visit<s_depth<TRAV>(K), TRAV>(w, node, inst, sigma);
    s.node[s_first(K) + inst] = (uint32_t)node | ((uint32_t)a << 30);
    s.reach[s_first(K) + inst] = reach;
    s.samp[s_first(K) + inst] = samp;
}

// the b + 1 child instances of every traverser instance of ply K: down to the next traverser ply's record, or to the depth-12 node
template <int K, int TRAV>
__device__ __forceinline__ void expand(const Walk &w, WalkLds &s, int tid) {
    constexpr int D = s_depth<TRAV>(K), b = s_cards(K);
    for (int j = tid; j < s_count(K + 1); j += kWalkThreads) {
        const int i = j / (b + 1), slot = j - i * (b + 1);
        const uint32_t rec = s.node[s_first(K) + i];
        const int pnode = (int)(rec & 0x3FFFFFFFu), c = slot == 0 ? (int)(rec >> 30) : slot - 1;
        const Row4 R = load_row(w.R + ((size_t)t_offset(D) + pnode) * 4);
        double sigma[4];
        scopa::mc_sigma(R.x, b, sigma);
        double reach = s.reach[s_first(K) + i];
        const double samp = s.samp[s_first(K) + i] * pick<b>(sigma, c);   // :62, :77
        int node = pnode * b + c;
        descend<D + 1, TRAV>(w, node, j, reach);
        if constexpr (K + 1 < kStages) {
            make_record<K + 1, TRAV>(w, s, node, j, reach, samp);
        } else {
            atomicAdd(w.lv + (size_t)TRAV * kTLeaves + node, 1ull);
            const int p0 = w.r2[node];
            s.leaf[j] = (int8_t)(TRAV == 0 ? p0 : -p0);
        }
    }
    __syncthreads();
}

// values up and the regret increments of ply K's instances (:79-83)
template <int K, int TRAV>
__device__ __forceinline__ void update(const Walk &w, WalkLds &s, int tid) {
    constexpr int D = s_depth<TRAV>(K), b = s_cards(K);
    const int8_t *below = K + 1 < kStages ? s.val + s_first(K + 1) : s.leaf;
    for (int i = tid; i < s_count(K); i += kWalkThreads) {
        const int node = (int)(s.node[s_first(K) + i] & 0x3FFFFFFFu);
        const int row = t_offset(D) + node;
        const Row4 R = load_row(w.R + (size_t)row * 4);
        double sigma[4], cfv[b];
        scopa::mc_sigma(R.x, b, sigma);
        s.val[s_first(K) + i] = below[i * (b + 1)];
#pragma unroll
        for (int c = 0; c < b; c++) cfv[c] = 0.5 * (double)below[i * (b + 1) + 1 + c];
        const double v = dot<b>(sigma, cfv);
        const double reach = s.reach[s_first(K) + i], samp = s.samp[s_first(K) + i];
        const double wt = samp > 0.0 ? reach / samp : 0.0;
#pragma unroll
        for (int c = 0; c < b; c++) {
            const double inc = wt * (cfv[c] - v);
            if (inc == 0.0) continue;   // adding 0.0 changes nothing: a loop child of probability 0 has weight 0 throughout its subtree
            if constexpr (D < 5) atomicAdd(s.delta + row * 5 + c, inc); else atomicAdd(w.delta + (size_t)row * 5 + c, inc);
        }
        if constexpr (D < 5) atomicAdd(s.delta + row * 5 + 4, 1.0); else atomicAdd(w.delta + (size_t)row * 5 + 4, 1.0);
    }
    __syncthreads();
}

template <int TRAV>
__device__ __forceinline__ void walk_one(const Walk &w, WalkLds &s, int tid) {
    if (tid == 0) {
        int node = 0;
        double reach = 1.0;
        descend<0, TRAV>(w, node, 0, reach);
        make_record<0, TRAV>(w, s, node, 0, reach, 1.0);
    }
    __syncthreads();
    expand<0, TRAV>(w, s, tid); expand<1, TRAV>(w, s, tid); expand<2, TRAV>(w, s, tid); expand<3, TRAV>(w, s, tid); expand<4, TRAV>(w, s, tid); expand<5, TRAV>(w, s, tid);
    update<5, TRAV>(w, s, tid); update<4, TRAV>(w, s, tid); update<3, TRAV>(w, s, tid); update<2, TRAV>(w, s, tid); update<1, TRAV>(w, s, tid); update<0, TRAV>(w, s, tid);
}

// tasks [0, 2 nb): task k is traverser k & 1 of global traversal b0 + (k >> 1); a workgroup takes tasks blockIdx.x, + gridDim.x, ...
__global__ void __launch_bounds__(kWalkThreads)
k_team_mccfr_walk(const double *__restrict__ g_R, uint8_t *g_seen, unsigned long long *g_lv, const int8_t *__restrict__ g_r2, double *g_delta, uint32_t iteration, uint32_t b0,
                  uint32_t nb, uint32_t seed_lo, uint32_t seed_hi) {
    __shared__ WalkLds s;
    const int tid = threadIdx.x;
    for (int k = tid; k < kShallowRows * 5; k += kWalkThreads) s.delta[k] = 0.0;
    __syncthreads();
    for (uint32_t task = blockIdx.x; task < 2u * nb; task += gridDim.x) {
        const Walk w{g_R, g_seen, g_lv, g_r2, g_delta, b0 + (task >> 1), iteration, seed_lo, seed_hi};
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
