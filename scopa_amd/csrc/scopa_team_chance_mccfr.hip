// scopa_team_chance_mccfr.hip -- external-sampling MCCFR on Team MiniScopa over a SET of deals with the deal sampled too: the sampling solver of
// scopa_team_mccfr.hip run on the rows the deals share by key (scopa_team_chance.hip).  On one deal the team game has perfect information and every
// history is its own infoset; here a team's rows are shared between the deals its acting seat cannot tell apart, and MCCFRTrainer(TPIMiniScopaGame)
// becomes a solver for a game of imperfect information.
//
// Within one deal the map from local row to global row is injective (a history fixes the node and so the key), so a traversal on one deal is the
// walk of scopa_team_mccfr_walk.h with every table address sent through the deal's map row: the MappedRows policy.  It keeps no seen marks and no
// leaf_visits, as the chance game keeps no leaf_reach_sum.
//
//   k_team_chance_mccfr_walk   grid W x m: workgroup (w, slot) serves ONE deal -- the slot's -- for the whole launch and takes that deal's tasks w, w + W,
//       ...; task k is traverser k & 1 of the traversal with global id first + (k >> 1), first = b0 + deal * stride (iterate: b0 = 0, stride = batch, so ids
//       follow the deal id and not its list position; traverse: the caller's b0, stride 0).  Its LDS accumulator of the 341 rows of depths 0..4 is indexed
//       by LOCAL row and flushed once at the end through the deal's map row; deeper rows go to the delta buffer [G][5] as float64 atomics at map[deal][row].
//       Rows are shared, so the arrival order of a row's increments spans workgroups of several deals: counts are exact, regrets reproducible to rounding.
//   k_team_chance_mccfr_apply  a lane per global row; a row with count > 0: R += delta[:4]; S += count * mc_sigma(R before the add); the row's sigma
//       by the regret matching the CFR reduce leaves (so scopa_team_chance_cfr_iterate may follow); delta <- 0.  A row with count 0 is not read
//       beyond its count and not written.  No discount.
#include <algorithm>
#include <vector>

#include "scopa_team_chance.h"
#include "scopa_team_mccfr_walk.h"
#include "scopa_tree_passes.h"

using scopa::fail;

namespace {

__global__ void __launch_bounds__(kWalkThreads)
k_team_chance_mccfr_walk(const double *__restrict__ g_R, const int32_t *__restrict__ g_map, const int8_t *__restrict__ g_r2, double *g_delta,
                         const int32_t *__restrict__ g_list /* [gridDim.y] deal ids, or NULL: slot + deal0 */, int deal0, uint32_t iteration, uint32_t b0, uint32_t stride,
                         uint32_t nb, uint32_t seed_lo, uint32_t seed_hi) {
    __shared__ WalkLds s;
    const int tid = threadIdx.x;
    const int deal = g_list ? g_list[blockIdx.y] : deal0 + (int)blockIdx.y;
    const int32_t *map = g_map + (size_t)deal * kTChoice;
    const uint32_t first = b0 + (uint32_t)deal * stride;
    for (int k = tid; k < kShallowRows * 5; k += kWalkThreads) s.delta[k] = 0.0;
    __syncthreads();
    for (uint32_t task = blockIdx.x; task < 2u * nb; task += gridDim.x) {
        const Walk<MappedRows> w{g_R, nullptr, nullptr, g_r2 + (size_t)deal * kTLeaves, g_delta, first + (task >> 1), iteration, seed_lo, seed_hi, MappedRows{map}};
        if ((task & 1u) == 0u) walk_one<0>(w, s, tid); else walk_one<1>(w, s, tid);
    }
    for (int k = tid; k < kShallowRows * 5; k += kWalkThreads) {
        const double d = s.delta[k];
        if (d != 0.0) atomicAdd(g_delta + (size_t)map[k / 5] * 5 + (k % 5), d);
    }
}

template <int B>
__device__ __forceinline__ void apply_row(long long g, double count, double *d, double *g_R, double *g_S, double *g_sig) {
    Row4 R = load_row(g_R + g * 4), S = load_row(g_S + g * 4), L = {{0.0, 0.0, 0.0, 0.0}};
    double sigma[4];
    scopa::mc_sigma(R.x, B, sigma);
#pragma unroll
    for (int c = 0; c < B; c++) {
        R.x[c] += d[c];
        S.x[c] += count * sigma[c];
    }
    scopa::regret_match<B>(R.x, L.x);
    store_row(g_R + g * 4, R);
    store_row(g_S + g * 4, S);
    store_row(g_sig + g * 4, L);
}

__global__ void __launch_bounds__(256)
k_team_chance_mccfr_apply(const uint64_t *__restrict__ g_key, double *g_R, double *g_S, double *g_sig, double *g_delta, long long G) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    double *d = g_delta + g * 5;
    const double count = d[4];
    if (count == 0.0) return;
    const int b = t_branch(key_depth(g_key[g]));
    if (b == 4) apply_row<4>(g, count, d, g_R, g_S, g_sig);
    else if (b == 3) apply_row<3>(g, count, d, g_R, g_S, g_sig);
    else apply_row<2>(g, count, d, g_R, g_S, g_sig);
#pragma unroll
    for (int c = 0; c < 5; c++) d[c] = 0.0;
}

// the delta buffer, at the first MCCFR call on the handle
int32_t ensure_state(scopa_team_chance *g, const char *no_memory) {
    scopa_ctx *ctx = g->ctx;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    if (g->d_mc_delta) return SCOPA_OK;
    const size_t bytes = (size_t)g->G * 40;
    if (hipMalloc(&g->d_mc_delta, bytes) != hipSuccess) { g->d_mc_delta = nullptr; return fail(ctx, SCOPA_ENOMEM, no_memory); }
    SC_HIP(ctx, hipMemsetAsync(g->d_mc_delta, 0, bytes, ctx->stream));
    return SCOPA_OK;
}

// every list of a call holds m distinct ids in [0, n)
bool lists_ok(int n, int32_t n_lists, int32_t m, const int32_t *h_deals) {
    std::vector<int32_t> seen((size_t)n, -1);
    for (int32_t it = 0; it < n_lists; it++)
        for (int32_t k = 0; k < m; k++) {
            const int32_t d = h_deals[(size_t)it * m + k];
            if (d < 0 || d >= n || seen[(size_t)d] == it) return false;
            seen[(size_t)d] = it;
        }
    return true;
}

// the deal lists of a call, once, into g->d_mc_list (grown as needed); synchronises the stream: the caller's rows are only borrowed.  Lists the
// buffer already holds are left there
int32_t upload_lists(scopa_team_chance *g, size_t n_ids, const int32_t *h_deals, const char *no_memory) {
    scopa_ctx *ctx = g->ctx;
    if (g->h_mc_list.size() == n_ids && std::equal(h_deals, h_deals + n_ids, g->h_mc_list.begin())) return SCOPA_OK;
    g->h_mc_list.clear();
    if (n_ids > g->mc_list_cap) {
        SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (g->d_mc_list) { (void)hipFree(g->d_mc_list); g->d_mc_list = nullptr; g->mc_list_cap = 0; }
        if (hipMalloc(&g->d_mc_list, n_ids * 4) != hipSuccess) { g->d_mc_list = nullptr; return fail(ctx, SCOPA_ENOMEM, no_memory); }
        g->mc_list_cap = n_ids;
    }
    SC_HIP(ctx, hipMemcpyAsync(g->d_mc_list, h_deals, n_ids * 4, hipMemcpyHostToDevice, ctx->stream));
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    g->h_mc_list.assign(h_deals, h_deals + n_ids);
    return SCOPA_OK;
}

// one walk launch over m deals (d_list, or deal0 .. deal0 + m - 1), nb traversal pairs each.  A workgroup keeps its deal and its LDS accumulator for the
// whole launch: W workgroups per deal, the grid at about two resident workgroups per compute unit (53 600 bytes of LDS and the walk's registers allow two)
int32_t walk_launch(scopa_team_chance *g, const int32_t *d_list, int deal0, int m, uint32_t iteration, uint32_t b0, uint32_t stride, uint32_t nb) {
    scopa_ctx *ctx = g->ctx;
    const uint32_t tasks = 2u * nb, resident = 2u * (uint32_t)ctx->n_cus;
    uint32_t W = resident / (uint32_t)m;
    W = W < 1u ? 1u : W;
    W = W > tasks ? tasks : W;
    hipLaunchKernelGGL(k_team_chance_mccfr_walk, dim3(W, (unsigned)m), dim3(kWalkThreads), 0, ctx->stream, (const double *)g->d_R, (const int32_t *)g->d_map, (const int8_t *)g->d_r2,
                       g->d_mc_delta, d_list, deal0, iteration, b0, stride, nb, (uint32_t)ctx->seed, (uint32_t)(ctx->seed >> 32));
    SC_HIP(ctx, hipGetLastError());
    g->mccfr_decision += (unsigned long long)m * nb * (kDraws0 + kDraws1);
    g->mccfr_terminal += (unsigned long long)m * nb * 2ull * kTerminals;
    return SCOPA_OK;
}

int32_t apply_launch(scopa_team_chance *g) {
    scopa_ctx *ctx = g->ctx;
    hipLaunchKernelGGL(k_team_chance_mccfr_apply, dim3((unsigned)((g->G + 255) / 256)), dim3(256), 0, ctx->stream, (const uint64_t *)g->d_gkey, g->d_R, g->d_S, g->d_sig, g->d_mc_delta,
                       g->G);
    SC_HIP(ctx, hipGetLastError());
    g->mccfr_iteration++;
    return SCOPA_OK;
}

bool batch_ok(const scopa_team_chance *g, uint32_t batch) { return batch != 0 && batch <= (1u << 24) && (unsigned long long)g->n * batch <= (1ull << 32); }

}  // namespace

extern "C" {

int32_t scopa_team_chance_mccfr_traverse(scopa_team_chance *g, uint32_t iteration, int32_t deal, uint32_t b0, uint32_t nb) {
    if (!g || nb > (1u << 24) || b0 > 0xFFFFFFFFu - nb || deal < 0 || deal >= g->n) return SCOPA_EINVAL;
    const int32_t rc = ensure_state(g, "scopa_team_chance_mccfr_traverse: no device memory for the delta buffer");
    if (rc != SCOPA_OK || nb == 0) return rc;
    return walk_launch(g, nullptr, deal, 1, iteration, b0, 0u, nb);
}

int32_t scopa_team_chance_mccfr_apply(scopa_team_chance *g) {
    if (!g) return SCOPA_EINVAL;
    const int32_t rc = ensure_state(g, "scopa_team_chance_mccfr_apply: no device memory for the delta buffer");
    if (rc != SCOPA_OK) return rc;
    return apply_launch(g);
}

int32_t scopa_team_chance_mccfr_walk(scopa_team_chance *g, uint32_t iteration, uint32_t batch, int32_t m, const int32_t *h_deals) {
    if (!g || !batch_ok(g, batch)) return SCOPA_EINVAL;
    if (h_deals && (m < 1 || m > g->n || !lists_ok(g->n, 1, m, h_deals))) return SCOPA_EINVAL;
    if (int32_t rc = ensure_state(g, "scopa_team_chance_mccfr_walk: no device memory for the delta buffer")) return rc;
    if (h_deals) { if (int32_t rc = upload_lists(g, (size_t)m, h_deals, "scopa_team_chance_mccfr_walk: no device memory for the list")) return rc; }
    return walk_launch(g, h_deals ? g->d_mc_list : nullptr, 0, h_deals ? m : g->n, iteration, 0u, batch, batch);
}

int32_t scopa_team_chance_mccfr_iterate(scopa_team_chance *g, int32_t n_iters, uint32_t batch, int32_t m, const int32_t *h_deals) {
    if (!g || n_iters < 0 || n_iters > (1 << 20) || !batch_ok(g, batch)) return SCOPA_EINVAL;
    if (h_deals && (m < 1 || m > g->n || !lists_ok(g->n, n_iters, m, h_deals))) return SCOPA_EINVAL;
    if (n_iters == 0) return SCOPA_OK;
    if (int32_t rc = ensure_state(g, "scopa_team_chance_mccfr_iterate: no device memory for the delta buffer")) return rc;
    if (h_deals) { if (int32_t rc = upload_lists(g, (size_t)n_iters * (size_t)m, h_deals, "scopa_team_chance_mccfr_iterate: no device memory for the lists")) return rc; }   // once
    const int slots = h_deals ? m : g->n;
    for (int32_t it = 0; it < n_iters; it++) {   // one walk launch and the apply per iteration on the context's stream, no host synchronisation in between
        if (int32_t rc = walk_launch(g, h_deals ? g->d_mc_list + (size_t)it * m : nullptr, 0, slots, g->mccfr_iteration, 0u, batch, batch)) return rc;
        if (int32_t rc = apply_launch(g)) return rc;
    }
    return SCOPA_OK;
}

int32_t scopa_team_chance_mccfr_counters(scopa_team_chance *g, uint64_t *decision_visits, uint64_t *terminal_visits, uint32_t *iterations) {
    if (!g) return SCOPA_EINVAL;
    if (decision_visits) *decision_visits = g->mccfr_decision;
    if (terminal_visits) *terminal_visits = g->mccfr_terminal;
    if (iterations) *iterations = g->mccfr_iteration;
    return SCOPA_OK;
}

int32_t scopa_team_chance_mccfr_delta_get(scopa_team_chance *g, double *h_delta) {
    if (!g || !h_delta) return SCOPA_EINVAL;
    scopa_ctx *ctx = g->ctx;
    const int32_t rc = ensure_state(g, "scopa_team_chance_mccfr_delta_get: no device memory for the delta buffer");
    if (rc != SCOPA_OK) return rc;
    SC_HIP(ctx, hipMemcpyAsync(h_delta, g->d_mc_delta, (size_t)g->G * 40, hipMemcpyDeviceToHost, ctx->stream));
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SCOPA_OK;
}

}  // extern "C"
