// scopa_sdcfr_avg.hip -- the SDCFR average policy as a tabular policy: StrategyBuffer.get_average_policy (deep_cfr.py:137-160) at every
// decision node of the deal, one [n_infosets][4] table in hand order (the format scopa_exploitability and the tabular evaluation take).
//
// The reference's average policy is a per-state mix: for each stored snapshot s (FIFO order) policy += positive_regret_policy(net_s(x), mask)
// * (weight_s / total), float32 (nets.py:93-101).  The SDCFR features depend on the mover's hand and the table alone (deep_cfr.py:213-275), so
// the mix is a function of the infoset and the deal's tree holds all of it: the player's 737 / 916 decision nodes x S snapshots.
//   pass 1 (k_sdcfr_avg_terms):  per (16-node tile, snapshot) the 34-128-64-16 MLP on the matrix cores (v_mfma_f32_16x16x4_f32, the tile
//           k_sdcfr_policy runs: sd_tile_policy, scopa_sdcfr_tile.h), regret matching, times coef_s -> terms[s][node] (float4, hand order)
//   pass 2 (k_sdcfr_avg_reduce): one lane per node: the terms summed over s in FIFO order (float32, the reference's `policy +=`), normalised
//           over the legal slots in float64, uniform where the sum is 0 or not finite (evaluate_vs_random, deep_cfr.py:391-397), written to
//           the node's infoset row.
// No atomics: every (node, snapshot) term has one writer and every sum one order, so the table is the same bits for any grid.
#include "scopa_ctx.h"
#include "scopa_sdcfr_tile.h"

using namespace scopa;

namespace {
// a player's decision nodes, ply by ply (plies player, player + 2, ...): 1 + 16 + 144 + 576 = 737 (player 0), 4 + 48 + 288 + 576 = 916 (player 1)
__host__ __device__ constexpr int av_nodes(int player) { return player ? 916 : 737; }
__host__ __device__ constexpr int av_tiles(int player) { return player ? 1 + 3 + 18 + 36 : 1 + 1 + 9 + 36; }
constexpr int kAvMaxNodes = 916;
constexpr int kAvWaves = 4;   // one tile at a time per workgroup, its layers split over four wavefronts as in k_sdcfr_policy

// tile t of the player -> its ply d, the index of its first node within the ply, and the player-list index of the ply's first node
__device__ __forceinline__ void av_tile(int player, int t, int &d, int &j0, int &base) {
    int m = 0;
    base = 0;
    for (; m < 3; m++) {
        const int w = level_width(player + 2 * m), tc = (w + 15) >> 4;
        if (t < tc) break;
        t -= tc;
        base += w;
    }
    d = player + 2 * m;
    j0 = 16 * t;
}
}  // namespace

// Pass 1.  Workgroup b handles snapshot b / groups and tiles [g * tiles_per_wg, ...) of the player, g = b % groups.  The snapshot's weights are read
// straight from the StrategyBuffer store (row-major W[out][in]) into registers once per workgroup (sd_load_slices_torch) and serve all its tiles,
// each of which is sd_tile_policy, the tile of k_sdcfr_policy (scopa_sdcfr_tile.h).
// The pass as a device function over n_tiles tiles of a list of n_nodes entries: node_of(tile, column, xbits, hand, nl, index) names the entry a lane
// computes -- its feature bits, hand nibbles and legal count -- and returns whether it is live; its term goes to terms[s][index].  k_sdcfr_avg_terms lists the
// player's decision nodes of one deal, k_chance_sdcfr_avg_terms the player's distinct keys of a set of deals by their representative nodes.
template <class NodeOf>
__device__ __forceinline__ void
av_terms(int n_nodes, int n_tiles, int groups, int tiles_per_wg,
         const float *__restrict__ w1, const float *__restrict__ b1, const float *__restrict__ w2, const float *__restrict__ b2,
         const float *__restrict__ w3, const float *__restrict__ b3, int max_size, const int32_t *__restrict__ slots,
         const float *__restrict__ coef, float4 *__restrict__ terms, NodeOf node_of) {
    __shared__ SdTileLds lds;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nj = lane & 15, q = lane >> 4;
    const int s = (int)blockIdx.x / groups, g = (int)blockIdx.x % groups;
    int slot = slots[s];
    float cs = coef[s];
    if ((unsigned)slot >= (unsigned)max_size) { slot = 0; cs = __builtin_nanf(""); }   // nothing is read outside the store: the node rows go uniform
    SdSlices W;
    sd_load_slices_torch(w1 + (size_t)slot * 128 * 34, b1 + (size_t)slot * 128, w2 + (size_t)slot * 64 * 128, b2 + (size_t)slot * 64,
                         w3 + (size_t)slot * 16 * 64, b3 + (size_t)slot * 16, wave, lane, W);
    const int t_end = (g + 1) * tiles_per_wg < n_tiles ? (g + 1) * tiles_per_wg : n_tiles;
    for (int t = g * tiles_per_wg; t < t_end; t++) {
        uint32_t xbits, hand;
        int nl, index;
        const bool live = node_of(t, nj, xbits, hand, nl, index);
        float pk = 0.0f;
        if (!sd_tile_policy(W, lds, xbits, hand, nl, wave, lane, pk)) continue;
        if (live) reinterpret_cast<float *>(terms + (size_t)s * n_nodes + index)[q] = pk * cs;   // strategy_policy * (weight / total)
    }
}

// feature bits (hand one-hot | table multi-hot << 16) and hand nibbles of `player` at one of its decision nodes
__device__ __forceinline__ void av_node_bits(const scopa_state &st, int player, uint32_t &xbits, uint32_t &hand) {
    uint32_t hand_bits = 0, table_bits = 0;
    for (int k = 0; k < st.nh[player]; k++) hand_bits |= 1u << nib(st.hand[player], k);
    for (int k = 0; k < st.nt; k++) table_bits |= 1u << nib(st.table, k);
    xbits = hand_bits | (table_bits << 16);
    hand = st.hand[player];
}

__global__ void __launch_bounds__(kAvWaves * 64)
k_sdcfr_avg_terms(const scopa_state *__restrict__ g_states, int player, int groups, int tiles_per_wg,
                  const float *__restrict__ w1, const float *__restrict__ b1, const float *__restrict__ w2, const float *__restrict__ b2,
                  const float *__restrict__ w3, const float *__restrict__ b3, int max_size, const int32_t *__restrict__ slots,
                  const float *__restrict__ coef, float4 *__restrict__ terms) {
    av_terms(av_nodes(player), av_tiles(player), groups, tiles_per_wg, w1, b1, w2, b2, w3, b3, max_size, slots, coef, terms,
             [=](int t, int nj, uint32_t &xbits, uint32_t &hand, int &nl, int &index) {
                 int d, j0, base;
                 av_tile(player, t, d, j0, base);
                 const int wd = level_width(d), j = j0 + nj;   // this lane's node: j-th of its ply, base + j-th of the player's
                 const bool live = j < wd;
                 av_node_bits(g_states[level_offset(d) + (live ? j : wd - 1)], player, xbits, hand);   // lanes beyond the ply compute a copy of its last node and store nothing
                 nl = nlegal_at(d);
                 index = base + j;
                 return live;
             });
}

// The same pass over the distinct keys of `player` in a set of deals: entry c of rep[n_keys] = {feature bits, hand nibbles, global id, legal count} of the key's
// representative node (k_chance_sdcfr_reps), sixteen keys per tile.  A column's result depends on its own operands alone, so a key's term carries the bits
// k_sdcfr_avg_terms gives every node of that key in any deal.
__global__ void __launch_bounds__(kAvWaves * 64)
k_chance_sdcfr_avg_terms(const uint4 *__restrict__ rep, int n_keys, int groups, int tiles_per_wg,
                         const float *__restrict__ w1, const float *__restrict__ b1, const float *__restrict__ w2, const float *__restrict__ b2,
                         const float *__restrict__ w3, const float *__restrict__ b3, int max_size, const int32_t *__restrict__ slots,
                         const float *__restrict__ coef, float4 *__restrict__ terms) {
    av_terms(n_keys, (n_keys + 15) >> 4, groups, tiles_per_wg, w1, b1, w2, b2, w3, b3, max_size, slots, coef, terms,
             [=](int t, int nj, uint32_t &xbits, uint32_t &hand, int &nl, int &index) {
                 const int c = 16 * t + nj;
                 const bool live = c < n_keys;
                 const uint4 r = rep[live ? c : n_keys - 1];
                 xbits = r.x; hand = r.y; nl = (int)r.w;
                 index = c;
                 return live;
             });
}

// The representative node of every distinct key: the first node (BFS order within the key's ply) of the key's first occurrence in CSR order, i.e. in its lowest
// deal.  One lane per global row; rank[g] = the row's index among its player's keys, ascending global id.  Once per handle.
__global__ void __launch_bounds__(256)
k_chance_sdcfr_reps(const uint64_t *__restrict__ gkey, const int32_t *__restrict__ occ_off, const int32_t *__restrict__ occ, const uint16_t *__restrict__ g_infoset /*[n][1653]*/,
                    const scopa_state *__restrict__ g_states /*[n][2229]*/, const int32_t *__restrict__ rank, uint4 *__restrict__ rep0, uint4 *__restrict__ rep1, long long G) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    const uint64_t key = gkey[g];
    const int player = (int)(key & 1), nl = (int)((key >> 1) & 7), d = 2 * (4 - nl) + player;   // a key fixes the player and the legal count, hence the ply
    const int o = occ[occ_off[g]], deal = o / kDecision, local = o - deal * kDecision;
    const uint16_t *inf = g_infoset + (size_t)deal * kDecision + level_offset(d);
    int j = 0;
    while (j < level_width(d) - 1 && (int)inf[j] != local) j++;
    uint32_t xbits, hand;
    av_node_bits(g_states[(size_t)deal * kNodes + level_offset(d) + j], player, xbits, hand);
    (player ? rep1 : rep0)[rank[g]] = make_uint4(xbits, hand, (uint32_t)g, (uint32_t)nl);
}

// entry i of a list of n_nodes: its terms summed over the snapshots in FIFO order (float32, the reference's `policy +=`), normalised over the nl legal
// slots in float64, uniform where that sum is 0 or not finite, zeros beyond; into row[4]
__device__ __forceinline__ void av_reduce_row(const float4 *__restrict__ terms, int n_nodes, int i, int n_snap, int nl, double *__restrict__ row) {
    float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    int s = 0;
    for (; s + 16 <= n_snap; s += 16) {   // sixteen loads in flight, the adds in FIFO order
        float4 t[16];
#pragma unroll
        for (int u = 0; u < 16; u++) t[u] = terms[(size_t)(s + u) * n_nodes + i];
#pragma unroll
        for (int u = 0; u < 16; u++) { a[0] += t[u].x; a[1] += t[u].y; a[2] += t[u].z; a[3] += t[u].w; }
    }
    for (; s < n_snap; s++) {
        const float4 t = terms[(size_t)s * n_nodes + i];
        a[0] += t.x; a[1] += t.y; a[2] += t.z; a[3] += t.w;
    }
    double sum = 0.0;
    for (int k = 0; k < nl; k++) sum += (double)a[k];
    const bool uniform = !(sum > 0.0) || isinf(sum);   // 0, NaN, inf: the uniform choice evaluate_vs_random falls back to
    for (int k = 0; k < 4; k++) row[k] = k < nl ? (uniform ? 1.0 / (double)nl : (double)a[k] / sum) : 0.0;
}

// Pass 2.  Nodes of one infoset write the same row with the same bits: an infoset is P{p}:H[hand]_T[table] with hand and table in order
// (openspiel_mini_scopa.py:48-60), so its nodes have the same feature bits and hand nibbles; pass 1 computes a node's terms from those and the
// snapshot alone (an MFMA result column depends on its own operand column only) and this pass sums them in one fixed order.
__global__ void __launch_bounds__(256)
k_sdcfr_avg_reduce(const uint16_t *__restrict__ g_infoset, const float4 *__restrict__ terms, int player, int n_snap, double *__restrict__ policy) {
    const int n_nodes = av_nodes(player);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes) return;
    int m = 0, j = i;
    for (; m < 3 && j >= level_width(player + 2 * m); m++) j -= level_width(player + 2 * m);
    const int d = player + 2 * m, nl = nlegal_at(d);
    av_reduce_row(terms, n_nodes, i, n_snap, nl, policy + (size_t)g_infoset[level_offset(d) + j] * 4);
}

// one lane per global row of `player`'s keys: the same sum and row for entry c of the key list, written to the key's global row
__global__ void __launch_bounds__(256)
k_chance_sdcfr_avg_reduce(const uint4 *__restrict__ rep, int n_keys, const float4 *__restrict__ terms, int n_snap, double *__restrict__ policy_G) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_keys) return;
    const uint4 r = rep[c];
    av_reduce_row(terms, n_keys, c, n_snap, (int)r.w, policy_G + (size_t)r.z * 4);
}

extern "C" int32_t scopa_sdcfr_average_policy(scopa_ctx *ctx, int32_t player, int32_t n_snap, const float *d_w1, const float *d_b1,
                                              const float *d_w2, const float *d_b2, const float *d_w3, const float *d_b3, int32_t max_size,
                                              const int32_t *d_slots, const float *d_coef, double *d_policy) {
    if (!ctx || player < 0 || player > 1 || n_snap < 0 || max_size < 0 || n_snap > max_size || !d_policy) return SCOPA_EINVAL;
    if (n_snap > 0 && (!d_w1 || !d_b1 || !d_w2 || !d_b2 || !d_w3 || !d_b3 || !d_slots || !d_coef)) return SCOPA_EINVAL;
    SC_REQUIRE(ctx, ctx->has_deal, SCOPA_ESTATE, "scopa_sdcfr_average_policy: no deal set");
    if (n_snap > 0) {
        const uintptr_t any = (uintptr_t)d_b1 | (uintptr_t)d_w2 | (uintptr_t)d_b2 | (uintptr_t)d_w3 | (uintptr_t)d_b3;
        SC_REQUIRE(ctx, (any & 15) == 0, SCOPA_EINVAL, "scopa_sdcfr_average_policy: b1, w2, b2, w3, b3 are read 16 bytes at a time and must be 16-byte aligned");
    }
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t bytes = (size_t)n_snap * kAvMaxNodes * sizeof(float4);
    if (bytes > ctx->sdavg_bytes) {
        SC_HIP(ctx, hipStreamSynchronize(ctx->stream));   // an earlier call's launches may still read the old buffer
        if (ctx->d_sdavg) SC_HIP(ctx, hipFree(ctx->d_sdavg));
        ctx->d_sdavg = nullptr;
        ctx->sdavg_bytes = 0;
        SC_HIP(ctx, hipMalloc(&ctx->d_sdavg, bytes));
        ctx->sdavg_bytes = bytes;
    }
    float4 *terms = (float4 *)ctx->d_sdavg;
    if (n_snap > 0) {
        // about four workgroups per compute unit, the rest of the work as more tiles per workgroup (each loads its snapshot's weights once);
        // measured at S = 100, both players: targets of two, four, eight and sixty-four (one tile per workgroup) took 123, 109, 113 and 132 us
        const int n_tiles = av_tiles(player);
        int groups = (4 * ctx->n_cus + n_snap - 1) / n_snap;
        groups = groups < 1 ? 1 : groups > n_tiles ? n_tiles : groups;
        const int tiles_per_wg = (n_tiles + groups - 1) / groups;
        groups = (n_tiles + tiles_per_wg - 1) / tiles_per_wg;
        hipLaunchKernelGGL(k_sdcfr_avg_terms, dim3((unsigned)(n_snap * groups)), dim3(kAvWaves * 64), 0, ctx->stream, ctx->d_states, (int)player, groups,
                           tiles_per_wg, d_w1, d_b1, d_w2, d_b2, d_w3, d_b3, (int)max_size, d_slots, d_coef, terms);
        SC_HIP(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(k_sdcfr_avg_reduce, dim3((av_nodes(player) + 255) / 256), dim3(256), 0, ctx->stream, ctx->d_infoset, (const float4 *)terms,
                       (int)player, (int)n_snap, d_policy);
    SC_HIP(ctx, hipGetLastError());
    return SCOPA_OK;
}

// ---- the chance game's average policy over keys (scopa_chance.hip owns the handle, its buffers and the argument checks) -----------------------------
namespace scopa {

int32_t launch_chance_sdcfr_reps(scopa_ctx *ctx, long long G, const uint64_t *d_gkey, const int32_t *d_occ_off, const int32_t *d_occ, const uint16_t *d_infoset,
                                 const scopa_state *d_states, const int32_t *d_rank, void *d_rep0, void *d_rep1) {
    hipLaunchKernelGGL(k_chance_sdcfr_reps, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, ctx->stream, d_gkey, d_occ_off, d_occ, d_infoset, d_states, d_rank,
                       (uint4 *)d_rep0, (uint4 *)d_rep1, G);
    SC_HIP(ctx, hipGetLastError());
    return SCOPA_OK;
}

int32_t launch_chance_sdcfr_avg(scopa_ctx *ctx, int n_keys, const void *d_rep, int n_snap, const float *d_w1, const float *d_b1, const float *d_w2,
                                const float *d_b2, const float *d_w3, const float *d_b3, int max_size, const int32_t *d_slots, const float *d_coef, void *d_terms,
                                double *d_policy_G) {
    if (n_keys <= 0) return SCOPA_OK;
    if (n_snap > 0) {   // scopa_sdcfr_average_policy's grid rule over the key tiles
        const int n_tiles = (n_keys + 15) >> 4;
        int groups = (4 * ctx->n_cus + n_snap - 1) / n_snap;
        groups = groups < 1 ? 1 : groups > n_tiles ? n_tiles : groups;
        const int tiles_per_wg = (n_tiles + groups - 1) / groups;
        groups = (n_tiles + tiles_per_wg - 1) / tiles_per_wg;
        hipLaunchKernelGGL(k_chance_sdcfr_avg_terms, dim3((unsigned)(n_snap * groups)), dim3(kAvWaves * 64), 0, ctx->stream, (const uint4 *)d_rep, n_keys, groups,
                           tiles_per_wg, d_w1, d_b1, d_w2, d_b2, d_w3, d_b3, max_size, d_slots, d_coef, (float4 *)d_terms);
        SC_HIP(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(k_chance_sdcfr_avg_reduce, dim3((unsigned)((n_keys + 255) / 256)), dim3(256), 0, ctx->stream, (const uint4 *)d_rep, n_keys,
                       (const float4 *)d_terms, n_snap, d_policy_G);
    SC_HIP(ctx, hipGetLastError());
    return SCOPA_OK;
}

}  // namespace scopa
