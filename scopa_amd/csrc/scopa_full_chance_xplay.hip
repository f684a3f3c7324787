// scopa_full_chance_xplay.hip -- FullScopa over a set of decks, store against store: the exact cross-play matrix of K stores on the sub-games below a
// root across a set of decks (scopa_full_chance_cross_play) and the sampled seat-swapped match of one store against another from a handle's root, the
// deal included (scopa_full_chance_pair_match); include/scopa.h states the procedures that define the bits.
//
// Cross-play is scopa_full_chance_eval.hip's forest and value pass for K x K ordered pairs of stores and four quantities at once.  No response, so no
// grouping by pair and no sort; the forest is expanded once and every store is read once.
//
//   forest    scopa_full_chance_forest.h's: roots root_on(root, deck d) (k_full_chance_xplay_roots), deck-major, child a of g at g n_k + a, slot a
//             the mover's a-th card in ascending card id.  States are kept for two levels only (the level being keyed and the one it expands into).
//   leaves    k_full_chance_xplay_expand packs a terminal state into 4 bytes: r2_p0 (int8), scopas[0], scopas[1].  They are widened to
//             r = r2_p0 / 2.0, r * r, (double)scopas[0], (double)scopas[1] in registers by the first step up.
//   policy    k_full_chance_xplay_policy, a lane per node: wide_key ONCE, then the read-only probe fw_find and full_eval_prob for each of the K
//             stores; the level's image is [store][slot][node].
//   value     k_full_chance_cross_play, one launch per level, a lane per (node, policy m of the level's mover): prob_m[node][.] is loaded once and
//             serves the K pairs (m, o) at player 0's levels, (o, m) at player 1's; per pair the four quantities are four accumulators in registers.
//             V of a level is [pair][quantity][node]: a wavefront's 64 nodes read 64 n_k consecutive doubles of every (pair, quantity) row.  The
//             lowest choice level (player 1 moves, the children are leaves) depends on player 1's policy alone, so it is computed and stored once
//             per b, [b][quantity][node], and the level above reads row b for every pair (a, b).  V is kept for two levels only.
//   means     k_full_chance_xplay_mean, a lane per (pair, quantity): (0.0 + V[root 0] + V[root 1] + ...) / n in deck order.
// No float64 atomic anywhere: the same handles, decks and order give the same bits.
//
// Scratch (one allocation, kept in hs[0], grown when a call needs more, freed by destroy), with n decks, K stores, T = 31 n (36^R - 1) / 35 stored
// nodes and E = n 36^R leaves:
//   24 K T + 52 E + the larger of 16 K E and (8 / 3) K^2 E + 8 K^2 E bytes + 40 n (every part rounded up to 256 bytes, 8 KiB more for the results):
//   prob 24 K T, states 64 (E / 2 + E / 4), packed leaves 4 E, V of the lowest level 32 K E / 2 sharing its buffer with the level two above it
//   (32 K^2 E / 12), V of the level between them 32 K^2 E / 4, and the decks.  2.9 GB where K = 16 and K E = 1 << 24.
#include <string.h>

#include <algorithm>
#include <new>

#include "scopa_ctx.h"
#include "scopa_full_chance_forest.h"
#include "scopa_full_chance_match.h"
#include "scopa_full_eval_passes.h"
#include "scopa_full_store_host.h"
#include "scopa_full_wide.h"

using namespace scopa_full;
using scopa::fail;

namespace {

constexpr int kMaxStores = 16;
constexpr uint64_t kMaxStoreLeaves = 1ull << 24;   // K x n x 36^R: bounds the K prob images
constexpr int32_t kMaxMatchDecks = 1 << 20;

struct XpStores {                                  // the K stores of a call, by value in the kernel's arguments
    const FwSlot *tab[kMaxStores];
    uint32_t mask[kMaxStores];
};

__global__ void __launch_bounds__(256)
k_full_chance_xplay_roots(const scopa_full_state root, const uint8_t *__restrict__ decks, uint32_t n, scopa_full_state *__restrict__ state) {
    const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= n) return;
    state[d] = root_on(root, decks + 40u * d);
}

__global__ void __launch_bounds__(256)
k_full_chance_xplay_expand(const scopa_full_state *__restrict__ parent, uint32_t n_child, uint32_t tree_child, int p, int n, int round_end,
                           const uint8_t *__restrict__ decks, scopa_full_state *__restrict__ child, uint32_t *__restrict__ leaf) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_child) return;
    const scopa_full_state s = full_chance_forest_child(parent, c, tree_child, p, n, round_end, decks);
    if (leaf) leaf[c] = (uint32_t)(uint8_t)s.r2_p0 | ((uint32_t)s.scopas[0] << 8) | ((uint32_t)s.scopas[1] << 16);
    else child[c] = s;
}

// prob [K][3][N] of a level: the key once, every store probed from it
__global__ void __launch_bounds__(256)
k_full_chance_xplay_policy(const scopa_full_state *__restrict__ st, uint32_t N, int p, int n, const XpStores S, int K, int which, double *__restrict__ prob) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const scopa_full_state s = st[i];
    const WideKey key = wide_key(s, p);
    for (int j = 0; j < K; j++) {
        const FwSlot *__restrict__ tab = S.tab[j];
        const int slot = fw_find(tab, S.mask[j], key.a, key.b);
        double pr[4];
        full_eval_prob(tab, slot, n, which, pr);
#pragma unroll
        for (int k = 0; k < 3; k++) prob[((size_t)j * 3 + (size_t)k) * N + i] = k < n ? pr[k] : 0.0;
    }
}

// the four quantities of a packed leaf
__device__ __forceinline__ void xp_widen(uint32_t w, double x[4]) {
    const double r = (double)(int8_t)(w & 0xFFu) / 2.0;
    x[0] = r;
    x[1] = r * r;
    x[2] = (double)((w >> 8) & 0xFFu);
    x[3] = (double)((w >> 16) & 0xFFu);
}

// One level of the value pass; blockIdx.y = m, the policy of the level's mover p.  V rows are [row][quantity][node].
//   kLeaf     the children are packed leaves: V[m] of the level, one row per m (the mover is player 1: m = b)
//   otherwise for every o < K the pair (m, o) at p = 0, (o, m) at p = 1; the child's row is the pair's, or row b where `child_by_b` (the children
//             are the lowest level)
template <bool kLeaf>
__global__ void __launch_bounds__(256)
k_full_chance_cross_play(const void *__restrict__ child, int child_by_b, const double *__restrict__ prob, uint32_t N, int n, int p, int K,
                         double *__restrict__ V) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const uint32_t m = blockIdx.y, c = i * (uint32_t)n;
    const size_t Nc = (size_t)N * (size_t)n;
    double pr[3];
#pragma unroll
    for (int a = 0; a < 3; a++) pr[a] = a < n ? prob[((size_t)m * 3 + (size_t)a) * N + i] : 0.0;
    if (kLeaf) {
        const uint32_t *__restrict__ leaf = (const uint32_t *)child;
        double v[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int a = 0; a < 3; a++)
            if (a < n) {
                double x[4];
                xp_widen(leaf[c + (uint32_t)a], x);
#pragma unroll
                for (int q = 0; q < 4; q++) v[q] += pr[a] * x[q];
            }
#pragma unroll
        for (int q = 0; q < 4; q++) V[((size_t)m * 4 + (size_t)q) * N + i] = v[q];
    } else {
        const double *__restrict__ Vc = (const double *)child;
        for (uint32_t o = 0; o < (uint32_t)K; o++) {
            const uint32_t a_ = p == 0 ? m : o, b_ = p == 0 ? o : m;
            const size_t pair = (size_t)a_ * (size_t)K + b_, crow = child_by_b ? (size_t)b_ : pair;
            double v[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const double *__restrict__ x = Vc + (crow * 4 + (size_t)q) * Nc + c;
#pragma unroll
                for (int a = 0; a < 3; a++)
                    if (a < n) v[q] += pr[a] * x[a];
            }
#pragma unroll
            for (int q = 0; q < 4; q++) V[(pair * 4 + (size_t)q) * N + i] = v[q];
        }
    }
}

// a lane per (pair, quantity): the mean of the n roots' values, added in deck order
__global__ void __launch_bounds__(256)
k_full_chance_xplay_mean(const double *__restrict__ V, uint32_t n, uint32_t rows, double *__restrict__ out) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    double v = 0.0;
    for (uint32_t d = 0; d < n; d++) v += V[(size_t)r * n + d];
    out[r] = v / (double)n;
}

// One lane per episode of the seat-swapped match from the root: the agent plays the average policy of its store, the opponent that of a second store
// (scopa_full_chance_match.h: the episode's one definition).
__global__ void __launch_bounds__(64)
k_full_chance_pair_match(const FwSlot *__restrict__ tab, uint32_t mask, const FwSlot *__restrict__ opp_tab, uint32_t opp_mask, const uint8_t *__restrict__ decks,
                         long long k_decks, const scopa_full_state root0, long long n, uint32_t stream_id, uint32_t seed_lo, uint32_t seed_hi,
                         long long *__restrict__ sums, int8_t *__restrict__ r2_agent) {
    full_chance_episode<true>(tab, mask, opp_tab, opp_mask, decks, k_decks, root0, n, stream_id, seed_lo, seed_hi, sums, r2_agent);
}

}  // namespace

namespace scopa_full {

struct FwXplay {
    char *d_buf = nullptr;
    size_t bytes = 0;
    scopa_full_state *d_state[2] = {nullptr, nullptr};    // levels of even / odd index
    uint32_t *d_leaf = nullptr;
    double *d_prob = nullptr;                             // level k at 3 K off[k]: [K][3][size[k]]
    double *d_V[2] = {nullptr, nullptr};                  // levels of odd / even distance from the lowest level: [0] holds the lowest
    double *d_out = nullptr;
    uint8_t *d_decks = nullptr;
};

void chance_xplay_free(FwXplay *x) {
    if (!x) return;
    if (x->d_buf) (void)hipFree(x->d_buf);
    delete x;
}

}  // namespace scopa_full

namespace {

// rows of V that level k of a forest of L levels holds: K at the lowest level, K x K above it
size_t v_rows(int k, int L, int K) { return k + 1 == L ? (size_t)K : (size_t)K * (size_t)K; }

int32_t ensure(scopa_full_chance *h, const Shape &s, uint32_t n, int K) {
    if (!h->xplay) {
        h->xplay = new (std::nothrow) FwXplay;
        if (!h->xplay) return fail(h->ctx, SCOPA_ENOMEM, "scopa_full_chance_cross_play: host record");
    }
    FwXplay *x = h->xplay;
    size_t st_n[2] = {0, 0}, v_b[2] = {0, 0};
    for (int k = 0; k < s.L; k++) {
        st_n[k & 1] = std::max(st_n[k & 1], (size_t)s.size[k]);
        const int side = (s.L - 1 - k) & 1;
        v_b[side] = std::max(v_b[side], 32 * v_rows(k, s.L, K) * (size_t)s.size[k]);
    }
    size_t at = 0;
    auto take = [&at](size_t b) { const size_t o = at; at += up256(b); return o; };
    const size_t o_s0 = take(64 * st_n[0]), o_s1 = take(64 * st_n[1]), o_leaf = take(4 * (size_t)s.size[s.L]), o_prob = take(24 * (size_t)K * s.off[s.L]),
                 o_v0 = take(v_b[0]), o_v1 = take(v_b[1]), o_out = take(8192), o_decks = take(40 * (size_t)n + 24);
    if (!x->d_buf || x->bytes < at) {
        SC_HIP(h->ctx, hipStreamSynchronize(h->ctx->stream));
        if (x->d_buf) { (void)hipFree(x->d_buf); x->d_buf = nullptr; x->bytes = 0; }
        char *buf = nullptr;
        const hipError_t err = hipMalloc((void **)&buf, at);
        if (err != hipSuccess) return fail(h->ctx, SCOPA_ENOMEM, "scopa_full_chance_cross_play: scratch of the forest", err);
        x->d_buf = buf; x->bytes = at;
    }
    char *buf = x->d_buf;
    x->d_state[0] = (scopa_full_state *)(buf + o_s0); x->d_state[1] = (scopa_full_state *)(buf + o_s1);
    x->d_leaf = (uint32_t *)(buf + o_leaf);
    x->d_prob = (double *)(buf + o_prob);
    x->d_V[0] = (double *)(buf + o_v0); x->d_V[1] = (double *)(buf + o_v1);
    x->d_out = (double *)(buf + o_out);
    x->d_decks = (uint8_t *)(buf + o_decks);
    return SCOPA_OK;
}

}  // namespace

extern "C" {

int32_t scopa_full_chance_cross_play(scopa_full_chance *const *hs, int32_t K, const scopa_full_state *root_state, const uint8_t *h_decks, int32_t k,
                                     int32_t which, double *h_out) {
    if (!hs || !h_out) return SCOPA_EINVAL;
    if (K < 1 || K > kMaxStores) return SCOPA_EINVAL;
    for (int32_t j = 0; j < K; j++)
        if (!hs[j]) return SCOPA_EINVAL;
    scopa_full_chance *h = hs[0];
    for (int32_t j = 1; j < K; j++)
        SC_REQUIRE(h->ctx, hs[j]->ctx == h->ctx, SCOPA_EINVAL, "scopa_full_chance_cross_play: the handles are of different contexts");
    SC_REQUIRE(h->ctx, which == 0 || which == 1, SCOPA_EINVAL, "scopa_full_chance_cross_play: which outside {0 (average policy), 1 (current sigma)}");
    const uint8_t *decks = h_decks ? h_decks : h->decks;
    if (!h_decks) k = h->n_decks;
    SC_REQUIRE(h->ctx, k >= 1, SCOPA_EINVAL, "scopa_full_chance_cross_play: k below 1");
    scopa_full_state root = root_state ? *root_state : h->root;
    SC_REQUIRE(h->ctx, root_ok(root), SCOPA_EINVAL, "scopa_full_chance_cross_play: the root must be a non-terminal state at a round boundary (step % 6 == 0)");
    root.game = 0u;
    const int R = 6 - (int)root.round;
    SC_REQUIRE(h->ctx, R <= kMaxRounds, SCOPA_ELIMIT, "scopa_full_chance_cross_play: more than 4 rounds from the root (36^R histories a deck are swept whole)");
    uint64_t leaves = (uint64_t)k;
    for (int r = 0; r < R; r++) leaves *= 36ull;                  // (k < 2^31, 36^4 < 2^21: no overflow)
    SC_REQUIRE(h->ctx, leaves <= kMaxLeaves, SCOPA_ELIMIT, "scopa_full_chance_cross_play: decks x 36^R above 1 << 22 (89 decks at R = 3, 2 at R = 4)");
    SC_REQUIRE(h->ctx, (uint64_t)K * leaves <= kMaxStoreLeaves, SCOPA_ELIMIT, "scopa_full_chance_cross_play: handles x decks x 36^R above 1 << 24");
    for (int32_t d = 0; d < k; d++)
        SC_REQUIRE(h->ctx, deck_fits(decks + 40 * (size_t)d, root), SCOPA_EINVAL,
                   "scopa_full_chance_cross_play: a deck does not pass create's check against the root of the call");
    SC_HIP(h->ctx, hipSetDevice(h->ctx->device));
    const uint32_t n = (uint32_t)k;
    const Shape s = shape_of(R, n);
    const int32_t rc = ensure(h, s, n, (int)K);
    if (rc != SCOPA_OK) return rc;
    FwXplay *x = h->xplay;
    hipStream_t st = h->ctx->stream;
    XpStores S;
    for (int j = 0; j < kMaxStores; j++) {
        const scopa_full_chance *hj = hs[j < K ? j : 0];
        S.tab[j] = hj->d_tab;
        S.mask[j] = (1u << hj->capacity_log2) - 1u;
    }
    const uint8_t *d_decks = h->d_decks;
    if (h_decks) {
        SC_HIP(h->ctx, hipMemcpyAsync(x->d_decks, h_decks, 40 * (size_t)n, hipMemcpyHostToDevice, st));
        d_decks = x->d_decks;
    }
    // 1, 2: the forest level by level, and every store's prob image of the level
    hipLaunchKernelGGL(k_full_chance_xplay_roots, grid_of(n), dim3(256), 0, st, root, d_decks, n, x->d_state[0]);
    EV_LAUNCHED(h->ctx, "k_full_chance_xplay_roots");
    for (int lv = 0; lv < s.L; lv++) {
        const int n_act = cards_of(lv), p = mover_of(lv);
        const bool leaf = lv + 1 == s.L;
        const uint32_t N = s.size[lv];
        const scopa_full_state *cur = x->d_state[lv & 1];
        hipLaunchKernelGGL(k_full_chance_xplay_policy, grid_of(N), dim3(256), 0, st, cur, N, p, n_act, S, (int)K, (int)which,
                           x->d_prob + 3 * (size_t)K * s.off[lv]);
        EV_LAUNCHED(h->ctx, "k_full_chance_xplay_policy");
        hipLaunchKernelGGL(k_full_chance_xplay_expand, grid_of(s.size[lv + 1]), dim3(256), 0, st, cur, s.size[lv + 1], s.size[lv + 1] / n, p, n_act,
                           (int)((lv & 3) == 3), d_decks, leaf ? (scopa_full_state *)nullptr : x->d_state[(lv + 1) & 1], leaf ? x->d_leaf : (uint32_t *)nullptr);
        EV_LAUNCHED(h->ctx, "k_full_chance_xplay_expand");
    }
    // 3: bottom up, every ordered pair and quantity in one launch per level
    for (int lv = s.L - 1; lv >= 0; lv--) {
        const int n_act = cards_of(lv), p = mover_of(lv), side = (s.L - 1 - lv) & 1;
        const uint32_t N = s.size[lv];
        const double *prob = x->d_prob + 3 * (size_t)K * s.off[lv];
        const dim3 grid((N + 255u) / 256u, (unsigned)K);
        if (lv + 1 == s.L)
            hipLaunchKernelGGL(k_full_chance_cross_play<true>, grid, dim3(256), 0, st, (const void *)x->d_leaf, 0, prob, N, n_act, p, (int)K, x->d_V[side]);
        else
            hipLaunchKernelGGL(k_full_chance_cross_play<false>, grid, dim3(256), 0, st, (const void *)x->d_V[side ^ 1], (int)(lv + 2 == s.L), prob, N, n_act, p, (int)K,
                               x->d_V[side]);
        EV_LAUNCHED(h->ctx, "k_full_chance_cross_play");
    }
    const uint32_t rows = 4u * (uint32_t)K * (uint32_t)K;
    hipLaunchKernelGGL(k_full_chance_xplay_mean, grid_of(rows), dim3(256), 0, st, (const double *)x->d_V[(s.L - 1) & 1], n, rows, x->d_out);
    EV_LAUNCHED(h->ctx, "k_full_chance_xplay_mean");
    double out[4 * kMaxStores * kMaxStores];
    SC_HIP(h->ctx, hipMemcpyAsync(out, x->d_out, 8 * (size_t)rows, hipMemcpyDeviceToHost, st));
    SC_HIP(h->ctx, hipStreamSynchronize(st));
    memcpy(h_out, out, 8 * (size_t)rows);                         // (h_out is written only by a call that completed)
    return SCOPA_OK;
}

int32_t scopa_full_chance_pair_match(scopa_full_chance *h, scopa_full_chance *h_b, int64_t n_episodes, uint32_t stream_id, const uint8_t *h_decks, int32_t k,
                                     int64_t h_sums[6], int8_t *h_r2_a) {
    if (!h || !h_b) return SCOPA_EINVAL;
    SC_REQUIRE(h->ctx, h_b->ctx == h->ctx, SCOPA_EINVAL, "scopa_full_chance_pair_match: the handles are of different contexts");
    SC_REQUIRE(h->ctx, n_episodes >= 0 && n_episodes <= (1ll << 36) && h_sums && stream_id < (1u << 24), SCOPA_EINVAL,      // (one launch: 2^30 workgroups of 64)
               "scopa_full_chance_pair_match: n_episodes outside [0, 1 << 36], stream_id at or above 1 << 24, or h_sums NULL");
    if (!h_decks) k = h->n_decks;
    SC_REQUIRE(h->ctx, k >= 1 && k <= kMaxMatchDecks, SCOPA_EINVAL, "scopa_full_chance_pair_match: k outside [1, 1 << 20]");
    if (h_decks)
        for (int32_t d = 0; d < k; d++)
            SC_REQUIRE(h->ctx, deck_fits(h_decks + 40 * (size_t)d, h->root), SCOPA_EINVAL, "scopa_full_chance_pair_match: a deck does not pass create's check against h_a's root");
    for (int i = 0; i < 6; i++) h_sums[i] = 0;
    if (!n_episodes) return SCOPA_OK;
    SC_REQUIRE(h->ctx, !h_r2_a || n_episodes <= (1ll << 31), SCOPA_EINVAL, "scopa_full_chance_pair_match: per-episode output asked for more than 1 << 31 episodes");
    SC_HIP(h->ctx, hipSetDevice(h->ctx->device));
    return run_match(h, "scopa_full_chance_pair_match", "k_full_chance_pair_match", n_episodes, h_decks, k, h_sums, h_r2_a, [&](const uint8_t *d_held, long long *d_sums, int8_t *d_r2) {
        hipLaunchKernelGGL(k_full_chance_pair_match, dim3((unsigned)((n_episodes + 63) / 64)), dim3(64), 0, h->ctx->stream, (const FwSlot *)h->d_tab,
                           (1u << h->capacity_log2) - 1u, (const FwSlot *)h_b->d_tab, (1u << h_b->capacity_log2) - 1u, (const uint8_t *)(d_held ? d_held : h->d_decks),
                           (long long)k, h->root, (long long)n_episodes, stream_id, (uint32_t)h->ctx->seed, (uint32_t)(h->ctx->seed >> 32), d_sums, d_r2);
    });
}

}  // extern "C"
