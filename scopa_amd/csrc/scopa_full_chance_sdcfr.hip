// scopa_full_chance_sdcfr.hip -- Single Deep CFR's external-sampling traversal and average policy on FullScopa over a set of decks
// (scopa_full_chance_sdcfr_* in include/scopa.h, where the contract is stated).  The forest form (traverse, average_policy) runs on the sub-games the
// exact sweeps cover: a round-boundary root with R <= 4 rounds to go and decks x 36^R <= 1 << 22.  The frontier form (traverse_frontier) keeps only
// the levels its traversals visit and runs from any round-boundary root, the deal included, on any deck count.
//
// The advantage net -- one per player, 96-128-64-40 -- reads 96 features that are a function of the mover's key pair (A, B) alone
// (scopa_full_sdcfr_tile.h), so it is defined at every key of every deck, trained on or not.
//
//   set-up    once per (root, handle decks), kept in the handle until another root is asked for: the deck-major forest of scopa_full_chance_forest.h is
//             expanded level by level through two state buffers; what stays is the key pair of every choice node (16 bytes) and the leaves' values
//             (float32, r2_p0 / 2); the states are freed.
//   policy    k_full_chance_sdcfr_policy: every choice node of the listed decks' trees under the net of its mover, 16 nodes a tile on
//             v_mfma_f32_16x16x4_f32.  The grid is cut by (player, chunk); a workgroup of four wavefronts loads its slices of ONE player's net into
//             registers once and loops over its chunk of that player's tiles; the layers are cut across the wavefronts and handed over through LDS.
//             Wavefronts 0..2 compute the third layer (48 = 3 x 16 outputs), the fourth finishes the tile: regret matching over the node's held cards
//             in ascending card id, policy[3] (float32) and the sampling thresholds[2] (uint64) -- or, in accumulate mode, acc += coef * policy.
//             Tiles never mix levels or decks; lanes past a level's end compute a copy of its last node and store nothing.
//   walk      k_full_chance_sdcfr_walk<TR>: a workgroup per traversal, the frontier of every level in LDS as node indices (child a of g is g n + a),
//             the other player's levels compare a Philox draw, named by the NODE, with the node's thresholds, values come back up in float32 in slot
//             order, and every traverser level's rows leave through 24-byte records in LDS in one sweep of 16-byte pieces.  No atomics.
//             LDS: 4 663 + 2 x 1 296 + 648 x 6 words = 44 572 bytes.
//   policy_at k_full_chance_sdcfr_policy_at: the policy launch's tile (ONE definition, scopa_full_sdcfr_tile.h) over a list of key pairs of one mover.
//   frontier  per chunk of traversals under the scratch budget: k_fsf_roots; per choice level policy_at over the level's pairs and k_fsf_expand<TR> (a
//             lane per child: the draw named by (level, path), the step, the child's state and key pair, or the leaf's value); per traverser level,
//             from the last to the first, k_fsf_up (an element per 16-byte piece of a row: features, regrets, the value handed up).  No atomics.
//   average   the policy launch once per snapshot in FIFO order with acc += coef * p (float32), then k_fsd_normalise in float64.
//   average_at k_full_chance_sdcfr_average_at: the same rows on a LIST of key pairs in ONE launch whatever the snapshot count.  A workgroup owns a fixed
//             share of the list's 16-pair tiles; it takes them 32 at a time, and for each such batch loops over the snapshots in FIFO order: the
//             register slices of the snapshot (fsd_load_slices), then the batch's tiles under it, acc = acc + coef * p (fsd_average_step) into the
//             workgroup's OWN accumulators in LDS (32 x 16 x 3 float32, written and read by the finishing wavefront alone), then the float64
//             normalisation of k_fsd_normalise and the rows.  One writer per accumulator: no atomics, no order between workgroups.
//   match     scopa_full_chance_sdcfr_match: scopa_full_chance_match's episodes with the nets' average policy in the agent's seat, level by level:
//             k_fsm_roots, then per choice level average_at over the contiguous half of the chunk whose mover is the agent (and over the other
//             half where the opponent is a second set of nets) and k_fsm_step (a lane per episode: the row or the opponent's store or uniform
//             play, the match's probability rule, its draw, fm_pick, the step, the one-card plies, the child's state and key pair; behind the last
//             level the six integer sums).
//   respond   scopa_full_chance_respond_nets_*: full_mccfr_walk<kRespond> at cut 0 against the nets' average policy, level by level in the frontier's
//             layout: k_fsf_roots; per responder level k_frn_claim (a lane per node: fw_claim in the responder's store, sigma of the frozen regrets,
//             (slot, sigma) kept per row) and k_frn_expand (a lane per child); per level of the other player average_at over the level's contiguous
//             pairs and k_frn_step (a lane per node: the match's rule on the row, the walk's draw at tag 144 + responder, fm_pick, the step); per
//             responder level going up k_frn_up (a lane per row: v, the float64 atomics into d_regret, count += 1).  Values are float64.
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "scopa_ctx.h"
#include "scopa_full_chance_forest.h"
#include "scopa_full_chance_match.h"
#include "scopa_full_sdcfr_tile.h"
#include "scopa_full_store_host.h"
#include "scopa_full_wide.h"
#include "scopa_philox.h"

using namespace scopa_full;
using scopa::fail;

namespace {

constexpr uint32_t kFsdPhiloxTag = 224u;          // counter word 3 = 224 + traverser
constexpr int kFsdPolicyWaves = 4, kFsdWalkThreads = 256;
constexpr int kFsdMaxPaths = 1296, kFsdMaxRowLevel = 648, kFsdMaxFrontier = 4663;   // 6^4; 3 x 6^3; 13 (6^4 - 1) / 5 + 6^4

// ---- set-up ----------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_fsd_roots(const scopa_full_state root, const uint8_t *__restrict__ decks, uint32_t n, scopa_full_state *__restrict__ state) {
    const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= n) return;
    state[d] = root_on(root, decks + 40u * d);
}

__global__ void __launch_bounds__(256)
k_fsd_keys(const scopa_full_state *__restrict__ st, uint32_t N, int p, ulonglong2 *__restrict__ keys) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const scopa_full_state s = st[i];
    const WideKey key = wide_key(s, p);
    keys[i] = make_ulonglong2(key.a, key.b);
}

__global__ void __launch_bounds__(256)
k_fsd_expand(const scopa_full_state *__restrict__ parent, uint32_t n_child, uint32_t tree_child, int p, int n, int round_end,
             const uint8_t *__restrict__ decks, scopa_full_state *__restrict__ child, float *__restrict__ leaf) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_child) return;
    const scopa_full_state s = full_chance_forest_child(parent, c, tree_child, p, n, round_end, decks);
    if (leaf) leaf[c] = (float)s.r2_p0 * 0.5f;
    else child[c] = s;
}

// ---- the policy launch -----------------------------------------------------------------------------------------------------------------------
// one player's tile list over one deck's tree: its choice levels in ascending order, a level's nodes sixteen at a time
struct FsdTiles {
    int n_lv, tile_off[9];                // tile_off[c]: tiles of one deck before the player's c-th level; tile_off[n_lv]: all of them
    uint32_t node_off[8], tree[8];        // the forest's nodes before that level; one deck's nodes in it
    int cards[8];
};
struct FsdPolicyArgs {
    FsdTiles t[2];
    int wg[2];                            // workgroups of player 0, of player 1 (0: that player is not evaluated)
    int m;                                // listed decks
};

// mode 0: pol[idx][3], thr[idx][2].  mode 1: acc[idx][3] += coef[0] * p
__global__ void __launch_bounds__(kFsdPolicyWaves * 64)
k_full_chance_sdcfr_policy(const ulonglong2 *__restrict__ g_keys, const int32_t *__restrict__ list, const FsdNet net0, const FsdNet net1, const FsdPolicyArgs args,
                           int mode, float *__restrict__ g_pol, unsigned long long *__restrict__ g_thr, const float *__restrict__ g_coef) {
    __shared__ FsdTileLds s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nj = lane & 15, q = lane >> 4;
    const int player = (int)blockIdx.x >= args.wg[0] ? 1 : 0;
    const int chunk = player ? (int)blockIdx.x - args.wg[0] : (int)blockIdx.x, n_chunks = args.wg[player];
    const FsdTiles &T = args.t[player];
    const int per_deck = T.tile_off[T.n_lv];
    const long long n_tiles = (long long)per_deck * args.m;
    const long long per = (n_tiles + n_chunks - 1) / n_chunks, t_begin = chunk * per, t_end = t_begin + per < n_tiles ? t_begin + per : n_tiles;
    FsdSlices W;
    fsd_load_slices(player ? net1 : net0, wave, lane, W);
    const float coef = mode ? g_coef[0] : 0.0f;

    for (long long t = t_begin; t < t_end; t++) {
        const int slot = (int)(t / per_deck), tt = (int)(t - (long long)slot * per_deck);
        int c = 0;
#pragma unroll
        for (int k = 1; k < 8; k++) c += (k < T.n_lv && tt >= T.tile_off[k]) ? 1 : 0;
        const uint32_t deck = list ? (uint32_t)list[slot] : (uint32_t)slot;
        const uint32_t tree = T.tree[c], j = (uint32_t)(tt - T.tile_off[c]) * 16u + (uint32_t)nj;
        const bool live = j < tree;
        const uint32_t idx = T.node_off[c] + deck * tree + (live ? j : tree - 1u);   // lanes beyond the level compute a copy of its last node and store nothing
        const int nl = T.cards[c];
        const ulonglong2 key = g_keys[idx];
        float pk = 0.0f;
        if (!fsd_tile_policy(W, s, key.x, key.y, nl, wave, lane, pk)) continue;
        if (mode) {
            if (live && q < 3) { float *a = g_pol + (size_t)idx * 3 + q; *a = *a + coef * pk; }
            continue;
        }
        if (live && q < 3) g_pol[(size_t)idx * 3 + q] = pk;
        unsigned long long thr[2] = {0ull, 0ull};
        fsd_tile_thresholds(s, nl, lane, pk, live, thr);
        if (q == 0 && live) {
            g_thr[(size_t)idx * 2] = thr[0];
            g_thr[(size_t)idx * 2 + 1] = thr[1];
        }
    }
}

// the policy launch on a LIST of n key pairs of one mover (n >= 1): the same tile, a workgroup loops over its share of the list's tiles; lanes past the
// list's end compute a copy of its last pair and store nothing.  The held cards are counted from word B
__global__ void __launch_bounds__(kFsdPolicyWaves * 64)
k_full_chance_sdcfr_policy_at(const ulonglong2 *__restrict__ g_keys, long long n, const FsdNet net, float *__restrict__ g_pol, unsigned long long *__restrict__ g_thr) {
    __shared__ FsdTileLds s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nj = lane & 15, q = lane >> 4;
    const long long n_tiles = (n + 15) / 16, n_chunks = gridDim.x;
    const long long per = (n_tiles + n_chunks - 1) / n_chunks, t_begin = (long long)blockIdx.x * per, t_end = t_begin + per < n_tiles ? t_begin + per : n_tiles;
    if (t_begin >= t_end) return;
    FsdSlices W;
    fsd_load_slices(net, wave, lane, W);
    for (long long t = t_begin; t < t_end; t++) {
        const long long j = t * 16 + nj;
        const bool live = j < n;
        const size_t idx = (size_t)(live ? j : n - 1);
        const ulonglong2 key = g_keys[idx];
        const int held = __popcll(key.y), nl = held < 3 ? held : 3;
        float pk = 0.0f;
        if (!fsd_tile_policy(W, s, key.x, key.y, nl, wave, lane, pk)) continue;
        if (live && q < 3) g_pol[idx * 3 + q] = pk;
        unsigned long long thr[2] = {0ull, 0ull};
        fsd_tile_thresholds(s, nl, lane, pk, live, thr);
        if (q == 0 && live) {
            g_thr[idx * 2] = thr[0];
            g_thr[idx * 2 + 1] = thr[1];
        }
    }
}

// ---- the frontier form ---------------------------------------------------------------------------------------------------------------------------
// A chunk of C traversals, numbered g0 .. g0 + C of the call's m x batch (g = slot * batch + i), level by level.  Level k of a traversal is a dense
// array of W_k paths; a level of the chunk is the C arrays one after the other: node (t, p) is element t W_k + p.
constexpr uint32_t kFsfPhiloxTag = 240u;          // counter word 3 = 240 + traverser
constexpr int kFsfMaxLevels = 24;

__device__ __forceinline__ uint32_t fsf_deck(const int32_t *__restrict__ list, long long g, int batch) {
    const int slot = (int)(g / batch);
    return list ? (uint32_t)list[slot] : (uint32_t)slot;
}

// a lane per traversal: the root on the traversal's deck and player 0's key pair there
__global__ void __launch_bounds__(256)
k_fsf_roots(const scopa_full_state root, const uint8_t *__restrict__ decks, const int32_t *__restrict__ list, long long g0, uint32_t C, int batch,
            scopa_full_state *__restrict__ state, ulonglong2 *__restrict__ keys) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= C) return;
    const scopa_full_state s = root_on(root, decks + 40u * fsf_deck(list, g0 + t, batch));
    state[t] = s;
    const WideKey key = wide_key(s, 0);
    keys[t] = make_ulonglong2(key.a, key.b);
}

// a lane per child of level k (mover k & 1 holding n cards; W paths a traversal): at the traverser's levels (trav) child a of path p is path p n + a;
// at the other player's ONE slot is drawn against the node's thresholds and the child keeps p.  After a round's last choice level the two one-card
// plies are played through.  The child's state and its mover's key pair go out, or -- below the last level -- the leaf's value r2_p0 / 2, negated
// for traverser 1
template <int TR>
__global__ void __launch_bounds__(256)
k_fsf_expand(const scopa_full_state *__restrict__ parent, const unsigned long long *__restrict__ g_thr, const uint8_t *__restrict__ decks,
             const int32_t *__restrict__ list, long long g0, int batch, uint32_t n_child, uint32_t W, int k, int n, int trav, int leaf, uint32_t seed_lo, uint32_t seed_hi,
             uint32_t iteration, uint32_t b0, scopa_full_state *__restrict__ child, ulonglong2 *__restrict__ keys, float *__restrict__ val) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_child) return;
    const uint32_t Wc = trav ? W * (uint32_t)n : W;   // paths a traversal has in the children's level
    const uint32_t t = c / Wc, r = c - t * Wc;
    const long long g = g0 + t;
    const uint32_t deck_id = fsf_deck(list, g, batch);
    uint32_t p, a;
    if (trav) { p = r / (uint32_t)n; a = r - p * (uint32_t)n; }
    else {
        p = r;
        const uint32_t trav_id = b0 + deck_id * (uint32_t)batch + (uint32_t)(g % batch);
        const scopa::philox_out x = scopa::philox4x32_10(((uint32_t)k << 24) | p, trav_id, iteration, kFsfPhiloxTag + (uint32_t)TR, seed_lo, seed_hi);
        const unsigned long long N = ((unsigned long long)(x.x0 >> 5) << 26) | (unsigned long long)(x.x1 >> 6);   // u = N * 2^-53 (u53)
        const unsigned long long *th = g_thr + ((size_t)t * W + p) * 2;
        const unsigned long long t0 = th[0], t1 = th[1];
        int s = (int)(t0 <= N) + (int)(t1 <= N);
        if (t0 == ~0ull) {   // a zero policy: uniform, (int)(u n) in float64
            const double u = (double)N * 0x1p-53;
            s = (int)(u * (double)n);
        }
        a = (uint32_t)(s < n - 1 ? s : n - 1);
    }
    const uint8_t *deck = decks + 40u * deck_id;
    scopa_full_state s = parent[(size_t)t * W + p];
    int cards[3];
    sorted_hand(s, k & 1, cards);
    step(s, deck, card_at(cards, (int)a));
    if ((k & 3) == 3) {                                           // the one-card plies: player 0's last card, then player 1's
        step(s, deck, hand_get(s, 0, 0));
        step(s, deck, hand_get(s, 1, 0));
    }
    if (leaf) {
        const float v = (float)s.r2_p0 * 0.5f;
        val[c] = TR == 0 ? v : -v;
        return;
    }
    child[c] = s;
    const WideKey key = wide_key(s, (k + 1) & 1);
    keys[c] = make_ulonglong2(key.a, key.b);
}

// one traverser level on the way back up, W paths a traversal holding n cards: element (row, piece) with row = t W + f.  Every piece restates the row's
// float32 arithmetic (v = 0; v = v + p[s] cfv[s]; d = cfv - v; d / (max|d| + 1e-8)); pieces 0..23 write the row's 96 features, 24..33 its 40 regrets,
// 16 bytes each; piece 0 also hands the node's value up (to d_root_values at the traverser's first level)
__global__ void __launch_bounds__(256)
k_fsf_up(const ulonglong2 *__restrict__ keys, const float *__restrict__ pol, const float *__restrict__ val_in, float *__restrict__ val_out, long long n_elems, uint32_t W,
         int n, int rank0, int rows, long long g0, unsigned long long write_base, uint32_t capacity, float *__restrict__ mem_feat, float *__restrict__ mem_regret) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_elems) return;
    const size_t rr = (size_t)(e / 34);
    const int i = (int)(e - (long long)rr * 34);
    const uint32_t t = (uint32_t)(rr / W), f = (uint32_t)(rr - (size_t)t * W);
    const ulonglong2 key = keys[rr];
    const float *pl = pol + rr * 3;
    float av[3] = {0.0f, 0.0f, 0.0f}, v = 0.0f;
    for (int k = 0; k < n; k++) { av[k] = val_in[rr * (size_t)n + k]; v = v + pl[k] * av[k]; }   // float32, slot order (no contraction: the build rounds every operation)
    float d[3], ri = 0.0f - v, mx = fabsf(ri);
    for (int k = 0; k < 3; k++) { d[k] = (k < n ? av[k] : 0.0f) - v; if (k < n) { const float a = fabsf(d[k]); mx = a > mx ? a : mx; } }
    if (mx > 0.0f) {
        const float den = mx + 1e-8f;
        ri = ri / den;
        for (int k = 0; k < 3; k++) d[k] = d[k] / den;
    }
    if (i == 0) val_out[rr] = v;
    const unsigned long long base = write_base + (unsigned long long)rows * (unsigned long long)(g0 + t) + (unsigned long long)rank0 + f;
    const size_t row = (size_t)(base % (unsigned long long)capacity);
    if (i < 24) {
        reinterpret_cast<float4 *>(mem_feat + row * kFsdIn)[i] =
            make_float4(fsd_feature(key.x, key.y, 4 * i), fsd_feature(key.x, key.y, 4 * i + 1), fsd_feature(key.x, key.y, 4 * i + 2), fsd_feature(key.x, key.y, 4 * i + 3));
    } else {
        const int c0 = 4 * (i - 24);
        float o[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int c = c0 + k;
            const int slot = __popcll(key.y & ((1ull << c) - 1ull));
            o[k] = ((key.y >> c) & 1ull) ? (slot == 0 ? d[0] : slot == 1 ? d[1] : d[2]) : ri;
        }
        reinterpret_cast<float4 *>(mem_regret + row * kFsdOut)[i - 24] = make_float4(o[0], o[1], o[2], o[3]);
    }
}

// ---- the walk launch ---------------------------------------------------------------------------------------------------------------------------
struct FsdWalkArgs {
    int L;                                // choice levels, 4 R
    int width[17], foff[18];              // the frontier of level lv: width[lv] nodes at s.node[foff[lv]..); level L = the leaves reached
    int rank0[16];                        // the rank of the first row of a traverser level (level-major, ascending path within a level)
    uint32_t node_off[16];                // the forest's nodes before level lv
    int rows;                             // ROWS(R)
};

struct FsdWalkLds {
    uint32_t node[kFsdMaxFrontier];       // index within its level of every frontier node, levels 0..L one after the other
    float val[2][kFsdMaxPaths];           // values on the way back up, by frontier position: the level at hand and the one below
    uint32_t rec[kFsdMaxRowLevel][6];     // the rows of the level at hand: rank | node (forest index) | regret of the cards not held | of the slots [3]
};
static_assert(sizeof(FsdWalkLds) == 44572, "LDS per workgroup");

__device__ __forceinline__ void fsd_sweep(const uint32_t (*rec)[6], int W, const ulonglong2 *__restrict__ keys, unsigned long long base, uint32_t capacity,
                                          float *__restrict__ mem_feat, float *__restrict__ mem_regret, int tid) {
    for (int e = tid; e < W * 34; e += kFsdWalkThreads) {
        const int rr = e / 34, i = e - rr * 34;
        const ulonglong2 key = keys[rec[rr][1]];
        const size_t row = (size_t)((base + (unsigned long long)rec[rr][0]) % (unsigned long long)capacity);
        if (i < 24) {
            reinterpret_cast<float4 *>(mem_feat + row * kFsdIn)[i] =
                make_float4(fsd_feature(key.x, key.y, 4 * i), fsd_feature(key.x, key.y, 4 * i + 1), fsd_feature(key.x, key.y, 4 * i + 2), fsd_feature(key.x, key.y, 4 * i + 3));
        } else {
            const int c0 = 4 * (i - 24);
            float o[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int c = c0 + k;
                const int slot = __popcll(key.y & ((1ull << c) - 1ull));
                o[k] = ((key.y >> c) & 1ull) ? __uint_as_float(rec[rr][3 + (slot < 2 ? slot : 2)]) : __uint_as_float(rec[rr][2]);
            }
            reinterpret_cast<float4 *>(mem_regret + row * kFsdOut)[i - 24] = make_float4(o[0], o[1], o[2], o[3]);
        }
    }
}

template <int TR>
__global__ void __launch_bounds__(kFsdWalkThreads)
k_full_chance_sdcfr_walk(const ulonglong2 *__restrict__ g_keys, const float *__restrict__ g_leaf, const int32_t *__restrict__ list, const float *__restrict__ g_pol,
                         const unsigned long long *__restrict__ g_thr, const FsdWalkArgs args, int batch, int wg_per_slot, float *__restrict__ mem_feat,
                         float *__restrict__ mem_regret, uint32_t capacity, unsigned long long write_base, float *__restrict__ root_values, uint32_t seed_lo,
                         uint32_t seed_hi, uint32_t iteration, uint32_t b0) {
    __shared__ FsdWalkLds s;
    const int tid = threadIdx.x, L = args.L;
    const int slot = (int)blockIdx.x / wg_per_slot, wg = (int)blockIdx.x - slot * wg_per_slot;
    const uint32_t deck = list ? (uint32_t)list[slot] : (uint32_t)slot;
    for (int i = wg; i < batch; i += wg_per_slot) {
        const uint32_t trav_id = b0 + deck * (uint32_t)batch + (uint32_t)i;
        const unsigned long long base = write_base + (unsigned long long)args.rows * ((unsigned long long)slot * (unsigned long long)batch + (unsigned long long)i);
        if (tid == 0) s.node[0] = deck;   // the root of deck d is node d of level 0
        __syncthreads();
        // ---- down: the frontier of every level ----
        for (int lv = 0; lv < L; lv++) {
            const int W = args.width[lv], o = args.foff[lv], o1 = args.foff[lv + 1], n = (lv & 3) < 2 ? 3 : 2;
            const bool trav = (lv & 1) == TR;
            for (int f = tid; f < W; f += kFsdWalkThreads) {
                const uint32_t g = s.node[o + f];
                if (trav) {
                    for (int k = 0; k < n; k++) s.node[o1 + f * n + k] = g * (uint32_t)n + (uint32_t)k;
                } else {
                    const scopa::philox_out x = scopa::philox4x32_10(((uint32_t)lv << 24) | g, trav_id, iteration, kFsdPhiloxTag + (uint32_t)TR, seed_lo, seed_hi);
                    const unsigned long long N = ((unsigned long long)(x.x0 >> 5) << 26) | (unsigned long long)(x.x1 >> 6);   // u = N * 2^-53 (u53)
                    const unsigned long long *th = g_thr + ((size_t)args.node_off[lv] + g) * 2;
                    const unsigned long long t0 = th[0], t1 = th[1];
                    int a = (int)(t0 <= N) + (int)(t1 <= N);
                    if (t0 == ~0ull) {   // a zero policy: uniform, (int)(u n) in float64
                        const double u = (double)N * 0x1p-53;
                        a = (int)(u * (double)n);
                    }
                    a = a < n - 1 ? a : n - 1;
                    s.node[o1 + f] = g * (uint32_t)n + (uint32_t)a;
                }
            }
            __syncthreads();
        }
        // ---- the leaves: r2_p0 / 2, negated for traverser 1 ----
        int cur = 0;
        for (int f = tid; f < args.width[L]; f += kFsdWalkThreads) {
            const float v = g_leaf[s.node[args.foff[L] + f]];
            s.val[cur][f] = TR == 0 ? v : -v;
        }
        __syncthreads();
        // ---- up: the traverser's levels; the other player's hand their sampled child's value on at the same position ----
        for (int lv = L - 1; lv >= 0; lv--) {
            if ((lv & 1) != TR) continue;
            const int W = args.width[lv], o = args.foff[lv], n = (lv & 3) < 2 ? 3 : 2;
            for (int f = tid; f < W; f += kFsdWalkThreads) {
                const uint32_t idx = args.node_off[lv] + s.node[o + f];
                const float *pl = g_pol + (size_t)idx * 3;
                float av[3] = {0.0f, 0.0f, 0.0f}, v = 0.0f;
                for (int k = 0; k < n; k++) { av[k] = s.val[cur][f * n + k]; v = v + pl[k] * av[k]; }   // float32, slot order (no contraction: the build rounds every operation)
                float d[3], ri = 0.0f - v, mx = fabsf(ri);
                for (int k = 0; k < 3; k++) { d[k] = (k < n ? av[k] : 0.0f) - v; if (k < n) { const float a = fabsf(d[k]); mx = a > mx ? a : mx; } }
                if (mx > 0.0f) {
                    const float den = mx + 1e-8f;
                    ri = ri / den;
                    for (int k = 0; k < 3; k++) d[k] = d[k] / den;
                }
                uint32_t *rec = s.rec[f];
                rec[0] = (uint32_t)(args.rank0[lv] + f); rec[1] = idx; rec[2] = __float_as_uint(ri);
                rec[3] = __float_as_uint(d[0]); rec[4] = __float_as_uint(d[1]); rec[5] = __float_as_uint(d[2]);
                s.val[cur ^ 1][f] = v;
            }
            __syncthreads();
            fsd_sweep(s.rec, W, g_keys, base, capacity, mem_feat, mem_regret, tid);
            cur ^= 1;
            __syncthreads();
        }
        if (tid == 0) root_values[(size_t)slot * batch + i] = s.val[cur][0];
        __syncthreads();
    }
}

// ---- the average policy ------------------------------------------------------------------------------------------------------------------------
// a lane per node of one level: float64 normalisation of the accumulated float32 policy over the legal slots, uniform where the sum is 0 or not finite
__global__ void __launch_bounds__(256)
k_fsd_normalise(const ulonglong2 *__restrict__ keys, const float *__restrict__ acc, uint32_t N, int n, unsigned long long *__restrict__ out_keys,
                double *__restrict__ out_pol) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    double a[3] = {(double)acc[(size_t)i * 3], (double)acc[(size_t)i * 3 + 1], n > 2 ? (double)acc[(size_t)i * 3 + 2] : 0.0};
    double sum = a[0] + a[1];
    if (n > 2) sum = sum + a[2];
    const bool ok = sum > 0.0 && sum <= 1.7976931348623157e308;   // positive and finite (a NaN fails both)
#pragma unroll
    for (int k = 0; k < 3; k++) out_pol[(size_t)i * 3 + k] = k < n ? (ok ? a[k] / sum : 1.0 / (double)n) : 0.0;
    const ulonglong2 key = keys[i];
    out_keys[(size_t)i * 2] = key.x;
    out_keys[(size_t)i * 2 + 1] = key.y;
}

}  // namespace

namespace scopa_full {

// the forest of one (root, decks): what stays of it after set-up
struct FsdForest {
    Shape s;
    uint32_t n = 0;
    ulonglong2 *d_keys = nullptr;         // [T] the key pair of every choice node, level-major, deck-major within a level
    float *d_leaf = nullptr;              // [n 36^R]
};

struct FwSdcfr {
    bool built = false;
    scopa_full_state root;                // the root the forest was built for (hands cleared)
    FsdForest f;
    float *d_pol = nullptr;               // [T][3]
    unsigned long long *d_thr = nullptr;  // [T][2]
    int32_t *d_list = nullptr;            // [n_decks]
    uint64_t visits = 0;
    bool called = false;                  // a traversal call has filled the tables of the forest at hand
    void *d_scratch = nullptr;            // the frontier form's level states, keys, policies and values (scopa_full_chance_sdcfr_traverse_frontier)
    size_t scratch_bytes = 0;
};

static void forest_free(FsdForest &f) {
    if (f.d_keys) (void)hipFree(f.d_keys);
    if (f.d_leaf) (void)hipFree(f.d_leaf);
    f.d_keys = nullptr; f.d_leaf = nullptr;
}

void chance_sdcfr_free(FwSdcfr *c) {
    if (!c) return;
    forest_free(c->f);
    if (c->d_pol) (void)hipFree(c->d_pol);
    if (c->d_thr) (void)hipFree(c->d_thr);
    if (c->d_list) (void)hipFree(c->d_list);
    if (c->d_scratch) (void)hipFree(c->d_scratch);
    delete c;
}

}  // namespace scopa_full

namespace {

scopa_full_state bare_root(scopa_full_state r) {
    r.game = 0u;
    r.hand[0] = r.hand[1] = 0u;
    r.nh[0] = r.nh[1] = 0;
    memset(r.pad, 0, sizeof(r.pad));
    return r;
}

// the forest below `root` on the n decks at d_decks (device): keys and leaves stay, the states go.  Synchronises the stream
int32_t forest_build(scopa_ctx *ctx, const scopa_full_state &root, const uint8_t *d_decks, uint32_t n, int R, FsdForest &f) {
    forest_free(f);
    f.s = shape_of(R, n);
    f.n = n;
    const Shape &s = f.s;
    hipStream_t st = ctx->stream;
    scopa_full_state *d_state[2] = {nullptr, nullptr};
    const size_t T = s.off[s.L];
    bool ok = hipMalloc((void **)&f.d_keys, T * sizeof(ulonglong2)) == hipSuccess && hipMalloc((void **)&f.d_leaf, (size_t)s.size[s.L] * sizeof(float)) == hipSuccess &&
              hipMalloc((void **)&d_state[0], (size_t)s.largest * sizeof(scopa_full_state)) == hipSuccess &&
              hipMalloc((void **)&d_state[1], (size_t)s.largest * sizeof(scopa_full_state)) == hipSuccess;
    hipError_t err = hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(k_fsd_roots, grid_of(n), dim3(256), 0, st, root, d_decks, n, d_state[0]);
        for (int lv = 0; lv < s.L && err == hipSuccess; lv++) {
            const int n_act = cards_of(lv), p = mover_of(lv);
            const bool leaf = lv + 1 == s.L;
            const scopa_full_state *cur = d_state[lv & 1];
            hipLaunchKernelGGL(k_fsd_keys, grid_of(s.size[lv]), dim3(256), 0, st, cur, s.size[lv], p, f.d_keys + s.off[lv]);
            hipLaunchKernelGGL(k_fsd_expand, grid_of(s.size[lv + 1]), dim3(256), 0, st, cur, s.size[lv + 1], s.size[lv + 1] / n, p, n_act, (int)((lv & 3) == 3), d_decks,
                               leaf ? (scopa_full_state *)nullptr : d_state[(lv + 1) & 1], leaf ? f.d_leaf : (float *)nullptr);
            err = hipGetLastError();
        }
    }
    const hipError_t e2 = hipStreamSynchronize(st);   // the states go away below
    if (d_state[0]) (void)hipFree(d_state[0]);
    if (d_state[1]) (void)hipFree(d_state[1]);
    if (!ok) { forest_free(f); return fail(ctx, SCOPA_ENOMEM, "scopa_full_chance_sdcfr: no device memory for the forest"); }
    if (err != hipSuccess || e2 != hipSuccess) { forest_free(f); return fail(ctx, SCOPA_EHIP, "scopa_full_chance_sdcfr: forest set-up", err != hipSuccess ? err : e2); }
    return SCOPA_OK;
}

// the checks every entry point shares, in cfr_iterate's order; n_decks: the decks the forest would hold
int32_t check_root(scopa_ctx *ctx, const scopa_full_state &root, uint64_t n_decks, int *R_out) {
    SC_REQUIRE(ctx, root_ok(root), SCOPA_EINVAL, "scopa_full_chance_sdcfr: the root must be a non-terminal state at a round boundary (step % 6 == 0)");
    const int R = 6 - (int)root.round;
    SC_REQUIRE(ctx, R <= kMaxRounds, SCOPA_ELIMIT, "scopa_full_chance_sdcfr: more than 4 rounds from the root");
    uint64_t leaves = n_decks;
    for (int r = 0; r < R; r++) leaves *= 36ull;
    SC_REQUIRE(ctx, leaves <= kMaxLeaves, SCOPA_ELIMIT, "scopa_full_chance_sdcfr: decks x 36^R above 1 << 22 (89 decks at R = 3, 2 at R = 4)");
    *R_out = R;
    return SCOPA_OK;
}

// the handle's forest for `root`, built where it is not the one at hand; (re)allocates the tables
int32_t ensure_handle_forest(scopa_full_chance *h, const scopa_full_state &root, int R) {
    scopa_ctx *ctx = h->ctx;
    if (!h->sd) {
        h->sd = new (std::nothrow) FwSdcfr;
        if (!h->sd) return fail(ctx, SCOPA_ENOMEM, "scopa_full_chance_sdcfr: host record");
    }
    FwSdcfr *c = h->sd;
    const scopa_full_state bare = bare_root(root);
    if (c->built && memcmp(&bare, &c->root, sizeof(bare)) == 0) return SCOPA_OK;
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));   // an earlier call's launches may still read the old forest
    c->built = false; c->called = false;
    if (c->d_pol) { (void)hipFree(c->d_pol); c->d_pol = nullptr; }
    if (c->d_thr) { (void)hipFree(c->d_thr); c->d_thr = nullptr; }
    if (int32_t rc = forest_build(ctx, root, h->d_decks, (uint32_t)h->n_decks, R, c->f)) return rc;
    const size_t T = c->f.s.off[c->f.s.L];
    if (hipMalloc((void **)&c->d_pol, T * 3 * sizeof(float)) != hipSuccess || hipMalloc((void **)&c->d_thr, T * 2 * sizeof(unsigned long long)) != hipSuccess ||
        (!c->d_list && hipMalloc((void **)&c->d_list, (size_t)h->n_decks * 4) != hipSuccess))
        return fail(ctx, SCOPA_ENOMEM, "scopa_full_chance_sdcfr: no device memory for the policy tables");
    SC_HIP(ctx, hipMemsetAsync(c->d_pol, 0, T * 3 * sizeof(float), ctx->stream));
    SC_HIP(ctx, hipMemsetAsync(c->d_thr, 0, T * 2 * sizeof(unsigned long long), ctx->stream));
    c->root = bare;
    c->built = true;
    return SCOPA_OK;
}

FsdTiles tiles_of(const Shape &s, uint32_t n, int player) {
    FsdTiles t;
    memset(&t, 0, sizeof(t));
    int at = 0;
    for (int lv = player; lv < s.L; lv += 2) {
        const int c = t.n_lv++;
        t.tile_off[c] = at;
        t.node_off[c] = (uint32_t)s.off[lv];
        t.tree[c] = s.size[lv] / n;
        t.cards[c] = cards_of(lv);
        at += (int)((t.tree[c] + 15u) / 16u);
    }
    for (int c = t.n_lv; c < 9; c++) t.tile_off[c] = at;
    return t;
}

// the policy launch over m decks of forest f (list: device, or NULL = decks 0..m-1); players: bit p set = player p's levels are evaluated
int32_t launch_policy(scopa_ctx *ctx, const FsdForest &f, const int32_t *d_list, int m, int players, const FsdNet &net0, const FsdNet &net1, int mode, float *d_pol,
                      unsigned long long *d_thr, const float *d_coef) {
    FsdPolicyArgs a;
    a.t[0] = tiles_of(f.s, f.n, 0);
    a.t[1] = tiles_of(f.s, f.n, 1);
    a.m = m;
    long long tiles[2];
    for (int p = 0; p < 2; p++) tiles[p] = ((players >> p) & 1) ? (long long)a.t[p].tile_off[a.t[p].n_lv] * m : 0;
    const long long all = tiles[0] + tiles[1];
    if (!all) return SCOPA_OK;
    const long long budget = std::min<long long>(8ll * ctx->n_cus, all);   // about eight workgroups per compute unit, cut between the players by their tiles
    for (int p = 0; p < 2; p++) a.wg[p] = tiles[p] ? (int)std::max<long long>(1, std::min<long long>(tiles[p], (budget * tiles[p] + all / 2) / all)) : 0;
    hipLaunchKernelGGL(k_full_chance_sdcfr_policy, dim3((unsigned)(a.wg[0] + a.wg[1])), dim3(kFsdPolicyWaves * 64), 0, ctx->stream, (const ulonglong2 *)f.d_keys, d_list, net0,
                       net1, a, mode, d_pol, d_thr, d_coef);
    SC_HIP(ctx, hipGetLastError());
    return SCOPA_OK;
}

FsdWalkArgs walk_args_of(const Shape &s, int traverser) {
    FsdWalkArgs a;
    memset(&a, 0, sizeof(a));
    a.L = s.L;
    int w = 1, at = 0, rank = 0;
    for (int lv = 0; lv <= s.L; lv++) {
        a.width[lv] = w;
        a.foff[lv] = at;
        at += w;
        if (lv == s.L) break;
        a.node_off[lv] = (uint32_t)s.off[lv];
        if ((lv & 1) == traverser) { a.rank0[lv] = rank; rank += w; w *= cards_of(lv); }
    }
    a.foff[s.L + 1] = at;
    a.rows = rank;
    return a;
}

int64_t rows_of(int R) { int64_t p = 1; for (int r = 0; r < R; r++) p *= 6; return 4 * (p - 1) / 5; }

bool list_ok(int n, int m, const int32_t *h_list) {
    std::vector<char> seen((size_t)n, 0);
    for (int k = 0; k < m; k++) {
        const int32_t d = h_list[k];
        if (d < 0 || d >= n || seen[(size_t)d]) return false;
        seen[(size_t)d] = 1;
    }
    return true;
}

// what both traversal forms ask of a call, in one order, before anything is launched or written.  frontier: any round-boundary root, no forest cap
int32_t check_traverse(scopa_full_chance *h, const scopa_full_state *root_state, bool frontier, int32_t traverser, int32_t batch, int32_t m_list, const int32_t *h_list,
                       const float *d_w1, const float *d_b1, const float *d_w2, const float *d_b2, const float *d_w3, const float *d_b3, const float *d_mem_feat,
                       const float *d_mem_regret, int64_t capacity, int64_t write_base, const float *d_root_values, uint32_t b0, scopa_full_state *root_out, int *R_out,
                       int *m_out) {
    scopa_ctx *ctx = h->ctx;
    const int n = h->n_decks;
    SC_REQUIRE(ctx, traverser == 0 || traverser == 1, SCOPA_EINVAL, "scopa_full_chance_sdcfr_traverse: traverser must be 0 or 1");
    scopa_full_state root = root_state ? *root_state : h->root;
    int R = 0;
    if (frontier) {
        SC_REQUIRE(ctx, root_ok(root), SCOPA_EINVAL, "scopa_full_chance_sdcfr_traverse_frontier: the root must be a non-terminal state at a round boundary (step % 6 == 0)");
        R = 6 - (int)root.round;
    } else if (int32_t rc = check_root(ctx, root, (uint64_t)n, &R)) return rc;
    root.game = 0u;
    for (int32_t d = 0; d < n; d++)
        SC_REQUIRE(ctx, deck_fits(h->decks + 40 * (size_t)d, root), SCOPA_EINVAL, "scopa_full_chance_sdcfr_traverse: a deck of the handle does not pass create's check against the root of the call");
    SC_REQUIRE(ctx, h_list ? (m_list >= 1 && m_list <= n) : (m_list == 0 || m_list == n), SCOPA_EINVAL,
               "scopa_full_chance_sdcfr_traverse: a list holds 1 .. n decks; without a list m is 0 (or n): all decks");
    SC_REQUIRE(ctx, !h_list || list_ok(n, m_list, h_list), SCOPA_EINVAL, "scopa_full_chance_sdcfr_traverse: a listed deck is outside [0, n) or listed twice");
    SC_REQUIRE(ctx, batch >= 1 && batch <= (1 << 24), SCOPA_EINVAL, "scopa_full_chance_sdcfr_traverse: batch outside [1, 1 << 24]");
    const int m = h_list ? m_list : n;
    SC_REQUIRE(ctx, d_w1 && d_b1 && d_w2 && d_b2 && d_w3 && d_b3 && d_mem_feat && d_mem_regret && d_root_values, SCOPA_EINVAL, "scopa_full_chance_sdcfr_traverse: NULL device pointer");
    const uintptr_t wany = (uintptr_t)d_w1 | (uintptr_t)d_b1 | (uintptr_t)d_w2 | (uintptr_t)d_b2 | (uintptr_t)d_w3 | (uintptr_t)d_b3 | (uintptr_t)d_root_values;
    SC_REQUIRE(ctx, (wany & 3) == 0 && ((uintptr_t)d_mem_feat & 15) == 0 && ((uintptr_t)d_mem_regret & 15) == 0, SCOPA_EINVAL,
               "scopa_full_chance_sdcfr_traverse: memory rows are stored 16 bytes at a time: d_mem_feat and d_mem_regret must be 16-byte aligned, the weights 4-byte");
    const int64_t rows = rows_of(R);
    SC_REQUIRE(ctx, capacity >= rows && capacity < ((int64_t)1 << 30) && write_base >= 0 && write_base < capacity, SCOPA_EINVAL,
               "scopa_full_chance_sdcfr_traverse: write_base must lie in [0, capacity), capacity in [ROWS, 2^30) rows");
    SC_REQUIRE(ctx, rows * m * batch <= capacity, SCOPA_EINVAL, "scopa_full_chance_sdcfr_traverse: memory ring too small for ROWS * m * batch rows");
    SC_REQUIRE(ctx, (uint64_t)b0 + (uint64_t)n * (uint64_t)batch <= ((uint64_t)1 << 32), SCOPA_EINVAL, "scopa_full_chance_sdcfr_traverse: traversal ids b0 + n_decks * batch exceed 2^32");
    *root_out = root;
    *R_out = R;
    *m_out = m;
    return SCOPA_OK;
}

// the scratch of the frontier form, in the handle's Deep CFR record (made here where no forest call has), grown where a call needs more
int32_t ensure_frontier_scratch(scopa_full_chance *h, size_t bytes) {
    scopa_ctx *ctx = h->ctx;
    if (!h->sd) {
        h->sd = new (std::nothrow) FwSdcfr;
        if (!h->sd) return fail(ctx, SCOPA_ENOMEM, "scopa_full_chance_sdcfr: host record");
    }
    FwSdcfr *c = h->sd;
    if (!c->d_list && hipMalloc((void **)&c->d_list, (size_t)h->n_decks * 4) != hipSuccess)
        return fail(ctx, SCOPA_ENOMEM, "scopa_full_chance_sdcfr_traverse_frontier: no device memory for the list");
    if (c->scratch_bytes >= bytes) return SCOPA_OK;
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));   // an earlier call's launches may still use the old block
    if (c->d_scratch) (void)hipFree(c->d_scratch);
    c->d_scratch = nullptr; c->scratch_bytes = 0;
    if (hipMalloc((void **)&c->d_scratch, bytes) != hipSuccess) return fail(ctx, SCOPA_ENOMEM, "scopa_full_chance_sdcfr_traverse_frontier: no device memory for the scratch");
    c->scratch_bytes = bytes;
    return SCOPA_OK;
}

// the policy launch on n >= 1 key pairs of one mover: about eight workgroups per compute unit, none without a tile
void launch_policy_at(scopa_ctx *ctx, const ulonglong2 *d_keys, long long n, const FsdNet &net, float *d_pol, unsigned long long *d_thr) {
    const long long tiles = (n + 15) / 16;
    const long long wg = std::min<long long>(8ll * ctx->n_cus, tiles);
    hipLaunchKernelGGL(k_full_chance_sdcfr_policy_at, dim3((unsigned)wg), dim3(kFsdPolicyWaves * 64), 0, ctx->stream, d_keys, n, net, d_pol, d_thr);
}

// bytes a traversal of the frontier form takes in scratch: two state buffers, the other player's keys, one level's policy and thresholds and two
// value buffers of 6^R paths, and the key pair and policy of every row
constexpr size_t kFsfPerPath = 2 * sizeof(scopa_full_state) + 16 + 12 + 16 + 2 * 4, kFsfPerRow = 16 + 12;
static_assert(sizeof(scopa_full_state) == 64, "the frontier's byte budget counts 64-byte states");

// ---- the average policy on a list ------------------------------------------------------------------------------------------------------------------
// one player's snapshots on the device: six tensors [max_size][...], the FIFO slot list and the float32 coefficients
struct FsdSnaps {
    const float *w1, *b1, *w2, *b2, *w3, *b3;
    const int32_t *slots;
    const float *coef;
    int n_snap;
};

constexpr int kFsaBatch = 32;             // tiles a workgroup keeps accumulators for at a time: a slice reload (110 floats a lane) per 32 tiles at most

// the float32 accumulate of the average policy: mode 1 of k_full_chance_sdcfr_policy compiles `*a + coef * pk` to v_mul_f32 then v_add_f32 (the build
// contracts nothing), which is what the two rounded operations here are
__device__ __forceinline__ float fsd_average_step(float acc, float coef, float p) { return __fadd_rn(acc, __fmul_rn(coef, p)); }

__global__ void __launch_bounds__(kFsdPolicyWaves * 64)
k_full_chance_sdcfr_average_at(const ulonglong2 *__restrict__ g_keys, long long n, const FsdSnaps S, double *__restrict__ g_out) {
    __shared__ FsdTileLds s;
    __shared__ float s_acc[kFsaBatch][3][16];   // the workgroup's own accumulators: [tile of the batch][slot][node], the fourth wavefront's alone
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nj = lane & 15, q = lane >> 4;
    const long long n_tiles = (n + 15) / 16, n_chunks = gridDim.x;
    const long long per = (n_tiles + n_chunks - 1) / n_chunks, t_begin = (long long)blockIdx.x * per, t_end = t_begin + per < n_tiles ? t_begin + per : n_tiles;
    if (t_begin >= t_end) return;
    for (long long b0 = t_begin; b0 < t_end; b0 += kFsaBatch) {
        const int nb = t_end - b0 < kFsaBatch ? (int)(t_end - b0) : kFsaBatch;
        if (wave == 3 && q < 3)
            for (int k = 0; k < nb; k++) s_acc[k][q][nj] = 0.0f;
        for (int i = 0; i < S.n_snap; i++) {   // FIFO order
            const size_t sl = (size_t)S.slots[i];
            const FsdNet net{S.w1 + sl * kFsdH1 * kFsdIn, S.b1 + sl * kFsdH1, S.w2 + sl * kFsdH2 * kFsdH1, S.b2 + sl * kFsdH2, S.w3 + sl * kFsdOut * kFsdH2, S.b3 + sl * kFsdOut};
            FsdSlices W;
            fsd_load_slices(net, wave, lane, W);
            const float coef = S.coef[i];
            for (int k = 0; k < nb; k++) {
                const long long j = (b0 + k) * 16 + nj;
                const size_t idx = (size_t)(j < n ? j : n - 1);   // lanes past the list's end compute a copy of its last pair and store nothing
                const ulonglong2 key = g_keys[idx];
                const int held = __popcll(key.y), nl = held < 3 ? held : 3;
                float pk = 0.0f;
                if (!fsd_tile_policy(W, s, key.x, key.y, nl, wave, lane, pk)) continue;
                if (q < 3) s_acc[k][q][nj] = fsd_average_step(s_acc[k][q][nj], coef, pk);
            }
        }
        if (wave != 3) continue;
        sd_order();
        if (q == 0)
            for (int k = 0; k < nb; k++) {   // k_fsd_normalise's rule over the held cards
                const long long j = (b0 + k) * 16 + nj;
                if (j >= n) continue;
                const int held = __popcll(g_keys[j].y), nl = held < 3 ? held : 3;
                const double a[3] = {(double)s_acc[k][0][nj], (double)s_acc[k][1][nj], nl > 2 ? (double)s_acc[k][2][nj] : 0.0};
                double sum = a[0] + a[1];
                if (nl > 2) sum = sum + a[2];
                const bool ok = sum > 0.0 && sum <= 1.7976931348623157e308;   // positive and finite (a NaN fails both)
#pragma unroll
                for (int c = 0; c < 3; c++) g_out[(size_t)j * 3 + c] = c < nl ? (ok ? a[c] / sum : 1.0 / (double)nl) : 0.0;
            }
        sd_order();
    }
}

// ONE launch whatever S.n_snap.  A slice reload costs about 2.6 tiles of one workgroup alone on its compute unit (measured: 6.4 us against 2.45 us a
// tile), and the launches of a match follow one another on one stream, so a short list is cut for latency: a workgroup per tile until every compute
// unit has one, then up to four tiles each.  From there on the reload is amortised: two workgroups per compute unit until each holds a batch of 32
// tiles, then more workgroups, eight per compute unit at most (the sweep: `grid` in profiles/full_chance_net_match_bench.json)
void launch_average_at(scopa_ctx *ctx, const ulonglong2 *d_keys, long long n, const FsdSnaps &S, double *d_out) {
    const long long tiles = (n + 15) / 16;
    const long long cus = ctx->n_cus;
    long long wg = tiles <= 4 * cus ? std::min(tiles, cus) : std::max(2 * cus, std::min(8 * cus, tiles / kFsaBatch));
    if (ctx->full_avg_grid > 0) wg = std::min<long long>(tiles, ctx->full_avg_grid);   // scopa_full_chance_debug_sdcfr_average_grid: a test's or a sweep's grid
    hipLaunchKernelGGL(k_full_chance_sdcfr_average_at, dim3((unsigned)wg), dim3(kFsdPolicyWaves * 64), 0, ctx->stream, d_keys, n, S, d_out);
}

// what a caller's snapshot set must satisfy before anything is launched
bool snaps_ok(int32_t n_snap, int32_t max_size, const float *const w[6], const int32_t *h_slots, const float *d_coef) {
    if (n_snap < 0 || max_size < 0 || n_snap > max_size) return false;
    if (!n_snap) return true;
    uintptr_t any = (uintptr_t)d_coef;
    for (int k = 0; k < 6; k++) { if (!w[k]) return false; any |= (uintptr_t)w[k]; }
    if (!h_slots || !d_coef || (any & 3)) return false;
    for (int32_t s = 0; s < n_snap; s++) if (h_slots[s] < 0 || h_slots[s] >= max_size) return false;
    return true;
}

// ---- the match ------------------------------------------------------------------------------------------------------------------------------------
// A chunk of C episodes, numbered g0 .. g0 + C of the call's n.  Episode i sits in seat 0 where 2 i < n, so a chunk's episodes of one seat are contiguous.
constexpr size_t kFsmPerEpisode = 2 * sizeof(scopa_full_state) + 16 + 24 + 24 + 8;   // two states, the key pair, the policy row, the trace row, r2 (padded)

__device__ __forceinline__ const uint8_t *fsm_deck(const uint8_t *__restrict__ decks, long long k_decks, long long i, long long n) {
    const long long j = 2 * i < n ? i : i - (n + 1) / 2;
    return decks + 40 * (j % k_decks);
}

// a lane per episode: the root on the episode's deck, player 0's key pair there, an empty trace row
__global__ void __launch_bounds__(256)
k_fsm_roots(const scopa_full_state root, const uint8_t *__restrict__ decks, long long k_decks, long long g0, uint32_t C, long long n,
            scopa_full_state *__restrict__ state, ulonglong2 *__restrict__ keys, int8_t *__restrict__ trace) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= C) return;
    const scopa_full_state s = root_on(root, fsm_deck(decks, k_decks, g0 + t, n));
    state[t] = s;
    const WideKey key = wide_key(s, 0);
    keys[t] = make_ulonglong2(key.a, key.b);
    if (trace)
        for (int k = 0; k < kFsfMaxLevels; k++) trace[(size_t)t * kFsfMaxLevels + k] = (int8_t)-1;
}

// a lane per episode at choice level k (mover k & 1): prob is uniform, or -- for the agent, and for an opponent that is a set of nets -- the row of
// average_at under the match's rule (total over the held cards > 1e-12: row / total), or the opponent store's row as full_chance_episode<true> reads it;
// the match's draw, fm_pick, the step and, behind a round's last choice level, the two one-card plies.  The child's state and its mover's key pair go
// out, or -- behind the last level -- the episode's r2 and the six sums
template <bool kStore>
__global__ void __launch_bounds__(256)
k_fsm_step(const scopa_full_state *__restrict__ parent, const double *__restrict__ pol, const FwSlot *__restrict__ opp_tab, uint32_t opp_mask, int opp_nets,
           const uint8_t *__restrict__ decks, long long k_decks, long long g0, uint32_t C, long long n, int k, int level0, int leaf, uint32_t stream_id,
           uint32_t seed_lo, uint32_t seed_hi, scopa_full_state *__restrict__ child, ulonglong2 *__restrict__ keys, int8_t *__restrict__ trace,
           long long *__restrict__ sums, int8_t *__restrict__ r2_agent) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= C) return;
    const long long i = g0 + t;
    const int seat = 2 * i < n ? 0 : 1;
    const uint8_t *deck = fsm_deck(decks, k_decks, i, n);
    scopa_full_state s = parent[t];
    const int p = k & 1, nl = nh_of(s, p);
    int cards[3];
    sorted_hand(s, p, cards);
    double prob[3];
    fw_uniform_probs(nl, prob);
    double S[3] = {0.0, 0.0, 0.0};
    bool have = false;
    if (p == seat || opp_nets) {
#pragma unroll
        for (int c = 0; c < 3; c++) S[c] = pol[(size_t)t * 3 + c];
        have = true;
    } else if (kStore) {
        const WideKey key = wide_key(s, p);
        const int slot = fw_find(opp_tab, opp_mask, key.a, key.b);
        if (slot >= 0) {
#pragma unroll
            for (int c = 0; c < 3; c++) S[c] = opp_tab[slot].strategy[c];
            have = true;
        }
    }
    if (have) fw_row_probs(S, nl, prob);
    const scopa::philox_out x = scopa::philox4x32_10((uint32_t)i, (uint32_t)((unsigned long long)i >> 32), (stream_id << 8) | (uint32_t)s.step, kMatchTag, seed_lo, seed_hi);
    const int a = fm_pick(prob, nl, scopa::u53(x.x0, x.x1));
    if (trace) trace[(size_t)t * kFsfMaxLevels + level0 + k] = (int8_t)a;
    step(s, deck, card_at(cards, a));
    if ((k & 3) == 3) {                                           // the one-card plies: player 0's last card, then player 1's
        step(s, deck, hand_get(s, 0, 0));
        step(s, deck, hand_get(s, 1, 0));
    }
    if (!leaf) {
        child[t] = s;
        const WideKey key = wide_key(s, (k + 1) & 1);
        keys[t] = make_ulonglong2(key.a, key.b);
        return;
    }
    const long long r2 = seat ? -(long long)s.r2_p0 : (long long)s.r2_p0;
    if (r2_agent) r2_agent[t] = (int8_t)r2;
    atomicAdd((unsigned long long *)sums + seat, (unsigned long long)r2);                      // (two's complement: the sums are signed)
    atomicAdd((unsigned long long *)sums + 2 + seat, (unsigned long long)(r2 * r2));
    atomicAdd((unsigned long long *)sums + 4, (unsigned long long)(seat ? s.scopas[1] : s.scopas[0]));
    atomicAdd((unsigned long long *)sums + 5, (unsigned long long)(seat ? s.scopas[0] : s.scopas[1]));
}

// ---- the response walk against the nets ------------------------------------------------------------------------------------------------------------
// full_mccfr_walk<kRespond> at cut 0 in the frontier's layout: a chunk of C traversals level by level, node (t, p) of level k at element t W_k + p, p the
// responder's own slot choices in mixed radix -- the walk's q.  The responder's levels widen (child a of p is p n + a), the other player's keep p.
// Values are float64 throughout.  Per path: two states, the key pair, the average row, two values; per responder row: sigma and the slot
constexpr size_t kFrnPerPath = 2 * sizeof(scopa_full_state) + 16 + 24 + 2 * 8, kFrnPerRow = 24 + 4;

struct FrnDraw { uint32_t iteration, seed_lo, seed_hi; };   // what fm_draw reads of a launch's arguments

// a responder level going down, a lane per node: the pair claimed in the responder's store (a full probe: slot -1, dropped += 1, a zero regret row), sigma
// of the row's FROZEN regrets; (slot, sigma[3]) kept per row for the way up
__global__ void __launch_bounds__(256)
k_frn_claim(const ulonglong2 *__restrict__ keys, uint32_t n_nodes, int n, FwSlot *__restrict__ tab, uint32_t mask, unsigned long long *__restrict__ cnt,
            int32_t *__restrict__ row_slot, double *__restrict__ row_sigma) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_nodes) return;
    const ulonglong2 key = keys[e];
    const int slot = fw_claim(tab, mask, key.x, key.y, cnt);
    double R[4], sigma[4];
    fm_row(tab[slot >= 0 ? slot : 0].regret, slot, R);
    scopa::mc_sigma(R, n, sigma);
    row_slot[e] = slot;
#pragma unroll
    for (int a = 0; a < 3; a++) row_sigma[(size_t)e * 3 + a] = sigma[a];
}

// the step behind choice level k: the mover's card of slot a and, behind a round's last choice level, the two one-card plies
__device__ __forceinline__ void frn_play(scopa_full_state &s, const uint8_t *__restrict__ deck, int k, int a) {
    int cards[3];
    sorted_hand(s, k & 1, cards);
    step(s, deck, card_at(cards, a));
    if ((k & 3) == 3) {                                           // the one-card plies: player 0's last card, then player 1's
        step(s, deck, hand_get(s, 0, 0));
        step(s, deck, hand_get(s, 1, 0));
    }
}

// what a child leaves behind: its state and its mover's key pair, or -- below the last level -- the leaf's value 0.5 r2_p0, negated for responder 1
__device__ __forceinline__ void frn_child(const scopa_full_state &s, int k, int responder, int leaf, size_t c, scopa_full_state *__restrict__ child,
                                          ulonglong2 *__restrict__ keys, double *__restrict__ val) {
    if (leaf) {
        const double v = 0.5 * (double)s.r2_p0;
        val[c] = responder ? -v : v;
        return;
    }
    child[c] = s;
    const WideKey key = wide_key(s, (k + 1) & 1);
    keys[c] = make_ulonglong2(key.a, key.b);
}

// a responder level going down, a lane per child: child a of node e is element e n + a
__global__ void __launch_bounds__(256)
k_frn_expand(const scopa_full_state *__restrict__ parent, const uint8_t *__restrict__ decks, const int32_t *__restrict__ list, long long g0, int nb, uint32_t n_child,
             uint32_t Wc, int k, int n, int responder, int leaf, scopa_full_state *__restrict__ child, ulonglong2 *__restrict__ keys, double *__restrict__ val) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_child) return;
    const uint32_t t = c / Wc, e = c / (uint32_t)n;
    const int a = (int)(c - e * (uint32_t)n);
    const uint8_t *deck = decks + 40u * fsf_deck(list, g0 + t, nb);
    scopa_full_state s = parent[e];
    frn_play(s, deck, k, a);
    frn_child(s, k, responder, leaf, c, child, keys, val);
}

// the other player's level, a lane per node (t, p): the nets' average row under the match's rule (pol NULL: no snapshots, uniform play), the walk's draw
// (state.step << 16 | p, b0 + i, iteration, deck_index << 8 | 144 + responder), fm_pick, the step; the child keeps p.  Nothing of the store is touched
__global__ void __launch_bounds__(256)
k_frn_step(const scopa_full_state *__restrict__ parent, const double *__restrict__ pol, const uint8_t *__restrict__ decks, const int32_t *__restrict__ list, long long g0,
           int nb, uint32_t n_nodes, uint32_t W, int k, int n, int responder, int leaf, const FrnDraw D, uint32_t b0, scopa_full_state *__restrict__ child,
           ulonglong2 *__restrict__ keys, double *__restrict__ val) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_nodes) return;
    const uint32_t t = e / W, p = e - t * W;
    const long long g = g0 + t;
    const uint32_t deck_id = fsf_deck(list, g, nb);
    const uint32_t trav_id = b0 + (uint32_t)(g % nb);
    scopa_full_state s = parent[e];
    double prob[3];
    fw_uniform_probs(n, prob);
    if (pol) {
        double S[3];
#pragma unroll
        for (int c = 0; c < 3; c++) S[c] = pol[(size_t)e * 3 + c];
        fw_row_probs(S, n, prob);
    }
    const int a = fm_pick(prob, n, fm_draw(D, (deck_id << 8) | (kRespondTag + (uint32_t)responder), trav_id, s, p));
    frn_play(s, decks + 40u * deck_id, k, a);
    frn_child(s, k, responder, leaf, e, child, keys, val);
}

// a responder level going up, a lane per row: v = sum of sigma[a] cfv[a] in slot order from 0.0, d_regret[a] += cfv[a] - v and count += 1 by the walk's
// atomics (a dropped row adds nothing), v handed up.  add_choice / add_term: the launch's visit counts, added once (the responder's first level)
__global__ void __launch_bounds__(256)
k_frn_up(const int32_t *__restrict__ row_slot, const double *__restrict__ row_sigma, const double *__restrict__ val_in, double *__restrict__ val_out, uint32_t n_rows,
         int n, FwSlot *__restrict__ tab, unsigned long long *__restrict__ cnt, unsigned long long add_choice, unsigned long long add_term) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_rows) return;
    const int slot = row_slot[e];
    double sigma[3], cfv[3], v = 0.0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        sigma[a] = row_sigma[(size_t)e * 3 + a];
        cfv[a] = a < n ? val_in[(size_t)e * (size_t)n + a] : 0.0;
    }
#pragma unroll
    for (int a = 0; a < 3; a++) if (a < n) v += sigma[a] * cfv[a];
    if (slot >= 0) {
#pragma unroll
        for (int a = 0; a < 3; a++) if (a < n) atomicAdd(&tab[slot].d_regret[a], cfv[a] - v);
        atomicAdd(&tab[slot].count, 1u);
    }
    val_out[e] = v;
    if (e == 0u && (add_choice | add_term)) {
        atomicAdd(cnt + kCntChoice, add_choice);
        atomicAdd(cnt + kCntTerminal, add_term);
    }
}

// the geometry of a response call: the levels' widths for `responder`, the ranks of its levels, the visits of one traversal and the chunk the budget allows
struct FrnPlan {
    int L, rows, rank0[kFsfMaxLevels];
    uint32_t width[kFsfMaxLevels + 1];
    size_t paths, per_trav;
    unsigned long long choice, term;
};

FrnPlan frn_plan(int R, int responder) {
    FrnPlan p;
    p.L = 4 * R;
    p.rows = 0; p.choice = 0;
    uint32_t w = 1;
    for (int k = 0; k < p.L; k++) {
        p.width[k] = w;
        p.rank0[k] = p.rows;
        p.choice += w;
        if ((k & 1) == responder) { p.rows += (int)w; w *= (uint32_t)cards_of(k); }
    }
    p.width[p.L] = w;
    p.term = w;
    p.paths = w;                                                           // 6^R: no level is wider than the leaves
    p.per_trav = p.paths * kFrnPerPath + (size_t)p.rows * kFrnPerRow;
    return p;
}

const char *kFrnFull = "scopa_full_chance_respond_nets: the responder's store is full along a probe (updates dropped): create a larger one and tables_set";

// what both response entry points ask of a call before anything is launched: the root, the decks below it, the responder-free arguments
int32_t frn_check(scopa_full_chance *h, const char *who, const scopa_full_state *root_state, uint32_t nb, const int32_t *h_lists, uint32_t n_lists, int32_t *m,
                  uint32_t b0, const scopa_full_sdcfr_snapshots *const *sets, int n_sets, scopa_full_state *root_out) {
    scopa_full_state root = root_state ? *root_state : h->root;
    if (!root_ok(root)) return refuse(h, who, "the root must be a non-terminal state at a round boundary (step % 6 == 0)");
    root.game = 0u;
    if (root_state)
        for (int32_t d = 0; d < h->n_decks; d++)
            if (!deck_fits(h->decks + 40 * (size_t)d, root)) return refuse(h, who, "a deck of the handle does not pass create's check against the root of the call");
    if (!(nb >= 1 && nb <= (1u << 24) && (uint64_t)b0 + nb <= (1ull << 32))) return refuse(h, who, "nb outside [1, 1 << 24] or traversal ids b0 + nb exceed 2^32");
    if (!h_lists) *m = h->n_decks;
    if (!(*m >= 0 && *m <= h->n_decks)) return refuse(h, who, "a list holds 0 .. n decks");
    if (h_lists)
        for (uint32_t t = 0; t < n_lists; t++)
            if (!list_ok(h->n_decks, *m, h_lists + (size_t)t * (size_t)*m)) return refuse(h, who, "a listed deck out of range or listed twice");
    if ((uint64_t)*m * nb > (1ull << 30)) return refuse(h, who, "listed decks x nb above 1 << 30");
    for (int q = 0; q < n_sets; q++) {
        if (!sets[q]) return refuse(h, who, "a NULL snapshot set");
        const float *const w[6] = {sets[q]->d_w1, sets[q]->d_b1, sets[q]->d_w2, sets[q]->d_b2, sets[q]->d_w3, sets[q]->d_b3};
        if (!snaps_ok(sets[q]->n_snap, sets[q]->max_size, w, sets[q]->h_slots, sets[q]->d_coef))
            return refuse(h, who, "a snapshot set needs 0 <= n_snap <= max_size, and with snapshots six 4-byte aligned tensors, slots in [0, max_size) and coefficients");
    }
    *root_out = root;
    return SCOPA_OK;
}

// the scratch of a response call: the slot lists of `sets` in the block's head, behind them room for the chunk the budget allows -> the chunk, the
// snapshot sets as the kernels take them and the start of the chunk's part
int32_t frn_scratch(scopa_full_chance *h, const char *who, const FrnPlan &P, long long total, const scopa_full_sdcfr_snapshots *const *sets, int n_sets, FsdSnaps *snaps,
                    long long *chunk_out, char **at_out) {
    scopa_ctx *ctx = h->ctx;
    const size_t budget = ctx->full_sdcfr_scratch > 0 ? (size_t)ctx->full_sdcfr_scratch : (size_t)1 << 30;
    long long chunk = (long long)std::min<size_t>(budget / P.per_trav, ((size_t)1 << 28) / P.paths);
    if (chunk < 1) return refuse(h, who, "the scratch budget is too small for one traversal");
    chunk = std::min(chunk, total);
    size_t slot_off[3] = {0, 0, 0};
    for (int q = 0; q < n_sets; q++) slot_off[q + 1] = slot_off[q] + (((size_t)sets[q]->n_snap * 4 + 15) & ~(size_t)15);
    const size_t head = std::max<size_t>(slot_off[n_sets], 16);
    SC_HIP(ctx, hipSetDevice(ctx->device));
    if (int32_t rc = ensure_frontier_scratch(h, head + (size_t)chunk * P.per_trav)) return rc;
    char *at = (char *)h->sd->d_scratch;
    for (int q = 0; q < n_sets; q++) {
        snaps[q] = FsdSnaps{sets[q]->d_w1, sets[q]->d_b1, sets[q]->d_w2, sets[q]->d_b2, sets[q]->d_w3, sets[q]->d_b3, (const int32_t *)(at + slot_off[q]), sets[q]->d_coef, (int)sets[q]->n_snap};
        if (sets[q]->n_snap)   // (pageable: staged before the call returns)
            SC_HIP(ctx, hipMemcpyAsync(at + slot_off[q], sets[q]->h_slots, (size_t)sets[q]->n_snap * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    *chunk_out = chunk;
    *at_out = at + head;
    return SCOPA_OK;
}

// one response traversal call's launches: `nb` traversals of `responder` on each of the m listed decks against the other player's snapshots S
int32_t frn_launch(scopa_full_chance *h, const scopa_full_state &root, int responder, int nb, const int32_t *d_list, int m, const FsdSnaps &S, const FrnPlan &P,
                   long long chunk, char *at, uint32_t iteration, uint32_t b0) {
    scopa_ctx *ctx = h->ctx;
    hipStream_t st = ctx->stream;
    const long long total = (long long)m * nb;
    const size_t CP = (size_t)chunk * P.paths, CR = (size_t)chunk * (size_t)P.rows;
    scopa_full_state *d_state[2];
    d_state[0] = (scopa_full_state *)at; at += CP * sizeof(scopa_full_state);
    d_state[1] = (scopa_full_state *)at; at += CP * sizeof(scopa_full_state);
    ulonglong2 *d_keys = (ulonglong2 *)at; at += CP * 16;
    double *d_pol = (double *)at; at += CP * 24;
    double *d_val[2];
    d_val[0] = (double *)at; at += CP * 8;
    d_val[1] = (double *)at; at += CP * 8;
    double *d_sigma = (double *)at; at += CR * 24;
    int32_t *d_slot = (int32_t *)at;
    const uint32_t mask = (1u << h->capacity_log2) - 1u;
    const FrnDraw D{iteration, (uint32_t)ctx->seed, (uint32_t)(ctx->seed >> 32)};
    for (long long g0 = 0; g0 < total; g0 += chunk) {
        const uint32_t C = (uint32_t)std::min(chunk, total - g0);
        hipLaunchKernelGGL(k_fsf_roots, grid_of(C), dim3(256), 0, st, root, (const uint8_t *)h->d_decks, d_list, g0, C, nb, d_state[0], d_keys);
        for (int k = 0; k < P.L; k++) {
            const int n = cards_of(k), leaf = k + 1 == P.L;
            const uint32_t nodes = C * P.width[k];
            const scopa_full_state *parent = d_state[k & 1];
            scopa_full_state *child = d_state[(k + 1) & 1];
            if ((k & 1) == responder) {
                const size_t r0 = (size_t)C * (size_t)P.rank0[k];             // the rows of a level live level-major: row (t, p) of level k is element C rank0[k] + t W_k + p
                hipLaunchKernelGGL(k_frn_claim, grid_of(nodes), dim3(256), 0, st, (const ulonglong2 *)d_keys, nodes, n, h->d_tab, mask, h->d_cnt, d_slot + r0, d_sigma + 3 * r0);
                const uint32_t n_child = C * P.width[k + 1];
                hipLaunchKernelGGL(k_frn_expand, grid_of(n_child), dim3(256), 0, st, parent, (const uint8_t *)h->d_decks, d_list, g0, nb, n_child, P.width[k + 1], k, n, responder,
                                   leaf, child, d_keys, d_val[0]);
            } else {
                if (S.n_snap) launch_average_at(ctx, d_keys, (long long)nodes, S, d_pol);
                hipLaunchKernelGGL(k_frn_step, grid_of(nodes), dim3(256), 0, st, parent, S.n_snap ? (const double *)d_pol : (const double *)nullptr, (const uint8_t *)h->d_decks,
                                   d_list, g0, nb, nodes, P.width[k], k, n, responder, leaf, D, b0, child, d_keys, d_val[0]);
            }
        }
        int cur = 0;
        for (int k = P.L - 1; k >= 0; k--) {
            if ((k & 1) != responder) continue;
            const size_t r0 = (size_t)C * (size_t)P.rank0[k];
            const uint32_t n_rows = C * P.width[k];
            const bool first = P.width[k] == 1;                               // the responder's first level: the launch's visits are added here, once per chunk
            hipLaunchKernelGGL(k_frn_up, grid_of(n_rows), dim3(256), 0, st, (const int32_t *)(d_slot + r0), (const double *)(d_sigma + 3 * r0), (const double *)d_val[cur],
                               d_val[cur ^ 1], n_rows, cards_of(k), h->d_tab, h->d_cnt, first ? (unsigned long long)C * P.choice : 0ull,
                               first ? (unsigned long long)C * P.term : 0ull);
            cur ^= 1;
        }
        SC_HIP(ctx, hipGetLastError());
    }
    return SCOPA_OK;
}

}  // namespace

extern "C" {

int32_t scopa_full_chance_sdcfr_policy_at(scopa_ctx *ctx, int32_t player, const uint64_t *d_keys2, int64_t n, const float *d_w1, const float *d_b1, const float *d_w2,
                                          const float *d_b2, const float *d_w3, const float *d_b3, float *d_policy, uint64_t *d_thr) {
    if (!ctx) return SCOPA_EINVAL;
    SC_REQUIRE(ctx, player == 0 || player == 1, SCOPA_EINVAL, "scopa_full_chance_sdcfr_policy_at: player must be 0 or 1");
    SC_REQUIRE(ctx, n >= 0 && n <= ((int64_t)1 << 28), SCOPA_EINVAL, "scopa_full_chance_sdcfr_policy_at: n outside [0, 1 << 28]");
    if (n == 0) return SCOPA_OK;
    SC_REQUIRE(ctx, d_keys2 && d_w1 && d_b1 && d_w2 && d_b2 && d_w3 && d_b3 && d_policy && d_thr, SCOPA_EINVAL, "scopa_full_chance_sdcfr_policy_at: NULL device pointer");
    const uintptr_t any = (uintptr_t)d_w1 | (uintptr_t)d_b1 | (uintptr_t)d_w2 | (uintptr_t)d_b2 | (uintptr_t)d_w3 | (uintptr_t)d_b3 | (uintptr_t)d_policy;
    SC_REQUIRE(ctx, (any & 3) == 0 && ((uintptr_t)d_keys2 & 15) == 0 && ((uintptr_t)d_thr & 7) == 0, SCOPA_EINVAL,
               "scopa_full_chance_sdcfr_policy_at: the key pairs must be 16-byte aligned, the thresholds 8-byte, the weights and the policy 4-byte");
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t p = (size_t)player;
    const FsdNet net{d_w1 + p * kFsdH1 * kFsdIn, d_b1 + p * kFsdH1, d_w2 + p * kFsdH2 * kFsdH1, d_b2 + p * kFsdH2, d_w3 + p * kFsdOut * kFsdH2, d_b3 + p * kFsdOut};
    launch_policy_at(ctx, (const ulonglong2 *)d_keys2, n, net, d_policy, (unsigned long long *)d_thr);
    SC_HIP(ctx, hipGetLastError());
    return SCOPA_OK;
}

int32_t scopa_full_chance_debug_sdcfr_scratch(scopa_ctx *ctx, int64_t bytes) {
    if (!ctx || bytes < 0) return SCOPA_EINVAL;
    ctx->full_sdcfr_scratch = bytes;
    return SCOPA_OK;
}

int32_t scopa_full_chance_sdcfr_traverse_frontier(scopa_full_chance *h, const scopa_full_state *root_state, int32_t traverser, int32_t batch, int32_t m_list,
                                                  const int32_t *h_list, const float *d_w1, const float *d_b1, const float *d_w2, const float *d_b2, const float *d_w3,
                                                  const float *d_b3, float *d_mem_feat, float *d_mem_regret, int64_t capacity, int64_t write_base, float *d_root_values,
                                                  uint32_t iteration, uint32_t b0) {
    if (!h) return SCOPA_EINVAL;
    scopa_ctx *ctx = h->ctx;
    scopa_full_state root;
    int R = 0, m = 0;
    if (int32_t rc = check_traverse(h, root_state, true, traverser, batch, m_list, h_list, d_w1, d_b1, d_w2, d_b2, d_w3, d_b3, d_mem_feat, d_mem_regret, capacity, write_base,
                                    d_root_values, b0, &root, &R, &m))
        return rc;
    // the widths of the levels, the ranks of the traverser's, and the chunk the byte budget allows
    const int L = 4 * R;
    uint32_t width[kFsfMaxLevels + 1];
    int rank0[kFsfMaxLevels];
    uint32_t w = 1;
    int rows = 0;
    for (int k = 0; k < L; k++) {
        width[k] = w;
        rank0[k] = rows;
        if ((k & 1) == traverser) { rows += (int)w; w *= (uint32_t)cards_of(k); }
    }
    width[L] = w;
    const size_t paths = width[L] > width[L - 1] ? width[L] : width[L - 1];   // 6^R
    const size_t per_trav = paths * kFsfPerPath + (size_t)rows * kFsfPerRow;
    const size_t budget = ctx->full_sdcfr_scratch > 0 ? (size_t)ctx->full_sdcfr_scratch : (size_t)1 << 30;
    const long long total = (long long)m * batch;
    long long chunk = (long long)std::min<size_t>(budget / per_trav, ((size_t)1 << 28) / paths);
    SC_REQUIRE(ctx, chunk >= 1, SCOPA_EINVAL, "scopa_full_chance_sdcfr_traverse_frontier: the scratch budget is too small for one traversal");
    chunk = std::min(chunk, total);
    SC_HIP(ctx, hipSetDevice(ctx->device));
    if (int32_t rc = ensure_frontier_scratch(h, (size_t)chunk * per_trav)) return rc;
    FwSdcfr *c = h->sd;
    hipStream_t st = ctx->stream;
    if (h_list) SC_HIP(ctx, hipMemcpyAsync(c->d_list, h_list, (size_t)m * 4, hipMemcpyHostToDevice, st));   // (pageable: the copy is staged before the call returns)
    const int32_t *d_list = h_list ? c->d_list : nullptr;
    // the block, cut for `chunk` traversals: the pieces read 16 bytes at a time first
    const size_t CP = (size_t)chunk * paths, CR = (size_t)chunk * (size_t)rows;
    char *at = (char *)c->d_scratch;
    scopa_full_state *d_state[2];
    d_state[0] = (scopa_full_state *)at; at += CP * sizeof(scopa_full_state);
    d_state[1] = (scopa_full_state *)at; at += CP * sizeof(scopa_full_state);
    ulonglong2 *d_keys = (ulonglong2 *)at; at += CP * 16;
    unsigned long long *d_thr = (unsigned long long *)at; at += CP * 16;
    ulonglong2 *d_row_keys = (ulonglong2 *)at; at += CR * 16;
    float *d_pol = (float *)at; at += CP * 12;
    float *d_row_pol = (float *)at; at += CR * 12;
    float *d_val[2];
    d_val[0] = (float *)at; at += CP * 4;
    d_val[1] = (float *)at;
    const FsdNet net[2] = {{d_w1, d_b1, d_w2, d_b2, d_w3, d_b3},
                           {d_w1 + kFsdH1 * kFsdIn, d_b1 + kFsdH1, d_w2 + kFsdH2 * kFsdH1, d_b2 + kFsdH2, d_w3 + kFsdOut * kFsdH2, d_b3 + kFsdOut}};
    const uint32_t seed_lo = (uint32_t)ctx->seed, seed_hi = (uint32_t)(ctx->seed >> 32);
    const auto expand = traverser == 0 ? k_fsf_expand<0> : k_fsf_expand<1>;
    for (long long g0 = 0; g0 < total; g0 += chunk) {
        const uint32_t C = (uint32_t)std::min(chunk, total - g0);
        // the keys of a traverser level live with the rows, level-major: row (t, f) of level k is element C rank0[k] + t W_k + f
        auto keys_of = [&](int k) { return (k & 1) == traverser ? d_row_keys + (size_t)C * (size_t)rank0[k] : d_keys; };
        hipLaunchKernelGGL(k_fsf_roots, grid_of(C), dim3(256), 0, st, root, (const uint8_t *)h->d_decks, d_list, g0, C, (int)batch, d_state[0], keys_of(0));
        for (int k = 0; k < L; k++) {
            const int trav = (k & 1) == traverser, leaf = k + 1 == L;
            const long long nodes = (long long)C * width[k];
            launch_policy_at(ctx, keys_of(k), nodes, net[k & 1], trav ? d_row_pol + 3 * (size_t)C * (size_t)rank0[k] : d_pol, d_thr);
            const uint32_t n_child = C * width[k + 1];
            hipLaunchKernelGGL(expand, grid_of(n_child), dim3(256), 0, st, (const scopa_full_state *)d_state[k & 1], (const unsigned long long *)d_thr,
                               (const uint8_t *)h->d_decks, d_list, g0, (int)batch, n_child, width[k], k, cards_of(k), trav, leaf, seed_lo, seed_hi, iteration, b0,
                               d_state[(k + 1) & 1], leaf ? (ulonglong2 *)nullptr : keys_of(k + 1), d_val[0]);
        }
        int cur = 0;
        for (int k = L - 1; k >= 0; k--) {
            if ((k & 1) != traverser) continue;
            const long long elems = (long long)C * width[k] * 34;
            float *out = width[k] == 1 ? d_root_values + g0 : d_val[cur ^ 1];   // the traverser's first level: the root's value
            hipLaunchKernelGGL(k_fsf_up, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, st, (const ulonglong2 *)(d_row_keys + (size_t)C * (size_t)rank0[k]),
                               (const float *)(d_row_pol + 3 * (size_t)C * (size_t)rank0[k]), (const float *)d_val[cur], out, elems, width[k], cards_of(k), rank0[k], rows, g0,
                               (unsigned long long)write_base, (uint32_t)capacity, d_mem_feat, d_mem_regret);
            cur ^= 1;
        }
        SC_HIP(ctx, hipGetLastError());
    }
    c->visits += (uint64_t)total * (uint64_t)(traverser == 0 ? 13 : 8) * (uint64_t)(rows / 4);
    return SCOPA_OK;
}


int32_t scopa_full_chance_sdcfr_features(const uint64_t *keys2, int64_t n, float *feat) {
    if (n < 0 || (n > 0 && (!keys2 || !feat))) return SCOPA_EINVAL;
    for (int64_t i = 0; i < n; i++)
        for (int f = 0; f < kFsdIn; f++) feat[i * kFsdIn + f] = fsd_feature(keys2[2 * i], keys2[2 * i + 1], f);
    return SCOPA_OK;
}

int32_t scopa_full_chance_sdcfr_traverse(scopa_full_chance *h, const scopa_full_state *root_state, int32_t traverser, int32_t batch, int32_t m_list, const int32_t *h_list,
                                         const float *d_w1, const float *d_b1, const float *d_w2, const float *d_b2, const float *d_w3, const float *d_b3,
                                         float *d_mem_feat, float *d_mem_regret, int64_t capacity, int64_t write_base, float *d_root_values, uint32_t iteration, uint32_t b0) {
    if (!h) return SCOPA_EINVAL;
    scopa_ctx *ctx = h->ctx;
    scopa_full_state root;
    int R = 0, m = 0;
    if (int32_t rc = check_traverse(h, root_state, false, traverser, batch, m_list, h_list, d_w1, d_b1, d_w2, d_b2, d_w3, d_b3, d_mem_feat, d_mem_regret, capacity, write_base,
                                    d_root_values, b0, &root, &R, &m))
        return rc;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    if (int32_t rc = ensure_handle_forest(h, root, R)) return rc;
    FwSdcfr *c = h->sd;
    hipStream_t st = ctx->stream;
    if (h_list) SC_HIP(ctx, hipMemcpyAsync(c->d_list, h_list, (size_t)m * 4, hipMemcpyHostToDevice, st));   // (pageable: the copy is staged before the call returns)
    const int32_t *d_list = h_list ? c->d_list : nullptr;
    const FsdNet net0{d_w1, d_b1, d_w2, d_b2, d_w3, d_b3};
    const FsdNet net1{d_w1 + kFsdH1 * kFsdIn, d_b1 + kFsdH1, d_w2 + kFsdH2 * kFsdH1, d_b2 + kFsdH2, d_w3 + kFsdOut * kFsdH2, d_b3 + kFsdOut};
    const int launches = ctx->full_sdcfr_launches;   // benchmark hook: 1 = the policy launch alone, 2 = the walk launch alone over the tables as they are
    SC_REQUIRE(ctx, launches != 2 || c->called, SCOPA_ESTATE, "scopa_full_chance_sdcfr_traverse: the walk launch alone needs the tables of an earlier call on this forest");
    if (launches != 2)
        if (int32_t rc = launch_policy(ctx, c->f, d_list, m, 3, net0, net1, 0, c->d_pol, c->d_thr, nullptr)) return rc;
    c->called = true;
    if (launches == 1) return SCOPA_OK;
    {   // about four workgroups per compute unit over all slots, at least one per slot, none without a traversal
        int wg_per_slot = (4 * ctx->n_cus + m - 1) / m;
        wg_per_slot = wg_per_slot < 1 ? 1 : wg_per_slot > batch ? batch : wg_per_slot;
        const FsdWalkArgs wa = walk_args_of(c->f.s, traverser);
        const auto walk = traverser == 0 ? k_full_chance_sdcfr_walk<0> : k_full_chance_sdcfr_walk<1>;
        hipLaunchKernelGGL(walk, dim3((unsigned)m * (unsigned)wg_per_slot), dim3(kFsdWalkThreads), 0, st, (const ulonglong2 *)c->f.d_keys, (const float *)c->f.d_leaf, d_list,
                           (const float *)c->d_pol, (const unsigned long long *)c->d_thr, wa, (int)batch, wg_per_slot, d_mem_feat, d_mem_regret, (uint32_t)capacity,
                           (unsigned long long)write_base, d_root_values, (uint32_t)ctx->seed, (uint32_t)(ctx->seed >> 32), iteration, b0);
        SC_HIP(ctx, hipGetLastError());
    }
    int64_t S = 0, p6 = 1;
    for (int r = 0; r < R; r++) { S += p6; p6 *= 6; }
    c->visits += (uint64_t)m * (uint64_t)batch * (uint64_t)(traverser == 0 ? 13 : 8) * (uint64_t)S;
    c->called = true;
    return SCOPA_OK;
}

int32_t scopa_full_chance_debug_sdcfr(scopa_ctx *ctx, int32_t launches) {
    if (!ctx || launches < 0 || launches > 2) return SCOPA_EINVAL;
    ctx->full_sdcfr_launches = launches;
    return SCOPA_OK;
}

int32_t scopa_full_chance_sdcfr_visits(scopa_full_chance *h, uint64_t *choice_visits) {
    if (!h || !choice_visits) return SCOPA_EINVAL;
    *choice_visits = h->sd ? h->sd->visits : 0;   // counted on the host from the traversal's fixed shape: no wait for the stream
    return SCOPA_OK;
}

int32_t scopa_full_chance_sdcfr_policy_get(scopa_full_chance *h, int64_t *n_nodes, float *h_policy, uint64_t *h_thr, uint64_t *h_keys2) {
    if (!h || !n_nodes) return SCOPA_EINVAL;
    scopa_ctx *ctx = h->ctx;
    SC_REQUIRE(ctx, h->sd && h->sd->built && h->sd->called, SCOPA_ESTATE, "scopa_full_chance_sdcfr_policy_get: no traversal call on the forest at hand yet");
    FwSdcfr *c = h->sd;
    const int64_t T = (int64_t)c->f.s.off[c->f.s.L], room = *n_nodes;
    *n_nodes = T;
    if (!h_policy && !h_thr && !h_keys2) return SCOPA_OK;
    SC_REQUIRE(ctx, room >= T, SCOPA_EINVAL, "scopa_full_chance_sdcfr_policy_get: less room than nodes");
    SC_HIP(ctx, hipSetDevice(ctx->device));
    if (h_policy) SC_HIP(ctx, hipMemcpyAsync(h_policy, c->d_pol, (size_t)T * 12, hipMemcpyDeviceToHost, ctx->stream));
    if (h_thr) SC_HIP(ctx, hipMemcpyAsync(h_thr, c->d_thr, (size_t)T * 16, hipMemcpyDeviceToHost, ctx->stream));
    if (h_keys2) SC_HIP(ctx, hipMemcpyAsync(h_keys2, c->f.d_keys, (size_t)T * 16, hipMemcpyDeviceToHost, ctx->stream));
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SCOPA_OK;
}

int32_t scopa_full_chance_sdcfr_average_policy(scopa_full_chance *h, const scopa_full_state *root_state, const uint8_t *h_decks, int32_t k, int32_t player, int32_t n_snap,
                                               const float *d_w1, const float *d_b1, const float *d_w2, const float *d_b2, const float *d_w3, const float *d_b3,
                                               const int32_t *h_slots, int32_t max_size, const float *d_coef, int64_t *n_rows, uint64_t *h_keys2, double *h_policy) {
    if (!h) return SCOPA_EINVAL;
    scopa_ctx *ctx = h->ctx;
    SC_REQUIRE(ctx, n_rows && (player == 0 || player == 1) && n_snap >= 0 && max_size >= 0 && n_snap <= max_size, SCOPA_EINVAL,
               "scopa_full_chance_sdcfr_average_policy: n_rows, player in {0, 1} and 0 <= n_snap <= max_size are required");
    SC_REQUIRE(ctx, !h_decks || k >= 1, SCOPA_EINVAL, "scopa_full_chance_sdcfr_average_policy: k < 1 with decks given");
    if (n_snap > 0) {
        SC_REQUIRE(ctx, d_w1 && d_b1 && d_w2 && d_b2 && d_w3 && d_b3 && h_slots && d_coef, SCOPA_EINVAL, "scopa_full_chance_sdcfr_average_policy: NULL pointer");
        for (int32_t s = 0; s < n_snap; s++)
            SC_REQUIRE(ctx, h_slots[s] >= 0 && h_slots[s] < max_size, SCOPA_EINVAL, "scopa_full_chance_sdcfr_average_policy: a snapshot slot outside [0, max_size)");
    }
    scopa_full_state root = root_state ? *root_state : h->root;
    const int n = h_decks ? k : h->n_decks;
    int R = 0;
    if (int32_t rc = check_root(ctx, root, (uint64_t)n, &R)) return rc;
    root.game = 0u;
    const uint8_t *decks = h_decks ? h_decks : h->decks;
    for (int32_t d = 0; d < n; d++)
        SC_REQUIRE(ctx, deck_fits(decks + 40 * (size_t)d, root), SCOPA_EINVAL, "scopa_full_chance_sdcfr_average_policy: a deck does not pass create's check against the root of the call");
    const Shape s = shape_of(R, (uint32_t)n);
    int64_t N = 0;
    for (int lv = player; lv < s.L; lv += 2) N += s.size[lv];
    const int64_t room = *n_rows;
    *n_rows = N;
    if (!h_keys2 && !h_policy) return SCOPA_OK;
    SC_REQUIRE(ctx, room >= N, SCOPA_EINVAL, "scopa_full_chance_sdcfr_average_policy: less room than rows");
    SC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    FsdForest tmp;
    uint8_t *d_decks = nullptr;
    const FsdForest *f = nullptr;
    if (h_decks) {   // held-out decks: a forest of the call's own
        if (hipMalloc((void **)&d_decks, 40 * (size_t)n) != hipSuccess) return fail(ctx, SCOPA_ENOMEM, "scopa_full_chance_sdcfr_average_policy: no device memory for the decks");
        hipError_t e = hipMemcpyAsync(d_decks, h_decks, 40 * (size_t)n, hipMemcpyHostToDevice, st);
        int32_t rc = e == hipSuccess ? forest_build(ctx, root, d_decks, (uint32_t)n, R, tmp) : fail(ctx, SCOPA_EHIP, "scopa_full_chance_sdcfr_average_policy: decks", e);
        (void)hipFree(d_decks);   // (forest_build has synchronised)
        if (rc) return rc;
        f = &tmp;
    } else {
        if (int32_t rc = ensure_handle_forest(h, root, R)) return rc;
        f = &h->sd->f;
    }
    const size_t T = s.off[s.L];
    float *d_acc = nullptr;
    unsigned long long *d_ok = nullptr;
    double *d_op = nullptr;
    int32_t rc = SCOPA_OK;
    if (hipMalloc((void **)&d_acc, T * 12) != hipSuccess || hipMalloc((void **)&d_ok, (size_t)N * 16) != hipSuccess || hipMalloc((void **)&d_op, (size_t)N * 24) != hipSuccess)
        rc = fail(ctx, SCOPA_ENOMEM, "scopa_full_chance_sdcfr_average_policy: no device memory for the sums");
    hipError_t e = hipSuccess;
    if (!rc) e = hipMemsetAsync(d_acc, 0, T * 12, st);
    for (int32_t i = 0; i < n_snap && !rc && e == hipSuccess; i++) {   // FIFO order: acc += coef[i] * p_i
        const size_t sl = (size_t)h_slots[i];
        const FsdNet net{d_w1 + sl * kFsdH1 * kFsdIn, d_b1 + sl * kFsdH1, d_w2 + sl * kFsdH2 * kFsdH1, d_b2 + sl * kFsdH2, d_w3 + sl * kFsdOut * kFsdH2, d_b3 + sl * kFsdOut};
        rc = launch_policy(ctx, *f, nullptr, n, 1 << player, net, net, 1, d_acc, nullptr, d_coef + i);
    }
    if (!rc && e == hipSuccess) {
        int64_t at = 0;
        for (int lv = player; lv < s.L; lv += 2) {
            hipLaunchKernelGGL(k_fsd_normalise, grid_of(s.size[lv]), dim3(256), 0, st, (const ulonglong2 *)(f->d_keys + s.off[lv]), (const float *)(d_acc + 3 * s.off[lv]), s.size[lv],
                               cards_of(lv), d_ok + 2 * at, d_op + 3 * at);
            at += s.size[lv];
        }
        e = hipGetLastError();
        if (e == hipSuccess && h_keys2) e = hipMemcpyAsync(h_keys2, d_ok, (size_t)N * 16, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && h_policy) e = hipMemcpyAsync(h_policy, d_op, (size_t)N * 24, hipMemcpyDeviceToHost, st);
    }
    const hipError_t e2 = hipStreamSynchronize(st);
    if (d_acc) (void)hipFree(d_acc);
    if (d_ok) (void)hipFree(d_ok);
    if (d_op) (void)hipFree(d_op);
    forest_free(tmp);
    if (rc) return rc;
    SC_HIP(ctx, e);
    SC_HIP(ctx, e2);
    return SCOPA_OK;
}

int32_t scopa_full_chance_sdcfr_average_at(scopa_ctx *ctx, int32_t player, const uint64_t *d_keys2, int64_t n, int32_t n_snap, const float *d_w1, const float *d_b1,
                                           const float *d_w2, const float *d_b2, const float *d_w3, const float *d_b3, const int32_t *h_slots, int32_t max_size,
                                           const float *d_coef, double *d_policy) {
    if (!ctx) return SCOPA_EINVAL;
    SC_REQUIRE(ctx, player == 0 || player == 1, SCOPA_EINVAL, "scopa_full_chance_sdcfr_average_at: player must be 0 or 1");
    SC_REQUIRE(ctx, n >= 0 && n <= ((int64_t)1 << 28), SCOPA_EINVAL, "scopa_full_chance_sdcfr_average_at: n outside [0, 1 << 28]");
    const float *const w[6] = {d_w1, d_b1, d_w2, d_b2, d_w3, d_b3};
    SC_REQUIRE(ctx, snaps_ok(n_snap, max_size, w, h_slots, d_coef), SCOPA_EINVAL,
               "scopa_full_chance_sdcfr_average_at: 0 <= n_snap <= max_size, and with snapshots six 4-byte aligned tensors, slots in [0, max_size) and coefficients are required");
    if (n == 0) return SCOPA_OK;
    SC_REQUIRE(ctx, d_keys2 && d_policy && ((uintptr_t)d_keys2 & 15) == 0 && ((uintptr_t)d_policy & 7) == 0, SCOPA_EINVAL,
               "scopa_full_chance_sdcfr_average_at: the key pairs must be 16-byte aligned, the policy rows 8-byte, neither NULL");
    SC_HIP(ctx, hipSetDevice(ctx->device));
    if ((size_t)n_snap > ctx->full_avg_slots_n) {
        SC_HIP(ctx, hipStreamSynchronize(ctx->stream));   // an earlier call's launch may still read the old list
        if (ctx->d_full_avg_slots) (void)hipFree(ctx->d_full_avg_slots);
        ctx->d_full_avg_slots = nullptr; ctx->full_avg_slots_n = 0;
        const size_t room = std::max<size_t>(64, (size_t)n_snap);
        if (hipMalloc(&ctx->d_full_avg_slots, room * 4) != hipSuccess) return fail(ctx, SCOPA_ENOMEM, "scopa_full_chance_sdcfr_average_at: no device memory for the slot list");
        ctx->full_avg_slots_n = room;
    }
    if (n_snap) SC_HIP(ctx, hipMemcpyAsync(ctx->d_full_avg_slots, h_slots, (size_t)n_snap * 4, hipMemcpyHostToDevice, ctx->stream));   // (pageable: staged before the call returns)
    const FsdSnaps S{d_w1, d_b1, d_w2, d_b2, d_w3, d_b3, (const int32_t *)ctx->d_full_avg_slots, d_coef, (int)n_snap};
    launch_average_at(ctx, (const ulonglong2 *)d_keys2, n, S, d_policy);
    SC_HIP(ctx, hipGetLastError());
    return SCOPA_OK;
}

int32_t scopa_full_chance_sdcfr_match(scopa_full_chance *h, int64_t n_episodes, uint32_t stream_id, const uint8_t *h_decks, int32_t k,
                                      const scopa_full_sdcfr_snapshots *agent, scopa_full_chance *opp_store, const scopa_full_sdcfr_snapshots *opp_nets,
                                      int64_t h_sums[6], int8_t *h_r2_agent, int8_t *h_trace) {
    if (!h) return SCOPA_EINVAL;
    scopa_ctx *ctx = h->ctx;
    SC_REQUIRE(ctx, n_episodes >= 0 && n_episodes <= (1ll << 36) && h_sums && stream_id < (1u << 24), SCOPA_EINVAL,
               "scopa_full_chance_sdcfr_match: n_episodes outside [0, 1 << 36], stream_id at or above 1 << 24, or h_sums NULL");
    if (!h_decks) k = h->n_decks;
    SC_REQUIRE(ctx, k >= 1 && k <= (1 << 20), SCOPA_EINVAL, "scopa_full_chance_sdcfr_match: k outside [1, 1 << 20]");
    if (h_decks)
        for (int32_t d = 0; d < k; d++)
            SC_REQUIRE(ctx, deck_fits(h_decks + 40 * (size_t)d, h->root), SCOPA_EINVAL, "scopa_full_chance_sdcfr_match: a deck does not pass create's check against the handle's root");
    SC_REQUIRE(ctx, agent && !(opp_store && opp_nets), SCOPA_EINVAL, "scopa_full_chance_sdcfr_match: the agent's two snapshot sets are required; the opponent is a store OR a second pair of sets");
    SC_REQUIRE(ctx, !opp_store || opp_store->ctx == ctx, SCOPA_EINVAL, "scopa_full_chance_sdcfr_match: the opponent's store is of another context");
    const scopa_full_sdcfr_snapshots *sets[4] = {agent, agent + 1, opp_nets, opp_nets ? opp_nets + 1 : nullptr};
    size_t slot_off[5] = {0, 0, 0, 0, 0};
    for (int q = 0; q < 4; q++) {
        slot_off[q + 1] = slot_off[q];
        if (!sets[q]) continue;
        const float *const w[6] = {sets[q]->d_w1, sets[q]->d_b1, sets[q]->d_w2, sets[q]->d_b2, sets[q]->d_w3, sets[q]->d_b3};
        SC_REQUIRE(ctx, snaps_ok(sets[q]->n_snap, sets[q]->max_size, w, sets[q]->h_slots, sets[q]->d_coef), SCOPA_EINVAL,
                   "scopa_full_chance_sdcfr_match: a snapshot set needs 0 <= n_snap <= max_size, and with snapshots six 4-byte aligned tensors, slots in [0, max_size) and coefficients");
        slot_off[q + 1] += ((size_t)sets[q]->n_snap * 4 + 15) & ~(size_t)15;
    }
    SC_REQUIRE(ctx, (!h_r2_agent && !h_trace) || n_episodes <= (1ll << 31), SCOPA_EINVAL, "scopa_full_chance_sdcfr_match: per-episode output asked for more than 1 << 31 episodes");
    const size_t budget = ctx->full_sdcfr_scratch > 0 ? (size_t)ctx->full_sdcfr_scratch : (size_t)1 << 30;
    long long chunk = (long long)std::min<size_t>(budget / kFsmPerEpisode, (size_t)1 << 28);
    SC_REQUIRE(ctx, chunk >= 1, SCOPA_EINVAL, "scopa_full_chance_sdcfr_match: the scratch budget is too small for one episode");
    for (int i = 0; i < 6; i++) h_sums[i] = 0;
    if (!n_episodes) return SCOPA_OK;
    chunk = std::min<long long>(chunk, n_episodes);
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t deck_bytes = h_decks ? ((40 * (size_t)k + 24 + 15) & ~(size_t)15) : 0;   // held-out decks travel in the block's head, behind the slot lists
    const size_t head = std::max<size_t>(slot_off[4] + deck_bytes, 16);
    if (int32_t rc = ensure_frontier_scratch(h, head + (size_t)chunk * kFsmPerEpisode)) return rc;
    hipStream_t st = ctx->stream;
    // the block, cut for `chunk` episodes behind the slot lists and the decks
    char *at = (char *)h->sd->d_scratch;
    uint8_t *d_held = h_decks ? (uint8_t *)(at + slot_off[4]) : nullptr;
    FsdSnaps snaps[4];
    memset(snaps, 0, sizeof(snaps));
    hipError_t e = hipSuccess;
    for (int q = 0; q < 4 && e == hipSuccess; q++) {
        if (!sets[q]) continue;
        snaps[q] = FsdSnaps{sets[q]->d_w1, sets[q]->d_b1, sets[q]->d_w2, sets[q]->d_b2, sets[q]->d_w3, sets[q]->d_b3, (const int32_t *)(at + slot_off[q]), sets[q]->d_coef, (int)sets[q]->n_snap};
        if (sets[q]->n_snap) e = hipMemcpyAsync(at + slot_off[q], sets[q]->h_slots, (size_t)sets[q]->n_snap * 4, hipMemcpyHostToDevice, st);   // (pageable: staged before the call returns)
    }
    at += head;
    const size_t C0 = (size_t)chunk;
    scopa_full_state *d_state[2];
    d_state[0] = (scopa_full_state *)at; at += C0 * sizeof(scopa_full_state);
    d_state[1] = (scopa_full_state *)at; at += C0 * sizeof(scopa_full_state);
    ulonglong2 *d_keys = (ulonglong2 *)at; at += C0 * 16;
    double *d_pol = (double *)at; at += C0 * 24;
    int8_t *d_trace = (int8_t *)at; at += C0 * 24;
    int8_t *d_r2 = (int8_t *)at;
    long long *d_sums = match_sums(h->d_cnt);
    if (e == hipSuccess && d_held) e = hipMemcpyAsync(d_held, h_decks, 40 * (size_t)k, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(d_sums, 0, 8 * 8, st);
    const uint8_t *decks = d_held ? d_held : h->d_decks;
    const int R = 6 - (int)h->root.round, L = 4 * R, level0 = 4 * (int)h->root.round;
    const long long n = n_episodes, half = (n + 1) / 2;
    const uint32_t seed_lo = (uint32_t)ctx->seed, seed_hi = (uint32_t)(ctx->seed >> 32);
    const auto step_launch = opp_store ? k_fsm_step<true> : k_fsm_step<false>;
    const FwSlot *opp_tab = opp_store ? opp_store->d_tab : nullptr;
    const uint32_t opp_mask = opp_store ? (1u << opp_store->capacity_log2) - 1u : 0u;
    for (long long g0 = 0; g0 < n && e == hipSuccess; g0 += chunk) {
        const uint32_t C = (uint32_t)std::min(chunk, n - g0);
        const long long c0 = std::max<long long>(0, std::min<long long>(C, half - g0));   // the chunk's episodes [0, c0) sit in seat 0, [c0, C) in seat 1
        hipLaunchKernelGGL(k_fsm_roots, grid_of(C), dim3(256), 0, st, h->root, decks, (long long)k, g0, C, n, d_state[0], d_keys, h_trace ? d_trace : (int8_t *)nullptr);
        for (int lv = 0; lv < L; lv++) {
            const int p = lv & 1;
            const long long off[2] = {p ? c0 : 0, p ? 0 : c0}, cnt[2] = {p ? (long long)C - c0 : c0, p ? c0 : (long long)C - c0};   // [0]: the agent moves; [1]: the opponent
            if (cnt[0]) launch_average_at(ctx, d_keys + off[0], cnt[0], snaps[p], d_pol + 3 * off[0]);
            if (opp_nets && cnt[1]) launch_average_at(ctx, d_keys + off[1], cnt[1], snaps[2 + p], d_pol + 3 * off[1]);
            hipLaunchKernelGGL(step_launch, grid_of(C), dim3(256), 0, st, (const scopa_full_state *)d_state[lv & 1], (const double *)d_pol, opp_tab, opp_mask, opp_nets ? 1 : 0,
                               decks, (long long)k, g0, C, n, lv, level0, (int)(lv + 1 == L), stream_id, seed_lo, seed_hi, d_state[(lv + 1) & 1], d_keys,
                               h_trace ? d_trace : (int8_t *)nullptr, d_sums, h_r2_agent ? d_r2 : (int8_t *)nullptr);
        }
        e = hipGetLastError();
        if (e == hipSuccess && h_r2_agent) e = hipMemcpyAsync(h_r2_agent + g0, d_r2, (size_t)C, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && h_trace) e = hipMemcpyAsync(h_trace + (size_t)g0 * kFsfMaxLevels, d_trace, (size_t)C * kFsfMaxLevels, hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h_sums, d_sums, 6 * 8, hipMemcpyDeviceToHost, st);
    const hipError_t e2 = hipStreamSynchronize(st);
    SC_HIP(ctx, e);
    SC_HIP(ctx, e2);
    return SCOPA_OK;
}

int32_t scopa_full_chance_debug_sdcfr_average_grid(scopa_ctx *ctx, int32_t workgroups) {
    if (!ctx || workgroups < 0) return SCOPA_EINVAL;
    ctx->full_avg_grid = workgroups;
    return SCOPA_OK;
}

int32_t scopa_full_chance_respond_nets_traverse(scopa_full_chance *h_resp, const scopa_full_state *root_state, int32_t responder, uint32_t nb, const int32_t *h_list,
                                                int32_t m, const scopa_full_sdcfr_snapshots *opponent, uint32_t iteration, uint32_t b0) {
    if (!h_resp) return SCOPA_EINVAL;
    scopa_full_chance *h = h_resp;
    const char *who = "scopa_full_chance_respond_nets_traverse";
    if (responder != 0 && responder != 1) return refuse(h, who, "responder outside {0, 1}");
    scopa_full_state root;
    const scopa_full_sdcfr_snapshots *sets[1] = {opponent};
    if (int32_t rc = frn_check(h, who, root_state, nb, h_list, 1, &m, b0, sets, 1, &root)) return rc;
    if (!m) return SCOPA_OK;
    const FrnPlan P = frn_plan(6 - (int)root.round, responder);
    FsdSnaps S;
    long long chunk = 0;
    char *at = nullptr;
    if (int32_t rc = frn_scratch(h, who, P, (long long)m * nb, sets, 1, &S, &chunk, &at)) return rc;
    scopa_ctx *ctx = h->ctx;
    if (h_list) SC_HIP(ctx, hipMemcpyAsync(h->sd->d_list, h_list, (size_t)m * 4, hipMemcpyHostToDevice, ctx->stream));   // (pageable: the copy is staged before the call returns)
    const int32_t rc = frn_launch(h, root, responder, (int)nb, h_list ? h->sd->d_list : nullptr, m, S, P, chunk, at, iteration, b0);
    const int32_t rc2 = check_dropped(h, kFrnFull);
    return rc != SCOPA_OK ? rc : rc2;
}

int32_t scopa_full_chance_respond_nets_iterate(scopa_full_chance *h_resp, const scopa_full_sdcfr_snapshots *nets, uint32_t batch, uint32_t n_iters, const int32_t *h_lists,
                                               int32_t m) {
    if (!h_resp) return SCOPA_EINVAL;
    scopa_full_chance *h = h_resp;
    const char *who = "scopa_full_chance_respond_nets_iterate";
    if (!nets) return refuse(h, who, "the two snapshot sets, player 0's and player 1's, are required");
    if (n_iters > (1u << 20)) return refuse(h, who, "n_iters above 1 << 20");
    scopa_full_state root;
    const scopa_full_sdcfr_snapshots *sets[2] = {nets, nets + 1};
    if (int32_t rc = frn_check(h, who, nullptr, batch, h_lists, n_iters, &m, 0u, sets, 2, &root)) return rc;
    if (!n_iters) return SCOPA_OK;
    scopa_ctx *ctx = h->ctx;
    FsdSnaps S[2];
    long long chunk = 0;
    char *at = nullptr;
    const int R = 6 - (int)root.round;
    if (m)
        if (int32_t rc = frn_scratch(h, who, frn_plan(R, 0), (long long)m * batch, sets, 2, S, &chunk, &at)) return rc;   // (both responders' plans take the same bytes)
    SC_HIP(ctx, hipSetDevice(ctx->device));
    int32_t *d_lists = nullptr;
    const size_t bytes = 4 * (size_t)n_iters * (size_t)m;
    if (h_lists && bytes) {                                               // uploaded once per call
        hipError_t e;
        if ((e = hipMalloc((void **)&d_lists, bytes)) != hipSuccess) return refuse(h, who, "the deck lists", SCOPA_ENOMEM, e);
        if ((e = hipMemcpyAsync(d_lists, h_lists, bytes, hipMemcpyHostToDevice, ctx->stream)) != hipSuccess) {
            (void)hipFree(d_lists);
            return fail(ctx, SCOPA_EHIP, "hipMemcpyAsync(H2D)", e);
        }
    }
    int32_t rc = SCOPA_OK;
    for (uint32_t t = 0; t < n_iters && rc == SCOPA_OK; t++)
        for (int resp = 0; resp < 2 && rc == SCOPA_OK; resp++) {
            if (m) rc = frn_launch(h, root, resp, (int)batch, d_lists ? d_lists + (size_t)t * m : nullptr, m, S[1 - resp], frn_plan(R, resp), chunk, at, h->iteration, 0u);
            if (rc == SCOPA_OK) rc = scopa_full_chance_apply(h);
        }
    const int32_t rc2 = check_dropped(h, kFrnFull);                       // synchronises: the lists may go
    if (d_lists) (void)hipFree(d_lists);
    return rc != SCOPA_OK ? rc : rc2;
}

}  // extern "C"
