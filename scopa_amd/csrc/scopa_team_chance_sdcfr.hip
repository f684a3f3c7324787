// scopa_team_chance_sdcfr.hip -- Single Deep CFR's external-sampling traversal and average policy on Team MiniScopa over a set of deals
// (scopa_team_chance_sdcfr_*).
//
// Reference behaviour: DeepCFR._external_sampling_cfr (src/algorithms/deep_cfr/deep_cfr.py:284-365) on TPIMiniScopaGame
// (src/envs/openspiel_team_mini_scopa.py): the "player" is the TEAM of the seat to move, ply k is played by seat k & 3, seats 0, 1 are team 0.
// _state_to_features reads H[...] and T[...] of the information-state string and nothing of its A[...] history, so the 34 features of
// MiniScopa -- the mover's hand one-hot, the table multi-hot, [1, 0] -- and the 34-128-64-16 advantage net apply unchanged, one net per team, and
// a node's features are a function of the handle's key (depth, the seat's initial hand in hand order, the cards played so far).
//
// A traversal of traverser T: T's plies recurse into every legal card in hand order, the other team's plies sample one card, the terminal is
// worth 0.5 * r2 of T's team.  Depths 0..11 have 4,4,4,4,3,3,3,3,2,2,2,2 legal cards and depths 12..15 one.  EVERY node of T -- the forced ones
// too -- evaluates T's net, takes value = sum policy[a] * child value and appends a memory row after its children; at a forced node the policy
// of the one legal card is relu(adv) / max(relu(adv), 1e-8): 1 where the advantage is at least 1e-8, 0 where it is not positive -- the reference
// has no uniform fall-back on the traverser's side, so the forced nodes' nets are evaluated as well (two depths of 331 776 nodes per deal).
// Per traversal: 501 choice rows + 2 x 576 forced rows = kTsdRows = 1 653 memory rows (MiniScopa's 1 653 decision NODES are another number);
// non-terminal visits 4 277 (traverser 0) / 3 127 (traverser 1), of which 1 973 / 823 at choice nodes; 576 arrivals at depth 12.
//
// Two launches per call, no atomics, no host synchronisation:
//   k_team_chance_sdcfr_policy  the regret-matching policy [4] (float32, hand order) and sampling thresholds [3] (uint64, sd_thresholds of
//       scopa_sdcfr_tile.h) of all 321 365 choice rows of every listed deal, each under the net of the row's team, and the forced policy of the
//       traverser's 2 x 331 776 forced nodes.  A throughput kernel: the grid is cut by (slot, team, chunk); a workgroup of four wavefronts loads
//       its slices of ONE team's net into registers once (64 registers per lane) and loops over its chunk of that team's 16-node tiles, the
//       each tile being sd_tile_policy (scopa_sdcfr_tile.h), the one k_sdcfr_policy runs: the layers cut across the wavefronts and handed over
//       through LDS, one K order (constant feature folded into the layer-1 bias, layer 3 as two chains added at the end), so equal features give equal bits.
//   k_team_chance_sdcfr_walk    a workgroup per traversal: the frontier of every depth in LDS (node index within its level, 2 549 words at
//       most), opponent plies compare a Philox draw with the node's thresholds as 64-bit integers (the zero-sum case keeps numpy's uniform
//       arithmetic), values come back up in float32 in hand order through two 576-float buffers, and every level's rows leave through 32-byte
//       records in LDS in one sweep of consecutive addresses per row.  A workgroup serves one slot for the whole launch.
//       LDS: 10 196 + 4 608 + 18 432 = 33 236 bytes.  Philox counter (local row of the node, traversal id, iteration, 96 + traverser).
#include <algorithm>
#include <new>
#include <vector>

#include "scopa_kernels.h"
#include "scopa_philox.h"
#include "scopa_sdcfr_tile.h"
#include "scopa_team_chance.h"
#include "scopa_team_passes.h"

using scopa::fail;

namespace {

constexpr int kTsdRows = SCOPA_TEAM_SDCFR_ROWS;   // memory rows of one traversal, either traverser
constexpr uint32_t kTsdPhiloxTag = 96u;           // counter word 3 = 96 + traverser
constexpr int kTsdRing = 4;                       // pinned staging rows of the deal lists

// ---- node info ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t tsd_seat_hand(const uint32_t (&w)[10], uint32_t seat) { return (((seat & 2u) ? w[4] : w[3]) >> (16u * (seat & 1u))) & 0xFFFFu; }
__device__ __forceinline__ uint32_t tsd_table_bits(const uint32_t (&w)[10]) {
    const int nt = (int)(w[9] & 255u);
    uint32_t bits = 0;
    for (int k = 0; k < 8; k++) if (k < nt) bits |= 1u << scopa::nib(w[2], k);
    return bits;
}

// feature bits (hand one-hot | table multi-hot << 16) and the mover's remaining hand nibbles (hand order) of every choice row of every deal
__global__ void __launch_bounds__(256)
k_tsd_ninfo(const scopa_team_state *__restrict__ g_roots, uint2 *__restrict__ g_ninfo, long long total) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int deal = (int)(i / kTChoice), row = (int)(i - (long long)deal * kTChoice);
    const int d = depth_of_row(row);
    const scopa_team_state root = g_roots[deal];
    uint32_t w[10];
    memcpy(w, &root, 40);
    team_walk(w, d, row - t_offset(d), d);
    const uint32_t seat = (uint32_t)d & 3u;
    const int nh = (int)((w[7] >> (8u * seat)) & 255u);
    const uint32_t hand = tsd_seat_hand(w, seat) & (nh >= 4 ? 0xFFFFu : ((1u << (4 * nh)) - 1u));
    uint32_t hand_bits = 0;
    for (int k = 0; k < 4; k++) if (k < nh) hand_bits |= 1u << scopa::nib(hand, k);
    g_ninfo[i] = make_uint2(hand_bits | (tsd_table_bits(w) << 16), hand);
}

// the same bits at the four forced nodes below every depth-12 node (the hand is one card: its nibble is the index of the set bit)
__global__ void __launch_bounds__(256)
k_tsd_finfo(const scopa_team_state *__restrict__ g_roots, uint32_t *__restrict__ g_finfo /*[n][4][331776]*/, long long total) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int deal = (int)(i / kTLeaves), leaf = (int)(i - (long long)deal * kTLeaves);
    const scopa_team_state root = g_roots[deal];
    uint32_t w[10];
    memcpy(w, &root, 40);
    team_walk(w, 12, leaf, 12);
#pragma unroll 1
    for (uint32_t f = 0; f < 4u; f++) {   // depth 12 + f is played by seat f
        const int card = scopa::nib(tsd_seat_hand(w, f), 0);
        g_finfo[((size_t)deal * 4 + f) * kTLeaves + leaf] = (1u << card) | (tsd_table_bits(w) << 16);
        scopa_team::step_words(w, card);
    }
}

// ---- the policy launch -------------------------------------------------------------------------------------------------------------------
// Team T's tile list: segments 0..5 are its choice depths 0,1,4,5,8,9 (+ 2 T), segments 6, 7 its forced depths 12, 13 (+ 2 T), which are
// evaluated only where T is the traverser.  A segment's nodes are tiled sixteen at a time; tiles of different segments do not mix.
__host__ __device__ constexpr int tsd_seg_depth(int team, int c) { return c < 6 ? 4 * (c >> 1) + (c & 1) + 2 * team : 12 + 2 * team + (c - 6); }
__host__ __device__ constexpr int tsd_seg_width(int team, int c) { return c < 6 ? t_width(tsd_seg_depth(team, c)) : kTLeaves; }
__host__ __device__ constexpr int tsd_tile_off(int team, int c) { int o = 0; for (int k = 0; k < c; k++) o += (tsd_seg_width(team, k) + 15) >> 4; return o; }
static_assert(tsd_tile_off(0, 6) == 3954 && tsd_tile_off(1, 6) == 16133 && tsd_tile_off(0, 8) == 3954 + 41472, "tiles per team");
constexpr int kTsdPolicyWaves = 4;

// the tables of a call over m slots, in one allocation
__host__ __device__ inline size_t tsd_tab_thr_off(int m) { return (size_t)m * kTChoice * sizeof(float4); }
__host__ __device__ inline size_t tsd_tab_fpol_off(int m) { return tsd_tab_thr_off(m) + (size_t)m * kTChoice * 3 * sizeof(unsigned long long); }
__host__ __device__ inline size_t tsd_tab_bytes(int m) { return tsd_tab_fpol_off(m) + (size_t)m * 2 * kTLeaves * sizeof(float); }

__global__ void __launch_bounds__(kTsdPolicyWaves * 64)
k_team_chance_sdcfr_policy(const uint2 *__restrict__ g_ninfo /*[n][321365]*/, const uint32_t *__restrict__ g_finfo /*[n][4][331776]*/, const int32_t *__restrict__ list /*[m] or NULL*/,
                           const float *__restrict__ g_image, int traverser, int wg0, int wg1, float4 *__restrict__ g_pol /*[m][321365]*/,
                           unsigned long long *__restrict__ g_thr /*[m][321365][3]*/, float *__restrict__ g_fpol /*[m][2][331776]*/) {
    __shared__ SdTileLds s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nj = lane & 15, q = lane >> 4;
    const int per_slot = wg0 + wg1, slot = (int)blockIdx.x / per_slot, r = (int)blockIdx.x - slot * per_slot;
    const int team = r >= wg0 ? 1 : 0, chunk = team ? r - wg0 : r, n_chunks = team ? wg1 : wg0;
    const size_t deal = list ? (size_t)list[slot] : (size_t)slot;
    int off[9];
#pragma unroll
    for (int c = 0; c < 9; c++) off[c] = team ? tsd_tile_off(1, c) : tsd_tile_off(0, c);
    const int n_tiles = team == traverser ? off[8] : off[6];
    const int per = (n_tiles + n_chunks - 1) / n_chunks, t_begin = chunk * per, t_end = t_begin + per < n_tiles ? t_begin + per : n_tiles;
    SdSlices W;   // this wavefront's slices of the team's net, once per workgroup
    sd_load_slices(g_image + (size_t)team * kImgFloats, wave, lane, W);
    const uint2 *ninfo = g_ninfo + deal * kTChoice;
    const uint32_t *finfo = g_finfo + deal * 4 * kTLeaves;
    float4 *pol_out = g_pol + (size_t)slot * kTChoice;
    unsigned long long *thr_out = g_thr + (size_t)slot * kTChoice * 3;
    float *fpol_out = g_fpol + (size_t)slot * 2 * kTLeaves;

    for (int t = t_begin; t < t_end; t++) {
        int c = 0;
#pragma unroll
        for (int k = 1; k < 8; k++) c += t >= off[k] ? 1 : 0;
        const int j = (t - off[c]) * 16 + nj;
        const int d = tsd_seg_depth(team, c);
        bool live;
        uint32_t xbits, hand;
        int nl, row = 0;
        if (c < 6) {
            const int wd = t_width(d);
            live = j < wd;
            row = t_offset(d) + (live ? j : wd - 1);   // lanes beyond the level compute a copy of its last node and store nothing
            const uint2 inf = ninfo[row];
            xbits = inf.x; hand = inf.y; nl = t_branch(d);
        } else {
            live = true;                                // 331 776 is a multiple of 16
            xbits = finfo[(size_t)(d - 12) * kTLeaves + j];
            hand = (uint32_t)(__ffs((int)(xbits & 0xFFFFu)) - 1);
            nl = 1;
        }
        float pk = 0.0f;
        if (!sd_tile_policy(W, s, xbits, hand, nl, wave, lane, pk)) continue;
        if (c >= 6) {
            if (q == 0) fpol_out[(size_t)(c - 6) * kTLeaves + j] = pk;
            continue;
        }
        if (live) reinterpret_cast<float *>(pol_out + row)[q] = pk;
        unsigned long long thr[3] = {0ull, 0ull, 0ull};
        sd_tile_thresholds(s, nl, lane, pk, live, thr);
        if (q == 0 && live) {
            unsigned long long *out = thr_out + (size_t)row * 3;
            out[0] = thr[0]; out[1] = thr[1]; out[2] = thr[2];
        }
    }
}

// ---- the walk launch -----------------------------------------------------------------------------------------------------------------------
// the shape of traverser TR's traversal: a node of depth d has w_mult children in it; w_rows(d) memory rows lie in the subtree of a node of depth d
template <int TR> __host__ __device__ constexpr bool w_trav(int d) { return ((d & 3) >> 1) == TR; }
template <int TR> __host__ __device__ constexpr int w_mult(int d) { return d < 12 && w_trav<TR>(d) ? t_branch(d) : 1; }
template <int TR> __host__ __device__ constexpr int w_width(int d) { int w = 1; for (int k = 0; k < d; k++) w *= w_mult<TR>(k); return w; }
template <int TR> __host__ __device__ constexpr int w_off(int d) { int o = 0; for (int k = 0; k < d; k++) o += w_width<TR>(k); return o; }
template <int TR> __host__ __device__ constexpr int w_rows(int d) { int r = 0; for (int k = 15; k >= d; k--) r = (w_trav<TR>(k) ? 1 : 0) + w_mult<TR>(k) * r; return r; }
constexpr int kTsdArrivals = 576, kTsdFrontier = 2549;
static_assert(w_rows<0>(0) == kTsdRows && w_rows<1>(0) == kTsdRows && w_width<0>(12) == kTsdArrivals && w_width<1>(12) == kTsdArrivals, "rows per traversal");
static_assert(w_off<0>(12) == 1973 && w_off<1>(12) == 823 && w_off<0>(13) == kTsdFrontier, "visits per traversal");
constexpr unsigned long long kTsdVisits0 = 1973 + 4 * kTsdArrivals, kTsdVisits1 = 823 + 4 * kTsdArrivals;
static_assert(kTsdVisits0 == SCOPA_TEAM_SDCFR_VISITS0 && kTsdVisits1 == SCOPA_TEAM_SDCFR_VISITS1, "include/scopa.h states the visits");

// memory row of the FIRST row in the subtree of frontier position f of depth d (depth-first post-order: a node's own row is the last of its subtree)
template <int TR>
__device__ __forceinline__ int w_start(int d, int f) {
    int s = 0;
#pragma unroll
    for (int k = 11; k >= 0; k--)
        if (k < d && w_trav<TR>(k)) {
            const int b = t_branch(k), a = f % b;
            f /= b;
            s += a * w_rows<TR>(k + 1);
        }
    return s;
}

constexpr int kTsdWalkThreads = 256;
struct TsdWalkLds {
    uint32_t node[kTsdFrontier];       // index within its level of every frontier node, depths 0..12 one after the other
    float val[2][kTsdArrivals];        // values on the way back up, by frontier position: the level at hand and the one below
    uint32_t rec[kTsdArrivals][8];     // the memory rows of the level at hand: rank | feature bits | hand nibbles + legal count << 16 | regret of the illegal slots | of the legal ones [4]
};
static_assert(sizeof(TsdWalkLds) == 33236, "LDS per workgroup");

// value = sum policy * action value (float32, hand order, :335), regrets = counterfactual_values - value over all 16 slots with zeros at the illegal
// ones (:324, :339), max-abs normalisation (add_experience :73-74): scopa_sdcfr_backward's arithmetic.  Leaves the row's record, returns the value
__device__ __forceinline__ float tsd_row(uint32_t *rec, int rank, uint32_t xbits, uint32_t hand, int nl, const float *pl, const float *av) {
    float value = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; k++) if (k < nl) value += pl[k] * av[k];
    float rv[4], ri = 0.0f - value, mx = fabsf(ri);
#pragma unroll
    for (int k = 0; k < 4; k++) { rv[k] = (k < nl ? av[k] : 0.0f) - value; if (k < nl) { const float a = fabsf(rv[k]); mx = a > mx ? a : mx; } }
    if (mx > 0.0f) {
        const float den = mx + 1e-8f;
        ri = ri / den;
#pragma unroll
        for (int k = 0; k < 4; k++) rv[k] = rv[k] / den;
    }
    rec[0] = (uint32_t)rank; rec[1] = xbits; rec[2] = (hand & 0xFFFFu) | ((uint32_t)nl << 16); rec[3] = __float_as_uint(ri);
#pragma unroll
    for (int k = 0; k < 4; k++) rec[4 + k] = __float_as_uint(rv[k]);
    return value;
}

// the level's W rows to the ring, pieces in memory order: nine pieces of a 136-byte feature row and four of a 64-byte regret (mask) row in consecutive lanes
__device__ __forceinline__ void tsd_sweep(const uint32_t (*rec)[8], int W, uint32_t base, uint32_t capacity, float *__restrict__ mem_feat, float *__restrict__ mem_regret,
                                          float *__restrict__ mem_mask, int tid) {
    for (int e = tid; e < W * 9; e += kTsdWalkThreads) {
        const int rr = e / 9, i = e - rr * 9;
        const uint32_t hb = rec[rr][1] >> (4 * i);
        uint32_t row = base + rec[rr][0];
        row = row >= capacity ? row - capacity : row;
        float *dst = mem_feat + (size_t)row * 34 + 4 * i;
        if (i < 8) *reinterpret_cast<SdF4A8 *>(dst) = SdF4A8{(float)(hb & 1u), (float)((hb >> 1) & 1u), (float)((hb >> 2) & 1u), (float)((hb >> 3) & 1u)};
        else *reinterpret_cast<float2 *>(dst) = make_float2(1.0f, 0.0f);   // [32] = float(player == current_player), [33] unused
    }
    for (int e = tid; e < W * 4; e += kTsdWalkThreads) {
        const int rr = e >> 2, i = e & 3;
        uint32_t row = base + rec[rr][0];
        row = row >= capacity ? row - capacity : row;
        const uint32_t hand = rec[rr][2] & 0xFFFFu;
        const int nl = (int)(rec[rr][2] >> 16);
        const float ri = __uint_as_float(rec[rr][3]);
        float o[4] = {ri, ri, ri, ri};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int card = (int)((hand >> (4 * k)) & 15u);
            if (k < nl && (card >> 2) == i) {
                const float v = __uint_as_float(rec[rr][4 + k]);
                o[0] = (card & 3) == 0 ? v : o[0]; o[1] = (card & 3) == 1 ? v : o[1]; o[2] = (card & 3) == 2 ? v : o[2]; o[3] = (card & 3) == 3 ? v : o[3];
            }
        }
        reinterpret_cast<float4 *>(mem_regret + (size_t)row * 16)[i] = make_float4(o[0], o[1], o[2], o[3]);
        if (mem_mask != nullptr) {   // no mask array (the default ring): a row's mask IS features[0..16)
            const uint32_t hb = rec[rr][1] >> (4 * i);
            reinterpret_cast<float4 *>(mem_mask + (size_t)row * 16)[i] = make_float4((float)(hb & 1u), (float)((hb >> 1) & 1u), (float)((hb >> 2) & 1u), (float)((hb >> 3) & 1u));
        }
    }
}

template <int TR>
__global__ void __launch_bounds__(kTsdWalkThreads)
k_team_chance_sdcfr_walk(const uint2 *__restrict__ g_ninfo, const uint32_t *__restrict__ g_finfo, const int8_t *__restrict__ g_r2 /*[n][331776]*/,
                         const int32_t *__restrict__ list, const float4 *__restrict__ g_pol, const unsigned long long *__restrict__ g_thr, const float *__restrict__ g_fpol,
                         int batch, int wg_per_slot, float *__restrict__ mem_feat, float *__restrict__ mem_regret, float *__restrict__ mem_mask, uint32_t capacity,
                         uint32_t write_base, float *__restrict__ root_values, uint32_t seed_lo, uint32_t seed_hi, uint32_t iteration, uint32_t b0) {
    __shared__ TsdWalkLds s;
    const int tid = threadIdx.x;
    const int slot = (int)blockIdx.x / wg_per_slot, wg = (int)blockIdx.x - slot * wg_per_slot;
    const size_t deal = list ? (size_t)list[slot] : (size_t)slot;
    const uint2 *ninfo = g_ninfo + deal * kTChoice;
    const uint32_t *finfo = g_finfo + (deal * 4 + 2 * TR) * kTLeaves;   // the traverser's two forced depths
    const int8_t *r2 = g_r2 + deal * kTLeaves;
    const float4 *pol = g_pol + (size_t)slot * kTChoice;
    const unsigned long long *thr = g_thr + (size_t)slot * kTChoice * 3;
    const float *fpol = g_fpol + (size_t)slot * 2 * kTLeaves;
    for (int i = wg; i < batch; i += wg_per_slot) {
        const uint32_t trav_id = b0 + (uint32_t)deal * (uint32_t)batch + (uint32_t)i;
        const uint32_t base = (uint32_t)(((unsigned long long)write_base + (unsigned long long)kTsdRows * ((unsigned long long)slot * (unsigned long long)batch + (unsigned long long)i)) %
                                         (unsigned long long)capacity);
        if (tid == 0) s.node[0] = 0;
        __syncthreads();
        // ---- down: the frontier of every depth ----
#pragma unroll
        for (int d = 0; d < 12; d++) {
            const int W = w_width<TR>(d), o = w_off<TR>(d), o1 = w_off<TR>(d + 1), b = t_branch(d);
            for (int f = tid; f < W; f += kTsdWalkThreads) {
                const uint32_t nd = s.node[o + f];
                if (w_trav<TR>(d)) {   // recurse on ALL legal actions, hand order (:326-336)
                    for (int k = 0; k < b; k++) s.node[o1 + f * b + k] = nd * (uint32_t)b + (uint32_t)k;
                } else {                // sample ONE action (:347-365): integer compares against the node's thresholds
                    const uint32_t row = (uint32_t)t_offset(d) + nd;
                    const scopa::philox_out x = scopa::philox4x32_10(row, trav_id, iteration, kTsdPhiloxTag + (uint32_t)TR, seed_lo, seed_hi);
                    const unsigned long long N = ((unsigned long long)(x.x0 >> 5) << 26) | (unsigned long long)(x.x1 >> 6);   // u = N * 2^-53 (u53)
                    const unsigned long long *th = thr + (size_t)row * 3;
                    const unsigned long long t0 = th[0], t1 = th[1], t2 = th[2];
                    int a = (int)(t0 <= N) + (int)(t1 <= N) + (int)(t2 <= N);
                    if (t0 == ~0ull) {   // probs.sum() == 0: np.random.choice(legal_actions), uniform, numpy's float64 arithmetic
                        const double u = (double)N * 0x1p-53;
                        a = (int)(u * (double)b);
                    }
                    a = a < b - 1 ? a : b - 1;
                    s.node[o1 + f] = nd * (uint32_t)b + (uint32_t)a;
                }
            }
            __syncthreads();
        }
        // ---- the forced tail: the traverser's two forced rows of every arrival, the deeper one first; the arrival's value ----
        int cur = 0;
#pragma unroll
        for (int fd = 1; fd >= 0; fd--) {
            for (int f = tid; f < kTsdArrivals; f += kTsdWalkThreads) {
                const uint32_t leaf = s.node[w_off<TR>(12) + f];
                const int p0 = r2[leaf];
                const float term = 0.5f * (float)(TR == 0 ? p0 : -p0);
                const float pl1[4] = {fpol[(size_t)kTLeaves + leaf], 0.0f, 0.0f, 0.0f}, av1[4] = {term, 0.0f, 0.0f, 0.0f};
                const int start = w_start<TR>(12, f);
                float v;
                if (fd == 1) {
                    const uint32_t xb = finfo[(size_t)kTLeaves + leaf];
                    v = tsd_row(s.rec[f], start, xb, (uint32_t)(__ffs((int)(xb & 0xFFFFu)) - 1), 1, pl1, av1);
                } else {
                    float v1 = 0.0f;
                    v1 += pl1[0] * av1[0];
                    const float pl0[4] = {fpol[leaf], 0.0f, 0.0f, 0.0f}, av0[4] = {v1, 0.0f, 0.0f, 0.0f};
                    const uint32_t xb = finfo[leaf];
                    v = tsd_row(s.rec[f], start + 1, xb, (uint32_t)(__ffs((int)(xb & 0xFFFFu)) - 1), 1, pl0, av0);
                    s.val[cur][f] = v;   // the other team's forced plies return their child's value unchanged
                }
                (void)v;
            }
            __syncthreads();
            tsd_sweep(s.rec, kTsdArrivals, base, capacity, mem_feat, mem_regret, mem_mask, tid);
            __syncthreads();
        }
        // ---- up: the traverser's choice levels; the other team's levels hand their sampled child's value on at the same position ----
#pragma unroll
        for (int d = 11; d >= 0; d--) {
            if (!w_trav<TR>(d)) continue;
            const int W = w_width<TR>(d), o = w_off<TR>(d), b = t_branch(d);
            for (int f = tid; f < W; f += kTsdWalkThreads) {
                const uint32_t row = (uint32_t)t_offset(d) + s.node[o + f];
                const float4 p4 = pol[row];
                const uint2 inf = ninfo[row];
                const float pl[4] = {p4.x, p4.y, p4.z, p4.w};
                float av[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                for (int k = 0; k < b; k++) av[k] = s.val[cur][f * b + k];
                s.val[cur ^ 1][f] = tsd_row(s.rec[f], w_start<TR>(d, f) + w_rows<TR>(d) - 1, inf.x, inf.y, b, pl, av);
            }
            __syncthreads();
            tsd_sweep(s.rec, W, base, capacity, mem_feat, mem_regret, mem_mask, tid);
            cur ^= 1;
            __syncthreads();
        }
        if (tid == 0) root_values[(size_t)slot * batch + i] = s.val[cur][0];
        __syncthreads();
    }
}

// ---- the average policy over keys ------------------------------------------------------------------------------------------------------------
struct TsdRanks { long long depth_off[12], team_base[12]; };   // global ids of depth d start at depth_off[d]; team_base[d]: keys of the depth's team at lower depths

// {feature bits, hand nibbles, global id, legal count} of every key's representative node -- its first occurrence in CSR order --, per team in ascending global id
__global__ void __launch_bounds__(256)
k_tsd_reps(const uint64_t *__restrict__ g_key, const int32_t *__restrict__ g_occ_off, const int32_t *__restrict__ g_occ, const uint2 *__restrict__ g_ninfo /*flat [n * 321365]*/,
           TsdRanks rk, uint4 *__restrict__ rep0, uint4 *__restrict__ rep1, long long G) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    const int d = key_depth(g_key[g]);
    const uint2 inf = g_ninfo[(size_t)g_occ[g_occ_off[g]]];
    long long idx = 0;
#pragma unroll
    for (int k = 0; k < 12; k++) idx = k == d ? g - rk.depth_off[k] + rk.team_base[k] : idx;
    (t_team(d) ? rep1 : rep0)[idx] = make_uint4(inf.x, inf.y, (uint32_t)g, (uint32_t)t_branch(d));
}

unsigned tsd_blocks(long long lanes) { return (unsigned)((lanes + 255) / 256); }

// the node-info images, once per handle
int32_t tsd_ensure_info(scopa_team_chance *g) {
    if (g->sd_info_built) return SCOPA_OK;
    scopa_ctx *ctx = g->ctx;
    const size_t rows = (size_t)g->n * kTChoice, leaves = (size_t)g->n * kTLeaves;
    scopa_team_state *d_roots = nullptr;
    bool ok = (g->d_sd_ninfo || hipMalloc(&g->d_sd_ninfo, rows * sizeof(uint2)) == hipSuccess) &&
              (g->d_sd_finfo || hipMalloc(&g->d_sd_finfo, leaves * 4 * sizeof(uint32_t)) == hipSuccess) &&
              hipMalloc(&d_roots, (size_t)g->n * sizeof(scopa_team_state)) == hipSuccess;
    if (!ok) {
        if (d_roots) (void)hipFree(d_roots);
        return fail(ctx, SCOPA_ENOMEM, "scopa_team_chance_sdcfr: no device memory for the node-info images");
    }
    hipError_t e = hipMemcpyAsync(d_roots, g->h_roots.data(), (size_t)g->n * sizeof(scopa_team_state), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_tsd_ninfo, dim3(tsd_blocks((long long)rows)), dim3(256), 0, ctx->stream, (const scopa_team_state *)d_roots, (uint2 *)g->d_sd_ninfo, (long long)rows);
        hipLaunchKernelGGL(k_tsd_finfo, dim3(tsd_blocks((long long)leaves)), dim3(256), 0, ctx->stream, (const scopa_team_state *)d_roots, g->d_sd_finfo, (long long)leaves);
        e = hipGetLastError();
    }
    const hipError_t e2 = hipStreamSynchronize(ctx->stream);   // the roots go away below; once per handle
    (void)hipFree(d_roots);
    SC_HIP(ctx, e);
    SC_HIP(ctx, e2);
    g->sd_info_built = true;
    return SCOPA_OK;
}

bool tsd_list_ok(int n, int m, const int32_t *h_deals) {
    std::vector<char> seen((size_t)n, 0);
    for (int k = 0; k < m; k++) {
        const int32_t d = h_deals[k];
        if (d < 0 || d >= n || seen[(size_t)d]) return false;
        seen[(size_t)d] = 1;
    }
    return true;
}

}  // namespace

namespace scopa {
void team_chance_sdcfr_release(scopa_team_chance *g) {
    void *bufs[] = {g->d_sd_ninfo, g->d_sd_finfo, g->d_sd_tab, g->d_sd_list, g->d_sd_rep[0], g->d_sd_rep[1], g->d_sd_terms};
    for (void *b : bufs) if (b) (void)hipFree(b);
    if (g->h_sd_list) (void)hipHostFree(g->h_sd_list);
    for (hipEvent_t &e : g->sd_ev) if (e) { (void)hipEventDestroy(e); e = nullptr; }
    g->d_sd_ninfo = nullptr; g->d_sd_finfo = nullptr; g->d_sd_tab = nullptr; g->d_sd_list = nullptr; g->h_sd_list = nullptr;
    g->d_sd_rep[0] = g->d_sd_rep[1] = nullptr; g->d_sd_terms = nullptr;
}
}  // namespace scopa

extern "C" {

int32_t scopa_team_chance_sdcfr_traverse(scopa_team_chance *g, int32_t traverser, int32_t batch, int32_t m_deals, const int32_t *h_deals, const float *d_image,
                                         float *d_mem_feat, float *d_mem_regret, float *d_mem_mask, int64_t capacity, int64_t write_base, float *d_root_values,
                                         uint32_t iteration, uint32_t b0) {
    if (!g) return SCOPA_EINVAL;
    scopa_ctx *ctx = g->ctx;
    const int n = g->n;
    SC_REQUIRE(ctx, traverser == 0 || traverser == 1, SCOPA_EINVAL, "scopa_team_chance_sdcfr_traverse: traverser must be 0 or 1");
    SC_REQUIRE(ctx, h_deals ? (m_deals >= 1 && m_deals <= n) : (m_deals == 0 || m_deals == n), SCOPA_EINVAL,
               "scopa_team_chance_sdcfr_traverse: a list holds 1 .. n deals; without a list m is 0 (or n): all deals");
    SC_REQUIRE(ctx, batch >= 0 && !(batch == 0 && h_deals), SCOPA_EINVAL, "scopa_team_chance_sdcfr_traverse: batch must be positive (0 without a list: no-op)");
    if (!batch) return SCOPA_OK;
    const int m = h_deals ? m_deals : n;
    SC_REQUIRE(ctx, d_image && d_mem_feat && d_mem_regret && d_root_values, SCOPA_EINVAL, "scopa_team_chance_sdcfr_traverse: NULL device pointer");
    SC_REQUIRE(ctx, !h_deals || tsd_list_ok(n, m, h_deals), SCOPA_EINVAL, "scopa_team_chance_sdcfr_traverse: a listed deal is outside [0, n) or listed twice");
    SC_REQUIRE(ctx, ((uintptr_t)d_image & 15) == 0, SCOPA_EINVAL, "scopa_team_chance_sdcfr_traverse: the weight image must be 16-byte aligned");
    SC_REQUIRE(ctx, ((uintptr_t)d_mem_feat & 7) == 0 && ((uintptr_t)d_mem_regret & 15) == 0 && ((uintptr_t)d_mem_mask & 15) == 0, SCOPA_EINVAL,
               "scopa_team_chance_sdcfr_traverse: memory rows are stored 8 / 16 bytes at a time: d_mem_feat must be 8-byte, d_mem_regret / d_mem_mask 16-byte aligned");
    SC_REQUIRE(ctx, capacity >= kTsdRows && capacity < ((int64_t)1 << 30) && write_base >= 0 && write_base < capacity, SCOPA_EINVAL,
               "scopa_team_chance_sdcfr_traverse: write_base must lie in [0, capacity), capacity in [1653, 2^30) rows");
    SC_REQUIRE(ctx, (int64_t)kTsdRows * m * batch <= capacity, SCOPA_EINVAL, "scopa_team_chance_sdcfr_traverse: memory ring too small for 1653 * m * batch rows");
    SC_REQUIRE(ctx, (uint64_t)b0 + (uint64_t)n * (uint64_t)batch <= ((uint64_t)1 << 32), SCOPA_EINVAL,
               "scopa_team_chance_sdcfr_traverse: traversal ids b0 + n * batch exceed 2^32");
    SC_HIP(ctx, hipSetDevice(ctx->device));
    scopa::Range range_("scopa team chance sdcfr traverse");
    if (int32_t rc = tsd_ensure_info(g)) return rc;
    if (m > g->sd_tab_slots) {
        SC_HIP(ctx, hipStreamSynchronize(ctx->stream));   // an earlier call's launches may still read the old tables
        if (g->d_sd_tab) { (void)hipFree(g->d_sd_tab); g->d_sd_tab = nullptr; g->sd_tab_slots = 0; g->sd_last_m = 0; }
        if (hipMalloc(&g->d_sd_tab, tsd_tab_bytes(m)) != hipSuccess) { g->d_sd_tab = nullptr; return fail(ctx, SCOPA_ENOMEM, "scopa_team_chance_sdcfr_traverse: no device memory for the policy tables"); }
        g->sd_tab_slots = m;
    }
    if (h_deals) {
        // the list reaches the device without a wait for the stream: through this turn's row of a pinned ring (free once the copy made from it
        // kTsdRing calls ago is done) and from there, in stream order behind the previous call's kernels, into d_sd_list
        if (!g->h_sd_list) {
            if (hipMalloc(&g->d_sd_list, (size_t)n * 4) != hipSuccess) { g->d_sd_list = nullptr; return fail(ctx, SCOPA_ENOMEM, "scopa_team_chance_sdcfr_traverse: no device memory for the list"); }
            if (hipHostMalloc(&g->h_sd_list, (size_t)kTsdRing * n * 4, hipHostMallocDefault) != hipSuccess) { g->h_sd_list = nullptr; return fail(ctx, SCOPA_ENOMEM, "scopa_team_chance_sdcfr_traverse: no pinned memory for the list"); }
            for (int i = 0; i < kTsdRing; i++) SC_HIP(ctx, hipEventCreateWithFlags(&g->sd_ev[i], hipEventDisableTiming));
        }
        const unsigned turn = g->sd_turn % kTsdRing;
        if (g->sd_turn >= (unsigned)kTsdRing) SC_HIP(ctx, hipEventSynchronize(g->sd_ev[turn]));
        int32_t *row = g->h_sd_list + (size_t)turn * n;
        std::copy(h_deals, h_deals + m, row);
        SC_HIP(ctx, hipMemcpyAsync(g->d_sd_list, row, (size_t)m * 4, hipMemcpyHostToDevice, ctx->stream));
        SC_HIP(ctx, hipEventRecord(g->sd_ev[turn], ctx->stream));
        g->sd_turn++;
        if (g->sd_turn >= 2u * kTsdRing) g->sd_turn -= kTsdRing;   // (stays >= kTsdRing: every row has been used)
    }
    const int32_t *d_list = h_deals ? g->d_sd_list : nullptr;
    unsigned char *tab = (unsigned char *)g->d_sd_tab;
    float4 *d_pol = (float4 *)tab;
    unsigned long long *d_thr = (unsigned long long *)(tab + tsd_tab_thr_off(m));
    float *d_fpol = (float *)(tab + tsd_tab_fpol_off(m));
    const int launches = ctx->team_sdcfr_launches;   // benchmark hook: 1 = the policy launch alone, 2 = the walk launch alone over the tables of the call before
    SC_REQUIRE(ctx, launches != 2 || g->sd_last_m == m, SCOPA_ESTATE, "scopa_team_chance_sdcfr_traverse: the walk launch alone needs the tables of a call over as many slots");
    g->sd_last_m = m;
    if (launches != 2) {   // about eight workgroups per compute unit over all slots, cut between the two teams by their tiles, one at least for each
        const int tiles0 = tsd_tile_off(0, traverser == 0 ? 8 : 6), tiles1 = tsd_tile_off(1, traverser == 1 ? 8 : 6);
        int per_slot = (8 * ctx->n_cus + m - 1) / m;
        per_slot = per_slot < 2 ? 2 : per_slot;
        int wg0 = (int)(((long long)per_slot * tiles0 + (tiles0 + tiles1) / 2) / (tiles0 + tiles1));
        wg0 = wg0 < 1 ? 1 : wg0 > per_slot - 1 ? per_slot - 1 : wg0;
        const int wg1 = per_slot - wg0;
        hipLaunchKernelGGL(k_team_chance_sdcfr_policy, dim3((unsigned)m * (unsigned)per_slot), dim3(kTsdPolicyWaves * 64), 0, ctx->stream, (const uint2 *)g->d_sd_ninfo,
                           (const uint32_t *)g->d_sd_finfo, d_list, d_image, (int)traverser, wg0, wg1, d_pol, d_thr, d_fpol);
        SC_HIP(ctx, hipGetLastError());
    }
    if (launches == 1) return SCOPA_OK;
    {   // about four workgroups per compute unit over all slots, at least one per slot, none without a traversal
        int wg_per_slot = (4 * ctx->n_cus + m - 1) / m;
        if (ctx->team_sdcfr_walk_groups > 0 && wg_per_slot > ctx->team_sdcfr_walk_groups) wg_per_slot = ctx->team_sdcfr_walk_groups;   // test hook
        wg_per_slot = wg_per_slot < 1 ? 1 : wg_per_slot > batch ? batch : wg_per_slot;
        const auto walk = traverser == 0 ? k_team_chance_sdcfr_walk<0> : k_team_chance_sdcfr_walk<1>;
        hipLaunchKernelGGL(walk, dim3((unsigned)m * (unsigned)wg_per_slot), dim3(kTsdWalkThreads), 0, ctx->stream, (const uint2 *)g->d_sd_ninfo, (const uint32_t *)g->d_sd_finfo,
                           (const int8_t *)g->d_r2, d_list, (const float4 *)d_pol, (const unsigned long long *)d_thr, (const float *)d_fpol, (int)batch, wg_per_slot, d_mem_feat,
                           d_mem_regret, d_mem_mask, (uint32_t)capacity, (uint32_t)write_base, d_root_values, (uint32_t)ctx->seed, (uint32_t)(ctx->seed >> 32), iteration, b0);
        SC_HIP(ctx, hipGetLastError());
    }
    g->sd_visits += (uint64_t)m * (uint64_t)batch * (traverser == 0 ? kTsdVisits0 : kTsdVisits1);
    return SCOPA_OK;
}

int32_t scopa_team_chance_sdcfr_visits(scopa_team_chance *g, uint64_t *decision_visits) {
    if (!g || !decision_visits) return SCOPA_EINVAL;
    *decision_visits = g->sd_visits;   // counted on the host from the traversal's fixed shape: no wait for the stream
    return SCOPA_OK;
}

int32_t scopa_team_chance_sdcfr_policy_get(scopa_team_chance *g, int32_t slot, float *h_policy, uint64_t *h_thr) {
    if (!g) return SCOPA_EINVAL;
    scopa_ctx *ctx = g->ctx;
    SC_REQUIRE(ctx, g->sd_last_m > 0, SCOPA_ESTATE, "scopa_team_chance_sdcfr_policy_get: no traversal call yet");
    SC_REQUIRE(ctx, slot >= 0 && slot < g->sd_last_m, SCOPA_EINVAL, "scopa_team_chance_sdcfr_policy_get: slot outside the last call's list");
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const unsigned char *tab = (const unsigned char *)g->d_sd_tab;
    if (h_policy) SC_HIP(ctx, hipMemcpyAsync(h_policy, tab + (size_t)slot * kTChoice * sizeof(float4), (size_t)kTChoice * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
    if (h_thr) SC_HIP(ctx, hipMemcpyAsync(h_thr, tab + tsd_tab_thr_off(g->sd_last_m) + (size_t)slot * kTChoice * 24, (size_t)kTChoice * 24, hipMemcpyDeviceToHost, ctx->stream));
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SCOPA_OK;
}

int32_t scopa_team_chance_sdcfr_forced_get(scopa_team_chance *g, int32_t slot, float *h_forced) {
    if (!g || !h_forced) return SCOPA_EINVAL;
    scopa_ctx *ctx = g->ctx;
    SC_REQUIRE(ctx, g->sd_last_m > 0, SCOPA_ESTATE, "scopa_team_chance_sdcfr_forced_get: no traversal call yet");
    SC_REQUIRE(ctx, slot >= 0 && slot < g->sd_last_m, SCOPA_EINVAL, "scopa_team_chance_sdcfr_forced_get: slot outside the last call's list");
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const unsigned char *tab = (const unsigned char *)g->d_sd_tab;
    SC_HIP(ctx, hipMemcpyAsync(h_forced, tab + tsd_tab_fpol_off(g->sd_last_m) + (size_t)slot * 2 * kTLeaves * sizeof(float), (size_t)2 * kTLeaves * sizeof(float),
                               hipMemcpyDeviceToHost, ctx->stream));
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SCOPA_OK;
}

int32_t scopa_team_chance_debug_sdcfr(scopa_ctx *ctx, int64_t terms_bytes, int32_t walk_groups, int32_t launches) {
    if (!ctx || terms_bytes < 0 || walk_groups < 0 || launches < 0 || launches > 2) return SCOPA_EINVAL;
    ctx->team_sdcfr_budget = terms_bytes;
    ctx->team_sdcfr_walk_groups = walk_groups;
    ctx->team_sdcfr_launches = launches;
    return SCOPA_OK;
}

int32_t scopa_team_chance_sdcfr_average_policy(scopa_team_chance *g, int32_t team, int32_t n_snap, const float *d_w1, const float *d_b1, const float *d_w2,
                                               const float *d_b2, const float *d_w3, const float *d_b3, int32_t max_size, const int32_t *d_slots,
                                               const float *d_coef, double *d_policy_G) {
    if (!g) return SCOPA_EINVAL;
    scopa_ctx *ctx = g->ctx;
    SC_REQUIRE(ctx, (team == 0 || team == 1) && n_snap >= 0 && max_size >= 0 && n_snap <= max_size && d_policy_G, SCOPA_EINVAL,
               "scopa_team_chance_sdcfr_average_policy: team in {0, 1}, 0 <= n_snap <= max_size and a policy table are required");
    if (n_snap > 0) {
        SC_REQUIRE(ctx, d_w1 && d_b1 && d_w2 && d_b2 && d_w3 && d_b3 && d_slots && d_coef, SCOPA_EINVAL, "scopa_team_chance_sdcfr_average_policy: NULL device pointer");
        const uintptr_t any = (uintptr_t)d_b1 | (uintptr_t)d_w2 | (uintptr_t)d_b2 | (uintptr_t)d_w3 | (uintptr_t)d_b3;
        SC_REQUIRE(ctx, (any & 15) == 0, SCOPA_EINVAL, "scopa_team_chance_sdcfr_average_policy: b1, w2, b2, w3, b3 are read 16 bytes at a time and must be 16-byte aligned");
    }
    SC_HIP(ctx, hipSetDevice(ctx->device));
    if (int32_t rc = tsd_ensure_info(g)) return rc;
    if (!g->sd_rep_built) {   // once per handle: the keys' representative nodes, per team in ascending global id
        TsdRanks rk;
        long long cnt[2] = {0, 0};
        for (int d = 0; d < 12; d++) {
            rk.depth_off[d] = g->depth_off[d];
            rk.team_base[d] = cnt[t_team(d)];
            cnt[t_team(d)] += g->depth_off[d + 1] - g->depth_off[d];
        }
        for (int t = 0; t < 2; t++)
            if (!g->d_sd_rep[t] && hipMalloc(&g->d_sd_rep[t], (size_t)(cnt[t] ? cnt[t] : 1) * sizeof(uint4)) != hipSuccess) {
                g->d_sd_rep[t] = nullptr;
                return fail(ctx, SCOPA_ENOMEM, "scopa_team_chance_sdcfr_average_policy: no device memory for the key list");
            }
        hipLaunchKernelGGL(k_tsd_reps, dim3(tsd_blocks(g->G)), dim3(256), 0, ctx->stream, (const uint64_t *)g->d_gkey, (const int32_t *)g->d_occ_off, (const int32_t *)g->d_occ,
                           (const uint2 *)g->d_sd_ninfo, rk, (uint4 *)g->d_sd_rep[0], (uint4 *)g->d_sd_rep[1], g->G);
        SC_HIP(ctx, hipGetLastError());
        g->sd_keys[0] = cnt[0]; g->sd_keys[1] = cnt[1];
        g->sd_rep_built = true;
    }
    // the keys go through in chunks whose terms [n_snap][chunk] float4 stay under the scratch budget (1 GiB unless scopa_team_chance_debug_sdcfr says otherwise);
    // a chunk is a multiple of sixteen keys, so every key sits in the tile column it has in one pass over all keys -- and a column's result
    // depends on its own operands alone
    const long long n_keys = g->sd_keys[team];
    const long long budget = ctx->team_sdcfr_budget > 0 ? ctx->team_sdcfr_budget : (1ll << 30);
    long long chunk = n_snap > 0 ? budget / (16ll * n_snap) : n_keys;
    chunk = chunk > (1ll << 30) ? (1ll << 30) : chunk;
    chunk = (chunk / 16) * 16;
    chunk = chunk < 16 ? 16 : chunk;
    chunk = chunk > n_keys ? n_keys : chunk;
    const size_t bytes = (size_t)n_snap * (size_t)chunk * 16;
    if (bytes > g->sd_terms_bytes) {
        SC_HIP(ctx, hipStreamSynchronize(ctx->stream));   // an earlier call's launches may still read the old buffer
        if (g->d_sd_terms) { (void)hipFree(g->d_sd_terms); g->d_sd_terms = nullptr; g->sd_terms_bytes = 0; }
        if (hipMalloc(&g->d_sd_terms, bytes) != hipSuccess) { g->d_sd_terms = nullptr; return fail(ctx, SCOPA_ENOMEM, "scopa_team_chance_sdcfr_average_policy: no device memory for the terms"); }
        g->sd_terms_bytes = bytes;
    }
    for (long long k0 = 0; k0 < n_keys; k0 += chunk) {
        const int cnt = (int)(n_keys - k0 < chunk ? n_keys - k0 : chunk);
        if (int32_t rc = scopa::launch_chance_sdcfr_avg(ctx, cnt, (const uint4 *)g->d_sd_rep[team] + k0, n_snap, d_w1, d_b1, d_w2, d_b2, d_w3, d_b3, max_size, d_slots, d_coef,
                                                        g->d_sd_terms, d_policy_G))
            return rc;
    }
    return SCOPA_OK;
}

}  // extern "C"
