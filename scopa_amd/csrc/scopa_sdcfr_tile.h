// scopa_sdcfr_tile.h -- the 34-128-64-16 advantage net (MiniScopa, Team MiniScopa) on the matrix cores, stated once: the layout of the packed net image
// (written by k_sdcfr_pack, scopa_sdcfr.hip), the one-instruction helpers of a 16-node tile, and the body of ONE such tile as a workgroup of four
// wavefronts runs it, from the feature bits of 16 nodes to their policy[4] in hand order and their sampling thresholds[3]: the register slices of a net
// (SdSlices, loaded from the packed image or from torch tensors), the LDS a tile hands its layers through (SdTileLds), sd_tile_policy and
// sd_tile_thresholds, the latter on the threshold rule sd_thresholds<N>, which FullScopa's wide net shares.  Definitions only, no kernel.  Included by
// scopa_sdcfr.hip (k_sdcfr_policy, k_chance_sdcfr_policy; its one-wavefront kernels use the helpers), scopa_sdcfr_avg.hip (k_sdcfr_avg_terms,
// k_chance_sdcfr_avg_terms), scopa_team_chance_sdcfr.hip (k_team_chance_sdcfr_policy), scopa_full_sdcfr_tile.h and (for v4f and mfma16)
// scopa_train_tile.h.  The static_assert below ties the layout to the size the public header states.
//
//   tile      v_mfma_f32_16x16x4_f32 with the WEIGHTS as the 16 x 4 operand (16 output units) and the 16 NODES as the columns: lane (q, nj) = (lane / 16,
//             lane % 16) holds outputs 4 q + r (r = 0..3) of node nj, which is the B-operand layout of the next layer's K-step over those four units.  A
//             column's result depends on its own node and the weights alone: which nodes share a tile changes no bit.
//   K order   every accumulator sees the K order of k_sdcfr_traverse: layer 1 starts at b1[u] + W1[u][32] (feature 32 is the constant 1, feature 33 is 0)
//             and adds the 32 feature bits four at a time, inputs 4 s + q in step s ascending; layer 2 starts at the bias and adds the 128 hidden units in
//             blocks of 16 ascending; layer 3 is TWO chains -- the bias + hidden blocks 0, 2 and blocks 1, 3 -- added at the end as o0 + o1.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/scopa.h"

namespace {
// the net image in LDS, per player (float32), written by k_sdcfr_pack from the torch tensors W[out][in]:
constexpr int kImgW1 = 0;                 // [8 mt][2 g][64 lanes][4 c] : W1[16 mt + lane%16][4 (4g + c) + lane/16]       4096
constexpr int kImgC1 = kImgW1 + 4096;     // [128]                      : b1[u] + W1[u][32]  (feature 32 is the constant 1)  128
constexpr int kImgW2 = kImgC1 + 128;      // [4 nt][8 mt][64 lanes][4 r]: W2[16 nt + lane%16][16 mt + 4 (lane/16) + r]     8192
constexpr int kImgB2 = kImgW2 + 8192;     // [64]                                                                            64
constexpr int kImgW3 = kImgB2 + 64;       // [4 nt][64 lanes][4 r]      : W3[lane%16][16 nt + 4 (lane/16) + r]             1024
constexpr int kImgB3 = kImgW3 + 1024;     // [16]                                                                            16
constexpr int kImgFloats = kImgB3 + 16;   // 13 520 (the 13 776 parameters less W1's columns 32, 33)
static_assert(kImgFloats == SCOPA_SDCFR_IMAGE_FLOATS, "include/scopa.h states the image size");

// A wavefront's LDS operations execute in order, so lane A's store is seen by lane B's later load without any wait; this only
// keeps the compiler from moving LDS accesses across the point (the wait for a load's data is the compiler's own s_waitcnt).
__device__ __forceinline__ void sd_order() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

typedef float v4f __attribute__((ext_vector_type(4)));
typedef unsigned v2u __attribute__((ext_vector_type(2)));
__device__ __forceinline__ v4f mfma16(float a, float b, v4f c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ v4f to_v4f(float4 x) { v4f r = {x.x, x.y, x.z, x.w}; return r; }
__device__ __forceinline__ float relu(float x) { return __builtin_amdgcn_fmed3f(x, 0.0f, __builtin_huge_valf()); }   // one v_max (fmaxf costs two: it quiets NaNs first)
// x + (the same register of lane ^ 16), then + lane ^ 32: gfx950's row swaps instead of two trips through the LDS crossbar
__device__ __forceinline__ float sum_row_groups(float x) {
    const unsigned xi = __float_as_uint(x);
    const v2u a = __builtin_amdgcn_permlane16_swap(xi, xi, false, false);     // rows (16 lanes) 1 <-> 0 and 3 <-> 2 of the two copies
    const float s = __uint_as_float(a[0]) + __uint_as_float(a[1]);
    const unsigned si = __float_as_uint(s);
    const v2u b = __builtin_amdgcn_permlane32_swap(si, si, false, false);     // upper half <-> lower half
    return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}
struct __attribute__((aligned(8))) SdF4A8 { float x, y, z, w; };   // sixteen bytes of a 136-byte feature row: rows alternate between 16- and 8-byte alignment

// ---- the tile of a workgroup of four wavefronts ----------------------------------------------------------------------------------------------------
// The tile's MLP is cut ACROSS the wavefronts -- layer 1: two of the eight 16-unit blocks each; layer 2: one of the four blocks each; layer 3: its two
// accumulator chains on wavefronts 0 and 1 -- with the activations handed over through LDS (an MFMA result IS the next layer's B operand, lane for
// lane: a float4 per lane and block).

// the slices wavefront `wave` of four keeps in registers (64 floats a lane): layer 1 unit blocks 2 wave, 2 wave + 1 (w1[h][g]: K-steps 4 g .. 4 g + 3 of
// block 2 wave + h; c1: the initial accumulator); layer 2 unit block `wave`; layer 3 hidden blocks (wave & 1) + 2 h (used by wavefronts 0 and 1)
struct SdSlices {
    float4 w1[2][2], c1[2], w2[8], w3[2], b2, b3;
};

// from k_sdcfr_pack's image of one player's net: 16 float4 per lane straight from global memory, all in flight at once (no staging of the 54 KB net, no
// barrier in front of the first MFMA)
__device__ __forceinline__ void sd_load_slices(const float *__restrict__ Wn, int wave, int lane, SdSlices &s) {
    const int q = lane >> 4;
    const float4 *w1 = reinterpret_cast<const float4 *>(Wn + kImgW1) + lane, *c1 = reinterpret_cast<const float4 *>(Wn + kImgC1) + q;
    const float4 *w2 = reinterpret_cast<const float4 *>(Wn + kImgW2) + lane, *w3 = reinterpret_cast<const float4 *>(Wn + kImgW3) + lane;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int mt = 2 * wave + h;
        s.c1[h] = c1[mt * 4];
#pragma unroll
        for (int g = 0; g < 2; g++) s.w1[h][g] = w1[(mt * 2 + g) * 64];
    }
#pragma unroll
    for (int mt = 0; mt < 8; mt++) s.w2[mt] = w2[(wave * 8 + mt) * 64];
#pragma unroll
    for (int h = 0; h < 2; h++) s.w3[h] = w3[((wave & 1) + 2 * h) * 64];
    s.b2 = (reinterpret_cast<const float4 *>(Wn + kImgB2) + q)[wave * 4];
    s.b3 = (reinterpret_cast<const float4 *>(Wn + kImgB3) + q)[0];
}

// the same slices straight from one net's torch tensors (row-major W[out][in]; b1, w2, b2, w3, b3 16-byte aligned): exactly the operands sd_load_slices
// takes from the image, the constant-1 feature 32 folded into the layer-1 bias as k_sdcfr_pack folds it (one float32 add).  For a kernel that uses
// each net once (the average policy's snapshots): a pack launch into the operand image would write and read the same 55 KB per net again for the same
// loads into the same registers.
__device__ __forceinline__ void sd_load_slices_torch(const float *__restrict__ W1, const float *__restrict__ B1, const float *__restrict__ W2,
                                                     const float *__restrict__ B2, const float *__restrict__ W3, const float *__restrict__ B3, int wave,
                                                     int lane, SdSlices &s) {
    const int nj = lane & 15, q = lane >> 4;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int mt = 2 * wave + h;
        const float *row = W1 + (16 * mt + nj) * 34;
#pragma unroll
        for (int g = 0; g < 2; g++)
            s.w1[h][g] = make_float4(row[4 * (4 * g + 0) + q], row[4 * (4 * g + 1) + q], row[4 * (4 * g + 2) + q], row[4 * (4 * g + 3) + q]);
        const int u = 16 * mt + 4 * q;
        const float4 bb = *reinterpret_cast<const float4 *>(B1 + u);
        s.c1[h] = make_float4(bb.x + W1[(u + 0) * 34 + 32], bb.y + W1[(u + 1) * 34 + 32], bb.z + W1[(u + 2) * 34 + 32], bb.w + W1[(u + 3) * 34 + 32]);
    }
#pragma unroll
    for (int mt = 0; mt < 8; mt++) s.w2[mt] = *reinterpret_cast<const float4 *>(W2 + (16 * wave + nj) * 128 + 16 * mt + 4 * q);
#pragma unroll
    for (int h = 0; h < 2; h++) s.w3[h] = *reinterpret_cast<const float4 *>(W3 + nj * 64 + 16 * ((wave & 1) + 2 * h) + 4 * q);
    s.b2 = *reinterpret_cast<const float4 *>(B2 + 16 * wave + 4 * q);
    s.b3 = *reinterpret_cast<const float4 *>(B3 + 4 * q);
}

// what a tile hands from wavefront to wavefront: the two hidden layers, layer 3's two chains, and wavefront 0's relu(adv) * mask [node][output]
struct SdTileLds {
    float4 h1[8][64], h2[4][64], o[2][64];
    float pos[16][16];
};
static_assert(sizeof(SdTileLds) == 15360, "the tile's LDS");

// ONE 16-node tile from the feature bits of lane's node (lane % 16; every wavefront passes the same bits: hand one-hot | table multi-hot << 16) to its
// regret-matching policy, positive_regret_policy (nets.py:93-101): relu(adv) * mask / max(sum, 1e-8), the mask being the hand's one-hot.  All four
// wavefronts of the workgroup call it together: it holds three workgroup barriers.  hand: the node's hand nibbles, nl: its legal actions.  Returns
// false in wavefronts 1..3, which are done with the tile; true in wavefront 0, where lane (q, node) then holds pk = policy[q] of its node in hand
// order (0 at q >= nl).  In wavefront 0 it ends with sd_order() behind its last read of pos, so the caller (or sd_tile_thresholds) may write pos
// again at once; the next tile writes h1, h2, o only past the barriers behind their last reads in this one, whatever wavefront 0 does in between.
__device__ __forceinline__ bool sd_tile_policy(const SdSlices &W, SdTileLds &s, uint32_t xbits, uint32_t hand, int nl, int wave, int lane, float &pk) {
    const int nj = lane & 15, q = lane >> 4;
    {   // layer 1: unit blocks 2 wave, 2 wave + 1
        v4f ha = to_v4f(W.c1[0]), hb = to_v4f(W.c1[1]);
        const uint32_t xs = xbits >> q;
#pragma unroll
        for (int g = 0; g < 2; g++) {
            const float x0 = (float)((xs >> (16 * g)) & 1u), x1 = (float)((xs >> (16 * g + 4)) & 1u);
            const float x2 = (float)((xs >> (16 * g + 8)) & 1u), x3 = (float)((xs >> (16 * g + 12)) & 1u);
            ha = mfma16(W.w1[0][g].x, x0, ha); hb = mfma16(W.w1[1][g].x, x0, hb);
            ha = mfma16(W.w1[0][g].y, x1, ha); hb = mfma16(W.w1[1][g].y, x1, hb);
            ha = mfma16(W.w1[0][g].z, x2, ha); hb = mfma16(W.w1[1][g].z, x2, hb);
            ha = mfma16(W.w1[0][g].w, x3, ha); hb = mfma16(W.w1[1][g].w, x3, hb);
        }
        s.h1[2 * wave][lane] = make_float4(relu(ha[0]), relu(ha[1]), relu(ha[2]), relu(ha[3]));
        s.h1[2 * wave + 1][lane] = make_float4(relu(hb[0]), relu(hb[1]), relu(hb[2]), relu(hb[3]));
    }
    __syncthreads();
    {   // layer 2: unit block `wave`
        v4f h2 = to_v4f(W.b2);
#pragma unroll
        for (int mt = 0; mt < 8; mt++) {
            const float4 a = s.h1[mt][lane];
            h2 = mfma16(W.w2[mt].x, a.x, h2);
            h2 = mfma16(W.w2[mt].y, a.y, h2);
            h2 = mfma16(W.w2[mt].z, a.z, h2);
            h2 = mfma16(W.w2[mt].w, a.w, h2);
        }
        s.h2[wave][lane] = make_float4(relu(h2[0]), relu(h2[1]), relu(h2[2]), relu(h2[3]));
    }
    __syncthreads();
    if (wave < 2) {   // layer 3: chain 0 = bias + blocks 0, 2 (wavefront 0), chain 1 = blocks 1, 3 (wavefront 1)
        v4f o = {0.0f, 0.0f, 0.0f, 0.0f};
        if (wave == 0) o = to_v4f(W.b3);
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const float4 a = s.h2[wave + 2 * h][lane];
            o = mfma16(W.w3[h].x, a.x, o);
            o = mfma16(W.w3[h].y, a.y, o);
            o = mfma16(W.w3[h].z, a.z, o);
            o = mfma16(W.w3[h].w, a.w, o);
        }
        s.o[wave][lane] = make_float4(o[0], o[1], o[2], o[3]);
    }
    __syncthreads();
    if (wave != 0) return false;
    float adv[4];
    {
        const float4 o0 = s.o[0][lane], o1 = s.o[1][lane];
        adv[0] = o0.x + o1.x; adv[1] = o0.y + o1.y; adv[2] = o0.z + o1.z; adv[3] = o0.w + o1.w;
    }
    float z = 0.0f;
    {   // lane (q, node) holds outputs 4 q .. 4 q + 3
        float4 pv;
        float *pp = &pv.x;
#pragma unroll
        for (int r = 0; r < 4; r++) { pp[r] = (((xbits >> (4 * q + r)) & 1u) && adv[r] > 0.0f) ? adv[r] : 0.0f; z += pp[r]; }
        *reinterpret_cast<float4 *>(&s.pos[nj][4 * q]) = pv;
        z = sum_row_groups(z);
    }
    const float den = z > 1e-8f ? z : 1e-8f;   // clamp_min(eps)
    sd_order();
    pk = q < nl ? s.pos[nj][(hand >> (4 * q)) & 15u] / den : 0.0f;   // lane (q, node): action q of the node, hand order
    sd_order();
    return true;
}

// What sampling from a node's float32 policy row needs.  np.random.choice(legal, p = probs / probs.sum()) (deep_cfr.py:347-365) is
// index = #{k : cdf_k / cdf_last <= u} with float32 p and a float64 cdf; every u the traversals draw is M * 2^-53 with an integer M < 2^53 (u53 of two
// Philox words), and x * 2^53 is exact in float64, so  x <= u  <=>  ceil(x * 2^53) <= M: the node's N - 1 thresholds are those integers and a visit
// compares 64-bit integers -- the same answer as the float64 compare, bit for bit, with the float32 / float64 divisions done once per node instead of
// once per visit.  pv: the policy of the nl <= N legal actions, zeros beyond.  thr[0] = ~0 marks probs.sum() == 0 (uniform choice: the visit keeps
// numpy's arithmetic for that case); thr[k] = 2^53 > every M at k >= nl - 1: never counted (cdf_k / cdf_last = 1 > u).
template <int N>
__device__ __forceinline__ void sd_thresholds(const float (&pv)[N], int nl, unsigned long long (&thr)[N - 1]) {
    float sum = pv[0];
#pragma unroll
    for (int k = 1; k < N; k++) if (k < nl) sum += pv[k];              // action_probs.sum(), float32, left to right
#pragma unroll
    for (int k = 0; k < N - 1; k++) thr[k] = 1ull << 53;
    if (sum == 0.0f) thr[0] = ~0ull;
    else {
        double cs = 0.0, cdf[N];
#pragma unroll
        for (int k = 0; k < N; k++) { const double pq = (double)(pv[k] / sum); cs = k ? cs + pq : pq; cdf[k] = cs; }   // float32 p, float64 cdf
        double last = cdf[0];
#pragma unroll
        for (int k = 1; k < N; k++) last = k < nl ? cdf[k] : last;
#pragma unroll
        for (int k = 0; k < N - 1; k++) if (k < nl - 1) thr[k] = (unsigned long long)ceil((cdf[k] / last) * 9007199254740992.0);
    }
}

// wavefront 0's tail behind sd_tile_policy: the node's four probabilities meet in lane (0, node) through the tile's pos area, and the lanes q == 0 that
// `take` get the node's thresholds (the others leave thr as it is); ends with the fence that lets the next tile reuse pos
__device__ __forceinline__ void sd_tile_thresholds(SdTileLds &s, int nl, int lane, float pk, bool take, unsigned long long (&thr)[3]) {
    const int nj = lane & 15, q = lane >> 4;
    s.pos[nj][q] = pk;
    sd_order();
    if (q == 0 && take) {
        const float4 p4 = *reinterpret_cast<const float4 *>(&s.pos[nj][0]);
        const float pv[4] = {p4.x, p4.y, p4.z, p4.w};
        sd_thresholds<4>(pv, nl, thr);
    }
    sd_order();
}
}  // namespace
