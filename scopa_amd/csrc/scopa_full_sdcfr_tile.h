// scopa_full_sdcfr_tile.h -- what a kernel that runs FullScopa's 96-128-64-40 advantage net on the matrix cores needs beside its own loop: the 96
// features of a key pair, and the register slices of one player's net that a workgroup of four wavefronts keeps resident while it loops over 16-node
// tiles, and the body of ONE such tile from the key pairs of 16 nodes to their policy[3] and thresholds[2] (fsd_tile_policy, fsd_tile_thresholds),
// which the forest's policy kernel and the list kernel both call.  Definitions only, no kernel.  The one-instruction helpers of a tile (mfma16, relu,
// sd_order, v4f) and the threshold rule (sd_thresholds) are scopa_sdcfr_tile.h's, the narrow net's header.  Included by scopa_full_chance_sdcfr.hip.
//
//   features  96 float32, a function of the mover's key pair (A, B) alone, every value dyadic (so exact in float32):
//               [0, 40)  the hand, one-hot by card id (word B) -- also the legal-action mask      [40, 80)  the table, multi-hot (A bits 16..55)
//               [80, 86) the round, one-hot        86  the mover's captured-card field / 64        87, 88  the mover's, the opponent's scopas / 32
//               89       1.0 if the player bit 62 is set                                            [90, 96)  0
//   tile      v_mfma_f32_16x16x4_f32 with the WEIGHTS as the 16 x 4 operand (16 output units) and the 16 NODES as the columns: lane (q, nj) = (lane / 16,
//             lane % 16) supplies weight W[unit nj of the block][input 4 s + q] and input 4 s + q of node nj, and holds outputs 4 q + r (r = 0..3) of node
//             nj.  A column's result depends on its own node and the weights alone: which nodes share a tile changes no bit.
//   K order   the order in which a unit's terms are accumulated is fixed: the accumulator starts at the bias; layer 1 adds steps s = 0 .. 22 in ascending
//             order, step s holding inputs 4 s .. 4 s + 3 (step 23, inputs 92..95, is skipped: they are 0 by definition, so W1's columns 92..95 are never
//             read); layer 2 adds the 128 hidden units in blocks of 16 ascending, within a block the four instructions r = 0..3 holding units
//             16 mt + 4 q + r over q; layer 3 the 64 units the same way.  Within one instruction the four products are added by the hardware in its own
//             fixed order.  Layer 3 is padded from 40 to 48 outputs with zero weights and biases.
#pragma once
#include "scopa_sdcfr_tile.h"

namespace {

constexpr int kFsdIn = SCOPA_FULL_SDCFR_FEATURES, kFsdH1 = 128, kFsdH2 = 64, kFsdOut = SCOPA_FULL_SDCFR_ACTIONS, kFsdOutPad = 48;
constexpr int kFsdSteps1 = 23;            // layer-1 steps of four inputs: inputs 0..91
static_assert(kFsdIn == 96 && kFsdOut == 40, "include/scopa.h states the net's shape");

// feature f of the key pair (a, b)
__host__ __device__ __forceinline__ float fsd_feature(uint64_t a, uint64_t b, int f) {
    if (f < 40) return (float)((b >> f) & 1ull);
    if (f < 80) return (float)((a >> (16 + (f - 40))) & 1ull);
    const int player = (int)((a >> 62) & 1ull);
    if (f < 86) return (int)((a >> 59) & 7ull) == f - 80 ? 1.0f : 0.0f;
    const uint32_t s0 = (uint32_t)((a >> 5) & 31ull), s1 = (uint32_t)(a & 31ull);
    if (f == 86) return (float)((a >> 10) & 63ull) / 64.0f;
    if (f == 87) return (float)(player ? s1 : s0) / 32.0f;
    if (f == 88) return (float)(player ? s0 : s1) / 32.0f;
    if (f == 89) return (float)player;
    return 0.0f;
}

// one player's net, torch layout W[out][in]
struct FsdNet { const float *w1, *b1, *w2, *b2, *w3, *b3; };

// the slices wavefront `wave` of four keeps in registers (110 floats a lane): layer 1 unit blocks 2 wave, 2 wave + 1; layer 2 unit block `wave`; layer 3
// output block `wave` (wavefronts 0..2; the fourth computes no third layer and finishes the tile instead)
struct FsdSlices {
    float w1[2][kFsdSteps1];
    float4 c1[2], w2[8], b2, w3[4], b3;
};

__device__ __forceinline__ void fsd_load_slices(const FsdNet &net, int wave, int lane, FsdSlices &s) {
    const int nj = lane & 15, q = lane >> 4;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int mt = 2 * wave + h;
        const float *row = net.w1 + (size_t)(16 * mt + nj) * kFsdIn + q;
#pragma unroll
        for (int st = 0; st < kFsdSteps1; st++) s.w1[h][st] = row[4 * st];
        const float *b = net.b1 + 16 * mt + 4 * q;
        s.c1[h] = make_float4(b[0], b[1], b[2], b[3]);
    }
#pragma unroll
    for (int mt = 0; mt < 8; mt++) {
        const float *w = net.w2 + (size_t)(16 * wave + nj) * kFsdH1 + 16 * mt + 4 * q;
        s.w2[mt] = make_float4(w[0], w[1], w[2], w[3]);
    }
    {
        const float *b = net.b2 + 16 * wave + 4 * q;
        s.b2 = make_float4(b[0], b[1], b[2], b[3]);
    }
    const int ob = wave < 3 ? wave : 2;   // (the fourth wavefront's copy is never used)
    const int unit = 16 * ob + nj;
#pragma unroll
    for (int h = 0; h < 4; h++) {
        s.w3[h] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (unit < kFsdOut) {
            const float *w = net.w3 + (size_t)unit * kFsdH2 + 16 * h + 4 * q;
            s.w3[h] = make_float4(w[0], w[1], w[2], w[3]);
        }
    }
    float b3[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int o = 16 * ob + 4 * q + r;
        b3[r] = o < kFsdOut ? net.b3[o] : 0.0f;
    }
    s.b3 = make_float4(b3[0], b3[1], b3[2], b3[3]);
}

// what a tile hands from wavefront to wavefront: the two hidden layers, the 40 (of 48) advantages of the 16 nodes, and the finishing wavefront's slots
struct FsdTileLds {
    float4 h1[8][64], h2[4][64];
    alignas(16) float adv[16][52];        // written 16 bytes at a time
    float pos[16][4];
};

// ONE 16-node tile from the key pair of lane's node (lane % 16; every wavefront passes the same pairs) to its policy, for the two kernels that run the
// net (k_full_chance_sdcfr_policy over a forest, k_full_chance_sdcfr_policy_at over a list).  All four wavefronts of the workgroup call it together:
// it holds three workgroup barriers.  nl: the node's held cards.  Returns false in wavefronts 0..2, which are done with the tile; true in the
// fourth, where lane (q, node) then holds pk = policy[q] of its node (0 at q >= nl).  The next tile writes h1, h2, adv only past the barriers behind
// their last reads in this one: the fourth wavefront joins them after its tail.
__device__ __forceinline__ bool fsd_tile_policy(const FsdSlices &W, FsdTileLds &s, uint64_t A, uint64_t B, int nl, int wave, int lane, float &pk) {
    const int nj = lane & 15, q = lane >> 4;
    {   // layer 1: unit blocks 2 wave, 2 wave + 1; steps 0..19 are the 80 card bits, 20..22 the scalars
        v4f ha = to_v4f(W.c1[0]), hb = to_v4f(W.c1[1]);
        const uint64_t table = (A >> 16) & ((1ull << 40) - 1ull);
        const uint64_t lo = (B | (table << 40)) >> q, hi = (table >> 24) >> q;   // features 0..63, 64..79, seen from input 4 s + q
#pragma unroll
        for (int st = 0; st < 16; st++) {
            const float x = (float)((lo >> (4 * st)) & 1ull);
            ha = mfma16(W.w1[0][st], x, ha); hb = mfma16(W.w1[1][st], x, hb);
        }
#pragma unroll
        for (int st = 16; st < 20; st++) {
            const float x = (float)((hi >> (4 * (st - 16))) & 1ull);
            ha = mfma16(W.w1[0][st], x, ha); hb = mfma16(W.w1[1][st], x, hb);
        }
#pragma unroll
        for (int st = 20; st < kFsdSteps1; st++) {
            const float x = fsd_feature(A, B, 4 * st + q);
            ha = mfma16(W.w1[0][st], x, ha); hb = mfma16(W.w1[1][st], x, hb);
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
    if (wave < 3) {   // layer 3: output block `wave` of the 48, one chain from the bias through the four hidden blocks
        v4f o = to_v4f(W.b3);
#pragma unroll
        for (int h = 0; h < 4; h++) {
            const float4 a = s.h2[h][lane];
            o = mfma16(W.w3[h].x, a.x, o);
            o = mfma16(W.w3[h].y, a.y, o);
            o = mfma16(W.w3[h].z, a.z, o);
            o = mfma16(W.w3[h].w, a.w, o);
        }
        *reinterpret_cast<float4 *>(&s.adv[nj][16 * wave + 4 * q]) = make_float4(o[0], o[1], o[2], o[3]);
    }
    __syncthreads();
    if (wave != 3) return false;
    // lane (q, node): slot q of the node = its q-th held card in ascending card id
    int card = 0;
    {
        uint64_t rest = B;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int cb = rest ? __ffsll((long long)rest) - 1 : 0;
            if (k == q) card = cb;
            rest &= rest - 1ull;
        }
    }
    const float adv = q < nl ? s.adv[nj][card] : 0.0f;
    const float x = (q < nl && adv > 0.0f) ? adv : 0.0f;      // relu(adv) * mask
    if (q < 3) s.pos[nj][q] = x;
    sd_order();
    float z = s.pos[nj][0] + s.pos[nj][1];
    if (nl > 2) z = z + s.pos[nj][2];                          // left to right over the held cards
    const float den = z > 1e-8f ? z : 1e-8f;                   // clamp_min(float32(1e-8))
    pk = q < nl ? x / den : 0.0f;
    sd_order();
    return true;
}

// the fourth wavefront's tail behind fsd_tile_policy: the sampling thresholds of the node's float32 policy, in the lanes q == 0 that `take`
// (the others leave thr as it is); ends with the fence that lets the next tile reuse pos
__device__ __forceinline__ void fsd_tile_thresholds(FsdTileLds &s, int nl, int lane, float pk, bool take, unsigned long long (&thr)[2]) {
    const int nj = lane & 15, q = lane >> 4;
    if (q < 3) s.pos[nj][q] = pk;
    sd_order();
    if (q == 0 && take) {
        const float pv[3] = {s.pos[nj][0], s.pos[nj][1], s.pos[nj][2]};
        sd_thresholds<3>(pv, nl, thr);
    }
    sd_order();
}

}  // namespace
