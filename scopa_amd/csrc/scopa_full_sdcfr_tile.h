// scopa_full_sdcfr_tile.h -- what a kernel that runs FullScopa's 96-128-64-40 advantage net on the matrix cores needs beside its own loop: the 96
// features of a key pair, and the register slices of one player's net that a workgroup of four wavefronts keeps resident while it loops over 16-node
// tiles.  Definitions only, no kernel.  The one-instruction helpers of a tile (mfma16, relu, sd_order, v4f) are scopa_sdcfr_tile.h's, which is
// included and left as it is.  Included by scopa_full_chance_sdcfr.hip.
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

}  // namespace
