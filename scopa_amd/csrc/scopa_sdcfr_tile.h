// scopa_sdcfr_tile.h -- what a kernel that runs the 34-128-64-16 advantage net on the matrix cores needs beside its own loop: the layout of the packed
// net image (written by k_sdcfr_pack, scopa_sdcfr.hip) and the few one-instruction helpers of a 16-node tile.  Definitions only, no kernel.  Included
// by scopa_team_chance_sdcfr.hip and (for v4f and mfma16) scopa_train_tile.h; scopa_sdcfr.hip and scopa_sdcfr_avg.hip keep their own copies of these lines (their sources are fingerprinted
// against recorded profiles), and the static_assert below ties the layout to the size the public header states.
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
}  // namespace
