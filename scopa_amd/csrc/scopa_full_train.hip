// scopa_full_train.hip -- one optimiser step of FullScopa's 96-128-64-40 advantage net (FullChanceDeepCFR, train_backend="hip") in THREE launches.
//
// The semantics and the math are scopa_train.hip's, stated once in scopa_train_tile.h; here are the wide net's constants, its kernels and its reduce structure:
//   k_full_train_grad   : a workgroup (4 wavefronts) per group of 16-row tiles, at most 256 workgroups (one per CU: 135 KB of LDS each, the dynamic segment):
//                         train_grad_body.  96 inputs: whole K steps and feature tiles, all 96 columns take part in layer 1 and in dW1 (rows given through
//                         add_experience may carry anything in columns 92..95), W1 staged 16 bytes at a time; 40 outputs in three 16-wide tiles on wavefronts
//                         0..2: W3's LDS rows 40..47 are zero-filled and outputs 40..47 dead; the gradient scale is 2 / (n_rows x 40).  The weight gradients
//                         (dW1 48, dW2 32, dW3 12 registers per lane) leave as ONE partial per workgroup.
//   k_full_train_reduce : 364 workgroups, 64 consecutive elements each: wavefront s sums the s-th quarter of the partials in ascending order, the four quarter sums are
//                         added in order; the summed gradient, the three loss sums and one sum of squares per workgroup go to memory.  No float atomics anywhere: the
//                         order of every sum is a function of (n_rows) alone, so two runs from one state give the same bits.
//   k_full_train_adam   : 91 workgroups: each adds the 364 sums of squares in the same fixed order (so all agree on the norm), then clips and applies Adam to its 256 elements
//                         in place on the net's tensors and on the [2][23272] moment buffer.
// The reduce / Adam stage is two launches, not scopa_train.hip's one workgroup, because a batch of thousands of rows leaves 256 partials of 93 KB: summed by one
// workgroup that is a 24 MB serial read; spread over the machine it is a few microseconds.
#include "scopa_train_tile.h"

using namespace scopa;

namespace {
struct WideNet { static constexpr int kIn = 96, kOut = 40, kSX = 97, kSD = 49, kST = 41, kTW1 = 100, kStridePad = 4; };   // kStridePad: the three loss slots, padded to whole 16 bytes
using S = TrainShape<WideNet>;
static_assert(S::kParams == 23272 && S::kOutTiles == 3, "parameter count and output tiles of the 96-128-64-40 MLP");
constexpr int kParams = S::kParams, kSlots = S::kSlots, kStride = S::kStride;
constexpr int kMaxPartials = 256;        // one workgroup per CU
constexpr int kRedBlocks = (kSlots + 63) / 64;     // 364
constexpr int kAdamBlocks = (kParams + 255) / 256; // 91
// the workgroup's LDS (floats from the start of the dynamic segment); the weights' offsets are multiples of 4
constexpr int kLRow = 0, kLW1 = 32, kLW2 = kLW1 + S::kH1 * S::kTW1, kLW3 = kLW2 + S::kH2 * S::kTW2, kLX = kLW3 + S::kOutP * S::kTW3, kLH1 = kLX + 16 * S::kSX, kLH2 = kLH1 + 16 * S::kS1,
              kLD = kLH2 + 16 * S::kS2, kLDz2 = kLD + 16 * S::kSD, kLDz1 = kLDz2 + 16 * S::kS2, kLT = kLDz1 + 16 * S::kS1, kLM = kLT + 16 * S::kST, kLdsFloats = kLM + 16 * S::kST;
static_assert(kLW1 % 4 == 0 && kLW2 % 4 == 0 && kLW3 % 4 == 0, "16-byte staging of the weights");
constexpr int kLdsBytes = kLdsFloats * 4;
static_assert(kLdsBytes == 137600 && kLdsBytes <= 160 * 1024, "one workgroup's LDS");
}  // namespace

__global__ void __launch_bounds__(256)
k_full_train_grad(const int64_t *__restrict__ g_rows, int n_rows, long long capacity, const float *__restrict__ g_feat, const float *__restrict__ g_regret, const float *__restrict__ g_mask,
                  const float *__restrict__ W1, const float *__restrict__ B1, const float *__restrict__ W2, const float *__restrict__ B2,
                  const float *__restrict__ W3, const float *__restrict__ B3, float *__restrict__ g_partial /* [gridDim.x][kStride] */) {
    extern __shared__ __align__(16) float s_mem[];
    Lds<float> *const m = lds_ptr(s_mem);
    train_grad_body<S>(TrainLds{lds_ptr(reinterpret_cast<long long *>(s_mem + kLRow)), m + kLW1, m + kLW2, m + kLW3, m + kLX, m + kLH1, m + kLH2, m + kLD, m + kLDz2, m + kLDz1, m + kLT, m + kLM},
                       g_rows, n_rows, capacity, g_feat, g_regret, g_mask, W1, B1, W2, B2, W3, B3, g_partial);
}

__global__ void __launch_bounds__(256)
k_full_train_reduce(const float *__restrict__ g_partial, int n_partials, float *__restrict__ g_sum /* [kStride] */, float *__restrict__ g_sq /* [kRedBlocks] */) {
    __shared__ float s_seg[4][64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, i = blockIdx.x * 64 + lane;
    const int per = (n_partials + 3) / 4, p0 = w * per, p1 = p0 + per < n_partials ? p0 + per : n_partials;   // wavefront w: partials p0 .. p1 - 1, in ascending order
    float acc = 0.0f;
    if (i < kSlots) {
        int p = p0;
        for (; p + 8 <= p1; p += 8) {   // eight loads in flight, added in order
            float t[8];
#pragma unroll
            for (int u = 0; u < 8; u++) t[u] = g_partial[(size_t)(p + u) * kStride + i];
#pragma unroll
            for (int u = 0; u < 8; u++) acc += t[u];
        }
        for (; p < p1; p++) acc += g_partial[(size_t)p * kStride + i];
    }
    s_seg[w][lane] = acc;
    __syncthreads();
    if (w == 0) {
        const float g = ((s_seg[0][lane] + s_seg[1][lane]) + s_seg[2][lane]) + s_seg[3][lane];
        if (i < kSlots) g_sum[i] = g;
        float sq = i < kParams ? g * g : 0.0f;   // (the loss slots are not part of the gradient)
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) sq += __shfl_xor(sq, off, 64);
        if (lane == 0) g_sq[blockIdx.x] = sq;
    }
}

__global__ void __launch_bounds__(256)
k_full_train_adam(const float *__restrict__ g_sum, const float *__restrict__ g_sq, int n_rows, float *__restrict__ W1, float *__restrict__ B1, float *__restrict__ W2,
                  float *__restrict__ B2, float *__restrict__ W3, float *__restrict__ B3, float *__restrict__ g_state /* [2][kParams] */, float step_size, float bc2_sqrt,
                  float beta2, float one_minus_beta1, float one_minus_beta2, float eps, float *__restrict__ g_loss) {
    __shared__ float s_red[4];
    const int tid = threadIdx.x, i = blockIdx.x * 256 + tid;
    float sq = 0.0f;   // every workgroup adds the same 364 values in the same order: they all get the same norm
    for (int k = tid; k < kRedBlocks; k += 256) sq += g_sq[k];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sq += __shfl_xor(sq, off, 64);
    if ((tid & 63) == 0) s_red[tid >> 6] = sq;
    __syncthreads();
    const float coef = train_clip_coef(sqrtf(((s_red[0] + s_red[1]) + s_red[2]) + s_red[3]));
    if (i < kParams)
        train_adam_element<S>(i, g_sum[i] * coef, TrainParams{W1, B1, W2, B2, W3, B3}, g_state, AdamScalars{step_size, bc2_sqrt, beta2, one_minus_beta1, one_minus_beta2, eps});
    if (i == 0) g_loss[0] += ((g_sum[kParams] + g_sum[kParams + 1]) + g_sum[kParams + 2]) / (float)(n_rows * S::kOut);   // this step's MSE, added to the caller's running sum
}

extern "C" {

int32_t scopa_full_sdcfr_train_params(void) { return kParams; }

int32_t scopa_full_sdcfr_train_steps(scopa_ctx *ctx, const int64_t *d_rows, int32_t n_rows, int32_t n_steps, const float *d_feat, const float *d_regret, const float *d_mask,
                                     int64_t capacity, float *d_w1, float *d_b1, float *d_w2, float *d_b2, float *d_w3, float *d_b3, float *d_state, int32_t first_step, float lr,
                                     float *d_loss) {
    const int32_t rc = train_check_args<S>(ctx, "scopa_full_sdcfr_train_steps", {d_rows, n_rows, n_steps, d_feat, d_regret, d_mask, capacity, {d_w1, d_b1, d_w2, d_b2, d_w3, d_b3}, d_state, first_step, lr, d_loss});
    if (rc != SCOPA_OK) return rc;
    SC_REQUIRE(ctx, kLdsBytes <= ctx->lds_limit, SCOPA_EINVAL, "scopa_full_sdcfr_train_steps: a workgroup keeps the net and a tile in 137 600 bytes of LDS");
    if (n_steps == 0) return SCOPA_OK;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    scopa::Range range_("scopa full sdcfr train");
    // [256 partials][kStride] | the summed gradient and loss [kStride] | the reduce workgroups' sums of squares [364]
    if (!ctx->d_full_train_partial) SC_HIP(ctx, hipMalloc(&ctx->d_full_train_partial, sizeof(float) * ((size_t)(kMaxPartials + 1) * kStride + kRedBlocks)));
    SC_LDS_ATTR(ctx, kLdsFullTrain, k_full_train_grad, kLdsBytes);
    float *partial = (float *)ctx->d_full_train_partial, *sum = partial + (size_t)kMaxPartials * kStride, *sq = sum + kStride;
    const int n_tiles = n_rows / 16, grid = n_tiles < kMaxPartials ? n_tiles : kMaxPartials;
    for (int e = 0; e < n_steps; e++) {
        hipLaunchKernelGGL(k_full_train_grad, dim3(grid), dim3(256), kLdsBytes, ctx->stream, d_rows + (size_t)e * n_rows, (int)n_rows, (long long)capacity, d_feat, d_regret, d_mask,
                           (const float *)d_w1, (const float *)d_b1, (const float *)d_w2, (const float *)d_b2, (const float *)d_w3, (const float *)d_b3, partial);
        hipLaunchKernelGGL(k_full_train_reduce, dim3(kRedBlocks), dim3(256), 0, ctx->stream, (const float *)partial, grid, sum, sq);
        const AdamScalars a = train_adam_scalars(first_step, e, lr);
        hipLaunchKernelGGL(k_full_train_adam, dim3(kAdamBlocks), dim3(256), 0, ctx->stream, (const float *)sum, (const float *)sq, (int)n_rows, d_w1, d_b1, d_w2, d_b2, d_w3, d_b3,
                           d_state, a.step_size, a.bc2_sqrt, a.beta2, a.one_minus_beta1, a.one_minus_beta2, a.eps, d_loss);
    }
    SC_HIP(ctx, hipGetLastError());
    return SCOPA_OK;
}

}  // extern "C"
