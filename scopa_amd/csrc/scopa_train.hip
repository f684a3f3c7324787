// scopa_train.hip -- one optimiser step of the advantage net (AdvantageNetwork.train, src/algorithms/deep_cfr/deep_cfr.py:77-116) in TWO launches.
//
// The reference's step on a 128-row batch -- gather, 34-128-64-16 MLP forward, MSE(pred * mask, target * mask), backward, clip_grad_norm_(1.0), Adam(5e-4) --
// is about thirty dependent PyTorch kernels of 4-5 us each whatever they compute.  The default stays PyTorch (north_star: "the SDCFR
// advantage MLP trains on PyTorch-ROCm"); this file is the OPT-IN alternative (`DeepCFR(train_backend="hip")`), measured beside it.  The math is
// scopa_train_tile.h's, shared with scopa_full_train.hip; here are the narrow net's constants, its kernels and its reduce structure:
//   k_sdcfr_train_grad : a workgroup per group of 16-row tiles, at most 32: train_grad_body on 87 168 bytes of static LDS; ONE partial gradient per workgroup
//                        (summed later in fixed order: the result does not depend on scheduling).  34 inputs: layer 1's ninth K step and dW1's third feature
//                        tile are predicated, W1 is staged 8 bytes at a time; 16 outputs: one output tile, nothing padded;
//   k_sdcfr_train_adam : one workgroup: sums the partials in order, 2-norm of the whole gradient, clip coefficient, Adam's update in place on the net's tensors
//                        and on the [2][13776] moment buffer.
#include "scopa_train_tile.h"

using namespace scopa;

namespace {
struct NarrowNet { static constexpr int kIn = 34, kOut = 16, kSX = 37, kSD = 17, kST = 17, kTW1 = 36, kStridePad = 1; };
using S = TrainShape<NarrowNet>;
static_assert(S::kParams == 13776, "parameter count of the 34-128-64-16 MLP");
constexpr int kParams = S::kParams, kMaxPartials = 32;
}  // namespace

__global__ void __launch_bounds__(256)
k_sdcfr_train_grad(const int64_t *__restrict__ g_rows, int n_rows, long long capacity, const float *__restrict__ g_feat, const float *__restrict__ g_regret, const float *__restrict__ g_mask,
                   const float *__restrict__ W1, const float *__restrict__ B1, const float *__restrict__ W2, const float *__restrict__ B2,
                   const float *__restrict__ W3, const float *__restrict__ B3, float *__restrict__ g_partial /* [gridDim.x][kStride] */) {
    __shared__ float s_x[16 * S::kSX], s_h1[16 * S::kS1], s_h2[16 * S::kS2], s_d[16 * S::kSD], s_dz2[16 * S::kS2], s_dz1[16 * S::kS1];
    __shared__ __align__(16) float s_w1[S::kH1 * S::kTW1], s_w2[S::kH2 * S::kTW2], s_w3[S::kOutP * S::kTW3];
    __shared__ float s_t[16 * S::kST], s_m[16 * S::kST];
    __shared__ long long s_row[16];
    train_grad_body<S>(TrainLds{lds_ptr(s_row), lds_ptr(s_w1), lds_ptr(s_w2), lds_ptr(s_w3), lds_ptr(s_x), lds_ptr(s_h1), lds_ptr(s_h2), lds_ptr(s_d), lds_ptr(s_dz2), lds_ptr(s_dz1), lds_ptr(s_t), lds_ptr(s_m)}, g_rows, n_rows, capacity, g_feat, g_regret, g_mask, W1, B1, W2, B2, W3, B3, g_partial);
}

__global__ void __launch_bounds__(1024)
k_sdcfr_train_adam(const float *__restrict__ g_partial, int n_partials, int n_rows, float *__restrict__ W1, float *__restrict__ B1, float *__restrict__ W2,
                   float *__restrict__ B2, float *__restrict__ W3, float *__restrict__ B3, float *__restrict__ g_state /* [2][kParams] */, float step_size, float bc2_sqrt,
                   float beta2, float one_minus_beta1, float one_minus_beta2, float eps, float *__restrict__ g_loss) {
    __shared__ float s_red[16];
    const int tid = threadIdx.x;
    constexpr int kPer = (kParams + 1023) / 1024;   // 14
    static_assert(kPer == 14, "the partial sums below go in two halves of seven");
    float g[kPer], sq = 0.0f;
    // the partials summed in order, eight per pass: their loads (14 elements x 8 partials per thread) are independent and in flight together -- as a loop over
    // a run-time count the 112 loads of a thread went out one after the other (35 us of a 50 us step)
#pragma unroll
    for (int j = 0; j < kPer; j++) g[j] = 0.0f;
    for (int p0 = 0; p0 < n_partials; p0 += 8) {
#pragma unroll
        for (int jh = 0; jh < kPer; jh += 7) {          // seven elements x eight partials = 56 loads in flight per thread (all fourteen at once spilled registers)
            float t[7][8];
#pragma unroll
            for (int j = 0; j < 7; j++) {
                const int i = tid + 1024 * (jh + j);
#pragma unroll
                for (int u = 0; u < 8; u++) t[j][u] = (i < kParams && p0 + u < n_partials) ? g_partial[(size_t)(p0 + u) * S::kStride + i] : 0.0f;
            }
#pragma unroll
            for (int j = 0; j < 7; j++)
#pragma unroll
                for (int u = 0; u < 8; u++) g[jh + j] += t[j][u];
        }
    }
#pragma unroll
    for (int j = 0; j < kPer; j++) sq += g[j] * g[j];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sq += __shfl_xor(sq, off, 64);
    if ((tid & 63) == 0) s_red[tid >> 6] = sq;
    __syncthreads();
    float tot = 0.0f;
#pragma unroll
    for (int k = 0; k < 16; k++) tot += s_red[k];
    const float coef = train_clip_coef(sqrtf(tot));
    const TrainParams params{W1, B1, W2, B2, W3, B3};
    const AdamScalars adam{step_size, bc2_sqrt, beta2, one_minus_beta1, one_minus_beta2, eps};
#pragma unroll
    for (int j = 0; j < kPer; j++) {
        const int i = tid + 1024 * j;
        if (i < kParams) train_adam_element<S>(i, g[j] * coef, params, g_state, adam);
    }
    if (tid == 0) {
        float l = 0.0f;
        for (int p = 0; p < n_partials; p++) l += g_partial[(size_t)p * S::kStride + kParams];
        g_loss[0] += l / (float)(n_rows * S::kOut);                                       // this step's MSE, added to the caller's running sum
    }
}

extern "C" {

int32_t scopa_sdcfr_train_params(void) { return kParams; }

int32_t scopa_sdcfr_train_steps(scopa_ctx *ctx, const int64_t *d_rows, int32_t n_rows, int32_t n_steps, const float *d_feat, const float *d_regret, const float *d_mask,
                                int64_t capacity, float *d_w1, float *d_b1, float *d_w2, float *d_b2, float *d_w3, float *d_b3, float *d_state, int32_t first_step, float lr,
                                float *d_loss) {
    const int32_t rc = train_check_args<S>(ctx, "scopa_sdcfr_train_steps", {d_rows, n_rows, n_steps, d_feat, d_regret, d_mask, capacity, {d_w1, d_b1, d_w2, d_b2, d_w3, d_b3}, d_state, first_step, lr, d_loss});
    if (rc != SCOPA_OK || n_steps == 0) return rc;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    scopa::Range range_("scopa sdcfr train");
    if (!ctx->d_train_partial) SC_HIP(ctx, hipMalloc(&ctx->d_train_partial, sizeof(float) * (size_t)kMaxPartials * S::kStride));
    const int n_tiles = n_rows / 16, grid = n_tiles < kMaxPartials ? n_tiles : kMaxPartials;
    for (int e = 0; e < n_steps; e++) {
        hipLaunchKernelGGL(k_sdcfr_train_grad, dim3(grid), dim3(256), 0, ctx->stream, d_rows + (size_t)e * n_rows, (int)n_rows, (long long)capacity, d_feat, d_regret, d_mask, (const float *)d_w1,
                           (const float *)d_b1, (const float *)d_w2, (const float *)d_b2, (const float *)d_w3, (const float *)d_b3, (float *)ctx->d_train_partial);
        const AdamScalars a = train_adam_scalars(first_step, e, lr);
        hipLaunchKernelGGL(k_sdcfr_train_adam, dim3(1), dim3(1024), 0, ctx->stream, (const float *)ctx->d_train_partial, grid, (int)n_rows, d_w1, d_b1, d_w2, d_b2, d_w3, d_b3,
                           d_state, a.step_size, a.bc2_sqrt, a.beta2, a.one_minus_beta1, a.one_minus_beta2, a.eps, d_loss);
    }
    SC_HIP(ctx, hipGetLastError());
    return SCOPA_OK;
}

int32_t scopa_sdcfr_train_step(scopa_ctx *ctx, const int64_t *d_rows, int32_t n_rows, const float *d_feat, const float *d_regret, const float *d_mask, int64_t capacity,
                               float *d_w1, float *d_b1, float *d_w2, float *d_b2, float *d_w3, float *d_b3, float *d_state, int32_t step, float lr, float *d_loss) {
    return scopa_sdcfr_train_steps(ctx, d_rows, n_rows, 1, d_feat, d_regret, d_mask, capacity, d_w1, d_b1, d_w2, d_b2, d_w3, d_b3, d_state, step, lr, d_loss);
}

}  // extern "C"
