// scopa_full_train.hip -- one optimiser step of FullScopa's 96-128-64-40 advantage net (FullChanceDeepCFR, train_backend="hip") in THREE launches.
//
// The semantics are scopa_train.hip's (AdvantageNetwork._step): gather n_rows ring rows, forward, loss = mean over n_rows x 40 of (pred m - target m)^2, backward
// (the mask enters d/dpred a second time), clip_grad_norm_(1.0) with min(1, 1 / (norm + 1e-6)), torch.optim.Adam's update with its scalars computed on the host in double.
//   k_full_train_grad   : a workgroup (4 wavefronts) per group of 16-row tiles, at most 256 workgroups (one per CU: 135 KB of LDS each).  Forward and backward of a tile on
//                         v_mfma_f32_16x16x4_f32, activations in LDS ([row][unit], odd strides), the weights staged there once per workgroup from the net's own torch
//                         tensors W[out][in] (16-byte loads; W and W^T operands are read from the one copy).  Layer 3 has 40 outputs in three 16-wide tiles: W3's LDS
//                         rows 40..47 are ZERO-FILLED (W3 [40][64] and b3 [40] end at row 39: nothing beyond is loaded), and outputs 40..47 are dead by construction
//                         (d = 0 there), so they reach neither the loss, dW3 / db3 nor dz2; the gradient scale is 2 / (n_rows x 40).  All 96 input columns take part
//                         in layer 1 and in dW1 (rows given through add_experience may carry anything in columns 92..95).  The weight gradients accumulate in MFMA
//                         accumulators across the workgroup's tiles (dW1 48, dW2 32, dW3 12 registers per lane) and leave as ONE partial per workgroup.
//   k_full_train_reduce : 364 workgroups, 64 consecutive elements each: wavefront s sums the s-th quarter of the partials in ascending order, the four quarter sums are
//                         added in order; the summed gradient, the three loss sums and one sum of squares per workgroup go to memory.  No float atomics anywhere: the
//                         order of every sum is a function of (n_rows) alone, so two runs from one state give the same bits.
//   k_full_train_adam   : 91 workgroups: each adds the 364 sums of squares in the same fixed order (so all agree on the norm), then clips and applies Adam to its 256 elements
//                         in place on the net's tensors and on the [2][23272] moment buffer.
// The reduce / Adam stage is two launches, not scopa_train.hip's one workgroup, because a batch of thousands of rows leaves 256 partials of 93 KB: summed by one
// workgroup that is a 24 MB serial read; spread over the machine it is a few microseconds.
// MFMA roles (one instruction = a 16 x 16 tile over 4 K values): A lane l = A[l % 16][l / 16], B lane l = B[l / 16][l % 16], D lane l register r = D[4 (l / 16) + r][l % 16].
#include <cmath>

#include "scopa_ctx.h"

using namespace scopa;

namespace {
constexpr int kIn = 96, kH1 = 128, kH2 = 64, kOut = 40, kOutP = 48;   // kOutP: the outputs padded to whole 16-wide tiles
constexpr int kOffW1 = 0, kOffB1 = kOffW1 + kH1 * kIn, kOffW2 = kOffB1 + kH1, kOffB2 = kOffW2 + kH2 * kH1, kOffW3 = kOffB2 + kH2, kOffB3 = kOffW3 + kOut * kH2;
constexpr int kParams = kOffB3 + kOut;   // 23 272, in net.parameters() order
static_assert(kParams == 23272, "parameter count of the 96-128-64-40 MLP");
constexpr int kMaxPartials = 256;        // one workgroup per CU
constexpr int kSlots = kParams + 3;      // a partial: the gradient, then the loss sums of wavefronts 0..2 (an output tile each)
constexpr int kStride = kParams + 4;     // ... padded to whole 16 bytes
constexpr int kRedBlocks = (kSlots + 63) / 64;     // 364
constexpr int kAdamBlocks = (kParams + 255) / 256; // 91
constexpr int kSX = 97, kS1 = 129, kS2 = 65, kSD = 49, kST = 41;   // LDS row strides (floats), odd: a wavefront reads a tile by rows and by columns
constexpr int kTW1 = 100, kTW2 = 132, kTW3 = 68;                    // row strides of the weights' LDS copies (multiples of 4 floats: they are staged 16 bytes at a time)
// the workgroup's LDS (floats from the start of the dynamic segment); the weights' offsets are multiples of 4
constexpr int kLRow = 0, kLW1 = 32, kLW2 = kLW1 + kH1 * kTW1, kLW3 = kLW2 + kH2 * kTW2, kLX = kLW3 + kOutP * kTW3, kLH1 = kLX + 16 * kSX, kLH2 = kLH1 + 16 * kS1,
              kLD = kLH2 + 16 * kS2, kLDz2 = kLD + 16 * kSD, kLDz1 = kLDz2 + 16 * kS2, kLT = kLDz1 + 16 * kS1, kLM = kLT + 16 * kST, kLdsFloats = kLM + 16 * kST;
static_assert(kLW1 % 4 == 0 && kLW2 % 4 == 0 && kLW3 % 4 == 0, "16-byte staging of the weights");
constexpr int kLdsBytes = kLdsFloats * 4;   // 137 600
static_assert(kLdsBytes <= 160 * 1024, "one workgroup's LDS");

typedef float v4f __attribute__((ext_vector_type(4)));
__device__ __forceinline__ v4f mfma(float a, float b, v4f c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
}  // namespace

__global__ void __launch_bounds__(256)
k_full_train_grad(const int64_t *__restrict__ g_rows, int n_rows, long long capacity, const float *__restrict__ g_feat, const float *__restrict__ g_regret, const float *__restrict__ g_mask,
                  const float *__restrict__ W1, const float *__restrict__ B1, const float *__restrict__ W2, const float *__restrict__ B2,
                  const float *__restrict__ W3, const float *__restrict__ B3, float *__restrict__ g_partial /* [gridDim.x][kStride] */) {
    extern __shared__ __align__(16) float s_mem[];
    long long *s_row = reinterpret_cast<long long *>(s_mem + kLRow);   // [16]
    float *s_w1 = s_mem + kLW1, *s_w2 = s_mem + kLW2, *s_w3 = s_mem + kLW3;   // the weights, staged once per workgroup
    float *s_x = s_mem + kLX, *s_h1 = s_mem + kLH1, *s_h2 = s_mem + kLH2, *s_d = s_mem + kLD, *s_dz2 = s_mem + kLDz2, *s_dz1 = s_mem + kLDz1;
    float *s_t = s_mem + kLT, *s_m = s_mem + kLM;                      // the tile's target and mask rows [16][40]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nj = lane & 15, q = lane >> 4;
    const int n_tiles = n_rows / 16;                       // (the host sends whole tiles only)
    const float dscale = 2.0f / (float)(n_rows * kOut);    // d MSE / d pred: 2 (pred m - target m) m / (rows x 40)
    const v4f zero = {0.0f, 0.0f, 0.0f, 0.0f};
    // weight gradients, accumulated over this workgroup's tiles in MFMA accumulators: wavefront w owns
    //   dW2 rows (unit2) 16 w .. 16 w + 15, all 8 column tiles (unit1);  dW1 rows (unit1) 32 w .. 32 w + 31, 6 column tiles (feature);  dW3 columns (unit2) 16 w .. + 15, 3 row tiles (output)
    v4f a_w2[8], a_w1[2][6], a_w3[3];
#pragma unroll
    for (int i = 0; i < 8; i++) a_w2[i] = zero;
#pragma unroll
    for (int h = 0; h < 2; h++)
#pragma unroll
        for (int c = 0; c < 6; c++) a_w1[h][c] = zero;
#pragma unroll
    for (int c = 0; c < 3; c++) a_w3[c] = zero;
    float db1 = 0.0f, db2 = 0.0f, db3 = 0.0f, loss = 0.0f;   // thread t: bias gradients of unit t (t < 128 / 64 / 40); loss: wavefronts 0..2, their output tile's share
    for (int e = tid; e < kH1 * kIn / 4; e += 256) { const int r = (4 * e) / kIn, c = 4 * e - r * kIn; *reinterpret_cast<float4 *>(&s_w1[r * kTW1 + c]) = reinterpret_cast<const float4 *>(W1)[e]; }
    for (int e = tid; e < kH2 * kH1 / 4; e += 256) { const int r = (4 * e) / kH1, c = 4 * e - r * kH1; *reinterpret_cast<float4 *>(&s_w2[r * kTW2 + c]) = reinterpret_cast<const float4 *>(W2)[e]; }
    for (int e = tid; e < kOut * kH2 / 4; e += 256) { const int r = (4 * e) / kH2, c = 4 * e - r * kH2; *reinterpret_cast<float4 *>(&s_w3[r * kTW3 + c]) = reinterpret_cast<const float4 *>(W3)[e]; }
    for (int e = tid; e < (kOutP - kOut) * kTW3; e += 256) s_w3[kOut * kTW3 + e] = 0.0f;   // rows 40..47 do not exist in W3: zero, never loaded

    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        __syncthreads();                                   // the previous tile's LDS is no longer read
        if (tid < 16) { const long long r = g_rows[(size_t)tile * 16 + tid]; s_row[tid] = r < 0 ? 0 : r >= capacity ? capacity - 1 : r; }   // (a row index outside the ring is clamped, never dereferenced)
        __syncthreads();
        for (int e = tid; e < 16 * kIn; e += 256) { const int r = e / kIn, c = e - r * kIn; s_x[r * kSX + c] = g_feat[(size_t)s_row[r] * kIn + c]; }
        for (int e = tid; e < 16 * kOut; e += 256) {       // no mask array: mask = features[0..40) (DeviceMemory's rule for num_actions = 40)
            const int r = e / kOut, c = e - r * kOut;
            s_t[r * kST + c] = g_regret[(size_t)s_row[r] * kOut + c];
            s_m[r * kST + c] = g_mask ? g_mask[(size_t)s_row[r] * kOut + c] : g_feat[(size_t)s_row[r] * kIn + c];
        }
        __syncthreads();
        {   // ---- layer 1: h1[unit][row] = relu(W1 x + b1) over all 96 columns; wavefront w: unit tiles 2 w, 2 w + 1
            v4f acc[2];
#pragma unroll
            for (int h = 0; h < 2; h++) { const float *b = B1 + 16 * (2 * w + h) + 4 * q; acc[h] = v4f{b[0], b[1], b[2], b[3]}; }
#pragma unroll 8
            for (int s = 0; s < kIn / 4; s++) {
                const int k = 4 * s + q;
                const float b = s_x[nj * kSX + k];
#pragma unroll
                for (int h = 0; h < 2; h++) acc[h] = mfma(s_w1[(16 * (2 * w + h) + nj) * kTW1 + k], b, acc[h]);
            }
#pragma unroll
            for (int h = 0; h < 2; h++)
#pragma unroll
                for (int r = 0; r < 4; r++) s_h1[nj * kS1 + 16 * (2 * w + h) + 4 * q + r] = fmaxf(acc[h][r], 0.0f);
        }
        __syncthreads();
        {   // ---- layer 2: wavefront w: unit tile w
            const float *b = B2 + 16 * w + 4 * q;
            v4f acc = {b[0], b[1], b[2], b[3]};
#pragma unroll 8
            for (int s = 0; s < 32; s++) { const int k = 4 * s + q; acc = mfma(s_w2[(16 * w + nj) * kTW2 + k], s_h1[nj * kS1 + k], acc); }
#pragma unroll
            for (int r = 0; r < 4; r++) s_h2[nj * kS2 + 16 * w + 4 * q + r] = fmaxf(acc[r], 0.0f);
        }
        __syncthreads();
        if (w < 3) {   // ---- layer 3, the loss and its gradient d[row][out]; wavefront w: output tile w (outputs 16 w .. 16 w + 15; 40..47 are padding)
            v4f acc;
#pragma unroll
            for (int r = 0; r < 4; r++) { const int o = 16 * w + 4 * q + r; acc[r] = o < kOut ? B3[o] : 0.0f; }
#pragma unroll
            for (int s = 0; s < 16; s++) { const int k = 4 * s + q; acc = mfma(s_w3[(16 * w + nj) * kTW3 + k], s_h2[nj * kS2 + k], acc); }
            float l = 0.0f;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int o = 16 * w + 4 * q + r;
                float dv = 0.0f;
                if (o < kOut) {
                    const float m = s_m[nj * kST + o], e = (acc[r] - s_t[nj * kST + o]) * m;   // pred * mask - target * mask
                    l += e * e;
                    dv = e * dscale * m;                                                         // d/dpred of (e e) carries the mask a second time (fractional masks)
                }
                s_d[nj * kSD + o] = dv;                                                          // (0 at the padded outputs: they reach no gradient)
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) l += __shfl_xor(l, off, 64);
            loss += l;
        }
        __syncthreads();
        {   // ---- dW3[out][unit2] += sum_row d[row][out] h2[row][unit2]   (wavefront w: unit2 tile w, 3 output tiles);   dz2 = (W3^T d) * (h2 > 0)   (wavefront w: unit2 tile w)
#pragma unroll
            for (int s = 0; s < 4; s++) {
                const int k = 4 * s + q;                                      // row within the tile
                const float b = s_h2[k * kS2 + 16 * w + nj];
#pragma unroll
                for (int c = 0; c < 3; c++) a_w3[c] = mfma(s_d[k * kSD + 16 * c + nj], b, a_w3[c]);
            }
            v4f acc = zero;
#pragma unroll
            for (int s = 0; s < kOutP / 4; s++) {
                const int k = 4 * s + q;                                      // here k is an OUTPUT: A = W3^T[unit2][out], B = d[out][row]
                acc = mfma(s_w3[k * kTW3 + 16 * w + nj], s_d[nj * kSD + k], acc);
            }
#pragma unroll
            for (int r = 0; r < 4; r++) { const int u = 16 * w + 4 * q + r; s_dz2[nj * kS2 + u] = s_h2[nj * kS2 + u] > 0.0f ? acc[r] : 0.0f; }
        }
        __syncthreads();
        {   // ---- dW2[unit2][unit1] += sum_row dz2[row][unit2] h1[row][unit1]   (wavefront w: unit2 tile w);   dz1 = (W2^T dz2) * (h1 > 0)   (wavefront w: unit1 tiles 2 w, 2 w + 1)
#pragma unroll
            for (int s = 0; s < 4; s++) {
                const int k = 4 * s + q;
                const float a = s_dz2[k * kS2 + 16 * w + nj];
#pragma unroll
                for (int c = 0; c < 8; c++) a_w2[c] = mfma(a, s_h1[k * kS1 + 16 * c + nj], a_w2[c]);
            }
            v4f acc[2] = {zero, zero};
#pragma unroll 4
            for (int s = 0; s < 16; s++) {
                const int k = 4 * s + q;                                      // unit2
                const float b = s_dz2[nj * kS2 + k];
#pragma unroll
                for (int h = 0; h < 2; h++) acc[h] = mfma(s_w2[k * kTW2 + 16 * (2 * w + h) + nj], b, acc[h]);
            }
#pragma unroll
            for (int h = 0; h < 2; h++)
#pragma unroll
                for (int r = 0; r < 4; r++) { const int u = 16 * (2 * w + h) + 4 * q + r; s_dz1[nj * kS1 + u] = s_h1[nj * kS1 + u] > 0.0f ? acc[h][r] : 0.0f; }
        }
        __syncthreads();
        {   // ---- dW1[unit1][feature] += sum_row dz1[row][unit1] x[row][feature]   (wavefront w: unit1 tiles 2 w, 2 w + 1, all 6 feature tiles); bias gradients
#pragma unroll
            for (int s = 0; s < 4; s++) {
                const int k = 4 * s + q;
                const float a0 = s_dz1[k * kS1 + 16 * (2 * w) + nj], a1 = s_dz1[k * kS1 + 16 * (2 * w + 1) + nj];
#pragma unroll
                for (int c = 0; c < 6; c++) {
                    const float b = s_x[k * kSX + 16 * c + nj];
                    a_w1[0][c] = mfma(a0, b, a_w1[0][c]);
                    a_w1[1][c] = mfma(a1, b, a_w1[1][c]);
                }
            }
#pragma unroll
            for (int r = 0; r < 16; r++) {
                if (tid < kH1) db1 += s_dz1[r * kS1 + tid];
                if (tid < kH2) db2 += s_dz2[r * kS2 + tid];
                if (tid < kOut) db3 += s_d[r * kSD + tid];
            }
        }
    }
    // ---- this workgroup's partial gradient (net.parameters() order) and partial loss
    float *out = g_partial + (size_t)blockIdx.x * kStride;
#pragma unroll
    for (int h = 0; h < 2; h++)
#pragma unroll
        for (int c = 0; c < 6; c++)
#pragma unroll
            for (int r = 0; r < 4; r++) out[kOffW1 + (16 * (2 * w + h) + 4 * q + r) * kIn + 16 * c + nj] = a_w1[h][c][r];
#pragma unroll
    for (int c = 0; c < 8; c++)
#pragma unroll
        for (int r = 0; r < 4; r++) out[kOffW2 + (16 * w + 4 * q + r) * kH1 + 16 * c + nj] = a_w2[c][r];
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int r = 0; r < 4; r++) { const int o = 16 * c + 4 * q + r; if (o < kOut) out[kOffW3 + o * kH2 + 16 * w + nj] = a_w3[c][r]; }
    if (tid < kH1) out[kOffB1 + tid] = db1;
    if (tid < kH2) out[kOffB2 + tid] = db2;
    if (tid < kOut) out[kOffB3 + tid] = db3;
    if (lane == 0 && w < 3) out[kParams + w] = loss;
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
    const float norm = sqrtf(((s_red[0] + s_red[1]) + s_red[2]) + s_red[3]);
    const float inv = 1.0f / (norm + 1e-6f), coef = inv < 1.0f ? inv : 1.0f;   // clip_grad_norm_(max_norm = 1.0): clip_coef = max_norm / (total_norm + 1e-6), clamped to 1
    if (i < kParams) {
        float *p = i < kOffB1 ? W1 + (i - kOffW1) : i < kOffW2 ? B1 + (i - kOffB1) : i < kOffB2 ? W2 + (i - kOffW2) : i < kOffW3 ? B2 + (i - kOffB2) : i < kOffB3 ? W3 + (i - kOffW3) : B3 + (i - kOffB3);
        const float gr = g_sum[i] * coef;
        const float m = g_state[i] + (gr - g_state[i]) * one_minus_beta1;                  // exp_avg.lerp_(grad, 1 - beta1)
        const float v = g_state[kParams + i] * beta2 + one_minus_beta2 * gr * gr;          // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
        g_state[i] = m;
        g_state[kParams + i] = v;
        *p = *p - step_size * (m / (sqrtf(v) / bc2_sqrt + eps));                          // param.addcdiv_(exp_avg, denom, value = -step_size)
    }
    if (i == 0) g_loss[0] += ((g_sum[kParams] + g_sum[kParams + 1]) + g_sum[kParams + 2]) / (float)(n_rows * kOut);   // this step's MSE, added to the caller's running sum
}

extern "C" {

int32_t scopa_full_sdcfr_train_params(void) { return kParams; }

int32_t scopa_full_sdcfr_train_steps(scopa_ctx *ctx, const int64_t *d_rows, int32_t n_rows, int32_t n_steps, const float *d_feat, const float *d_regret, const float *d_mask,
                                     int64_t capacity, float *d_w1, float *d_b1, float *d_w2, float *d_b2, float *d_w3, float *d_b3, float *d_state, int32_t first_step, float lr,
                                     float *d_loss) {
    if (!ctx || !d_rows || !d_feat || !d_regret || !d_w1 || !d_b1 || !d_w2 || !d_b2 || !d_w3 || !d_b3 || !d_state || !d_loss) return SCOPA_EINVAL;
    SC_REQUIRE(ctx, n_rows >= 16 && n_rows % 16 == 0 && n_rows <= (1 << 20), SCOPA_EINVAL, "scopa_full_sdcfr_train_steps: the batch must be a multiple of 16 rows (16 .. 2^20)");
    SC_REQUIRE(ctx, capacity >= 1 && first_step >= 1 && n_steps >= 0 && n_steps <= 4096 && lr > 0.0f, SCOPA_EINVAL,
               "scopa_full_sdcfr_train_steps: capacity, first_step (1-based) and lr must be positive, n_steps in 0 .. 4096");
    SC_REQUIRE(ctx, ((uintptr_t)d_w1 & 15) == 0 && ((uintptr_t)d_w2 & 15) == 0 && ((uintptr_t)d_w3 & 15) == 0, SCOPA_EINVAL,
               "scopa_full_sdcfr_train_steps: the weight tensors are staged 16 bytes at a time: d_w1, d_w2 and d_w3 must be 16-byte aligned");
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
        // torch.optim.Adam's scalars in double, rounded to float32 only where they meet the tensors; so are 1 - beta1 and 1 - beta2 (scopa_train.hip says why)
        const double step = (double)first_step + (double)e, bc1 = 1.0 - std::pow(0.9, step), bc2 = 1.0 - std::pow(0.999, step);
        hipLaunchKernelGGL(k_full_train_adam, dim3(kAdamBlocks), dim3(256), 0, ctx->stream, (const float *)sum, (const float *)sq, (int)n_rows, d_w1, d_b1, d_w2, d_b2, d_w3, d_b3,
                           d_state, (float)((double)lr / bc1), (float)std::sqrt(bc2), 0.999f, (float)(1.0 - 0.9), (float)(1.0 - 0.999), 1e-8f, d_loss);
    }
    SC_HIP(ctx, hipGetLastError());
    return SCOPA_OK;
}

}  // extern "C"
