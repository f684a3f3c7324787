// scopa_train_tile.h -- the Deep CFR optimiser step (AdvantageNetwork.train, src/algorithms/deep_cfr/deep_cfr.py:77-116) of an In-128-64-Out ReLU MLP, stated ONCE
// for the two nets that have a hand-written step: 34-128-64-16 (scopa_train.hip) and 96-128-64-40 (scopa_full_train.hip).  Definitions only, no kernel: each of
// those files gives its net's constants, owns its kernels' names, LDS and reduce structure, and instantiates
//   train_grad_body<S>    : gather, forward, masked MSE, backward of a workgroup's 16-row tiles on v_mfma_f32_16x16x4_f32 -> one partial gradient per workgroup;
//   train_clip_coef       : clip_grad_norm_(1.0)'s coefficient from the summed gradient's 2-norm;
//   train_adam_element<S> : torch.optim.Adam's update of one parameter, in place on the net's tensors and on the [2][kParams] moment buffer;
//   train_check_args<S>, train_adam_scalars : what the two entry points refuse, and Adam's scalars in double, on the host.
// The order of every floating-point operation is part of the statement (the bias starts the accumulator, K steps ascend, one accumulator per weight-gradient tile
// across the workgroup's tiles, bias gradients summed over rows 0..15 per thread, the loss reduced by wavefront shuffles): the partials are summed in fixed order
// afterwards, so a step's bits are a function of its inputs alone.
// MFMA roles (one instruction = a 16 x 16 tile over 4 K values): A lane l = A[l % 16][l / 16], B lane l = B[l / 16][l % 16], D lane l register r = D[4 (l / 16) + r][l % 16].
#pragma once
#include <cmath>
#include <cstdio>

#include "scopa_ctx.h"
#include "scopa_sdcfr_tile.h"   // v4f, mfma16

namespace {

// A net's shape.  Net gives what is chosen per net: kIn, kOut; the LDS row strides kSX (features), kSD (d), kST (target, mask) -- odd, a wavefront reads a tile by
// rows and by columns -- and kTW1 (W1's copy: a multiple of the 2 / 4 floats it is staged by); kStridePad, the floats between a partial's gradient and the next
// partial.  The strides are stated, not derived: they change no bit, but they do change bank behaviour.
template <class Net>
struct TrainShape : Net {
    using Net::kIn;
    using Net::kOut;
    static constexpr int kH1 = 128, kH2 = 64;
    static constexpr int kS1 = 129, kS2 = 65;      // LDS row strides of h1 / dz1 and h2 / dz2 (odd)
    static constexpr int kTW2 = 132, kTW3 = 68;    // row strides of W2's and W3's LDS copies (multiples of 4 floats: staged 16 bytes at a time)
    static constexpr int kOutTiles = (kOut + 15) / 16, kOutP = 16 * kOutTiles;   // the outputs padded to whole 16-wide tiles
    static constexpr int kInTiles = (kIn + 15) / 16, kInSteps = (kIn + 3) / 4;   // 16-wide feature tiles of dW1, K steps of layer 1
    static constexpr int kOffW1 = 0, kOffB1 = kOffW1 + kH1 * kIn, kOffW2 = kOffB1 + kH1, kOffB2 = kOffW2 + kH2 * kH1, kOffW3 = kOffB2 + kH2, kOffB3 = kOffW3 + kOut * kH2;
    static constexpr int kParams = kOffB3 + kOut;          // in net.parameters() order
    static constexpr int kSlots = kParams + kOutTiles;     // a partial: the gradient, then one loss sum per output tile (wavefronts 0 .. kOutTiles - 1)
    static constexpr int kStride = kParams + Net::kStridePad;
    static_assert(kIn % 2 == 0 && kOutTiles <= 4 && kStride >= kSlots && Net::kTW1 >= kIn && Net::kSX >= kIn && Net::kSD >= kOutP && Net::kST >= kOut, "shape");
};

// The body below is optimised as a function of its own before it is inlined into a kernel, so what a kernel's own text would tell the compiler is said in
// types: the LDS regions are pointers into the LDS address space (not generic ones, found out only after inlining), and a set of accumulator tiles that is indexed
// in a loop is ONE vector value, the form the compiler gives such an array inside a kernel (as an array it is split into tiles here, and the register allocator
// then needs a quarter more registers: the wide net's kernel no longer fits two waves a SIMD).
typedef float v2f __attribute__((ext_vector_type(2)));
template <class T> using Lds = __attribute__((address_space(3))) T;
template <class T> __device__ __forceinline__ Lds<T> *lds_ptr(T *p) { return (Lds<T> *)p; }   // of a __shared__ array or a part of the dynamic segment
template <int kTiles>
struct AccTiles {      // kTiles 16 x 16 MFMA accumulators (4 registers a lane each)
    typedef float vec __attribute__((ext_vector_type(4 * kTiles)));
    vec v;
    __device__ __forceinline__ v4f get(int c) const { return v4f{v[4 * c], v[4 * c + 1], v[4 * c + 2], v[4 * c + 3]}; }
    __device__ __forceinline__ void set(int c, v4f x) {
#pragma unroll
        for (int r = 0; r < 4; r++) v[4 * c + r] = x[r];
    }
};

struct TrainLds {      // a workgroup's LDS regions (the kernel owns them)
    Lds<long long> *row;                         // [16] the tile's ring rows
    Lds<float> *w1, *w2, *w3;                    // [kH1][kTW1], [kH2][kTW2], [kOutP][kTW3] (16-byte aligned): the weights, staged once per workgroup
    Lds<float> *x, *h1, *h2, *d, *dz2, *dz1;     // [16][kSX], [16][kS1], [16][kS2], [16][kSD], [16][kS2], [16][kS1]
    Lds<float> *t, *m;                           // [16][kST] the tile's target and mask rows
};
struct TrainParams { float *w1, *b1, *w2, *b2, *w3, *b3; };   // the net's own torch tensors W[out][in], b[out]
struct AdamScalars { float step_size, bc2_sqrt, beta2, one_minus_beta1, one_minus_beta2, eps; };

// One workgroup (256 threads) of the gradient launch: tiles blockIdx.x, blockIdx.x + gridDim.x, ... of n_rows / 16; its partial goes to g_partial[blockIdx.x][kStride].
// Padded shapes cost nothing where they do not occur: every `kX % n == 0 ||` below is a compile-time constant.
template <class S>
__device__ __forceinline__ void train_grad_body(const TrainLds &s, const int64_t *g_rows, int n_rows, long long capacity, const float *g_feat, const float *g_regret, const float *g_mask,
                                                const float *W1, const float *B1, const float *W2, const float *B2, const float *W3, const float *B3, float *g_partial) {
    constexpr int kIn = S::kIn, kH1 = S::kH1, kH2 = S::kH2, kOut = S::kOut, kOutP = S::kOutP, kOutTiles = S::kOutTiles, kInTiles = S::kInTiles;
    constexpr int kSX = S::kSX, kS1 = S::kS1, kS2 = S::kS2, kSD = S::kSD, kST = S::kST, kTW1 = S::kTW1, kTW2 = S::kTW2, kTW3 = S::kTW3;
    constexpr int kL1Unroll = kIn % 4 ? S::kInSteps : 8;   // (a layer 1 with a predicated last step is unrolled whole)
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nj = lane & 15, q = lane >> 4;
    const int n_tiles = n_rows / 16;                       // (the host sends whole tiles only)
    const float dscale = 2.0f / (float)(n_rows * kOut);    // d MSE / d pred: 2 (pred m - target m) m / (rows x outputs)
    const v4f zero = {0.0f, 0.0f, 0.0f, 0.0f};
    // weight gradients, accumulated over this workgroup's tiles in MFMA accumulators: wavefront w owns
    //   dW2 rows (unit2) 16 w .. 16 w + 15, all 8 column tiles (unit1);  dW1 rows (unit1) 32 w .. 32 w + 31, every column tile (feature);  dW3 columns (unit2) 16 w .. + 15, every row tile (output)
    AccTiles<8> a_w2 = {};
    AccTiles<kOutTiles> a_w3 = {};
    v4f a_w1[2][kInTiles];
#pragma unroll
    for (int h = 0; h < 2; h++)
#pragma unroll
        for (int c = 0; c < kInTiles; c++) a_w1[h][c] = zero;
    float db1 = 0.0f, db2 = 0.0f, db3 = 0.0f, loss = 0.0f;   // thread t: bias gradients of unit t (t < 128 / 64 / kOut); loss: wavefronts 0 .. kOutTiles - 1, their output tile's share
    // the weights, staged once per workgroup with coalesced loads (as MFMA operands straight from global memory every lane read 4 bytes of its own cache line, once
    // per K step and phase); both W and W^T operands are read from the one copy.  W1's rows are whole 16 bytes only where kIn % 4 == 0.
    if constexpr (kIn % 4 != 0) {
        for (int e = tid; e < kH1 * kIn / 2; e += 256) { const int r = (2 * e) / kIn, c = 2 * e - r * kIn; *reinterpret_cast<Lds<v2f> *>(&s.w1[r * kTW1 + c]) = reinterpret_cast<const v2f *>(W1)[e]; }
    } else {
        for (int e = tid; e < kH1 * kIn / 4; e += 256) { const int r = (4 * e) / kIn, c = 4 * e - r * kIn; *reinterpret_cast<Lds<v4f> *>(&s.w1[r * kTW1 + c]) = reinterpret_cast<const v4f *>(W1)[e]; }
    }
    for (int e = tid; e < kH2 * kH1 / 4; e += 256) { const int r = (4 * e) / kH1, c = 4 * e - r * kH1; *reinterpret_cast<Lds<v4f> *>(&s.w2[r * kTW2 + c]) = reinterpret_cast<const v4f *>(W2)[e]; }
    for (int e = tid; e < kOut * kH2 / 4; e += 256) { const int r = (4 * e) / kH2, c = 4 * e - r * kH2; *reinterpret_cast<Lds<v4f> *>(&s.w3[r * kTW3 + c]) = reinterpret_cast<const v4f *>(W3)[e]; }
    // rows kOut .. kOutP - 1 do not exist in W3 (W3 [kOut][64] and b3 [kOut] end at row kOut - 1): ZERO, never loaded.  The padded outputs are dead by
    // construction (d = 0 there), so they reach neither the loss, dW3 / db3 nor dz2.
    for (int e = tid; e < (kOutP - kOut) * kTW3; e += 256) s.w3[kOut * kTW3 + e] = 0.0f;

    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        __syncthreads();                                   // the previous tile's LDS is no longer read
        if (tid < 16) { const long long r = g_rows[(size_t)tile * 16 + tid]; s.row[tid] = r < 0 ? 0 : r >= capacity ? capacity - 1 : r; }   // (a row index outside the ring is clamped, never dereferenced)
        __syncthreads();
        for (int e = tid; e < 16 * kIn; e += 256) { const int r = e / kIn, c = e - r * kIn; s.x[r * kSX + c] = g_feat[(size_t)s.row[r] * kIn + c]; }
        for (int e = tid; e < 16 * kOut; e += 256) {       // the tile's target and mask rows (not on the critical path in front of the loss); no mask array: mask = features[0..kOut) (scopa_sdcfr.hip sd_mask_note)
            const int r = e / kOut, c = e - r * kOut;
            s.t[r * kST + c] = g_regret[(size_t)s.row[r] * kOut + c];
            s.m[r * kST + c] = g_mask ? g_mask[(size_t)s.row[r] * kOut + c] : g_feat[(size_t)s.row[r] * kIn + c];
        }
        __syncthreads();
        {   // ---- layer 1: h1[unit][row] = relu(W1 x + b1) over all kIn columns (rows given through add_experience may carry anything in any of them); wavefront w: unit tiles 2 w, 2 w + 1
            v4f acc[2];
#pragma unroll
            for (int h = 0; h < 2; h++) { const float *b = B1 + 16 * (2 * w + h) + 4 * q; acc[h] = v4f{b[0], b[1], b[2], b[3]}; }
#pragma unroll kL1Unroll
            for (int st = 0; st < S::kInSteps; st++) {
                const int k = 4 * st + q;
                const bool in = kIn % 4 == 0 || k < kIn;
                const float b = in ? s.x[nj * kSX + k] : 0.0f;
#pragma unroll
                for (int h = 0; h < 2; h++) acc[h] = mfma16(in ? s.w1[(16 * (2 * w + h) + nj) * kTW1 + k] : 0.0f, b, acc[h]);
            }
#pragma unroll
            for (int h = 0; h < 2; h++)
#pragma unroll
                for (int r = 0; r < 4; r++) s.h1[nj * kS1 + 16 * (2 * w + h) + 4 * q + r] = fmaxf(acc[h][r], 0.0f);
        }
        __syncthreads();
        {   // ---- layer 2: wavefront w: unit tile w
            const float *b = B2 + 16 * w + 4 * q;
            v4f acc = {b[0], b[1], b[2], b[3]};
#pragma unroll 8
            for (int st = 0; st < kH1 / 4; st++) { const int k = 4 * st + q; acc = mfma16(s.w2[(16 * w + nj) * kTW2 + k], s.h1[nj * kS1 + k], acc); }
#pragma unroll
            for (int r = 0; r < 4; r++) s.h2[nj * kS2 + 16 * w + 4 * q + r] = fmaxf(acc[r], 0.0f);
        }
        __syncthreads();
        if (w < kOutTiles) {   // ---- layer 3, the loss and its gradient d[row][out]; wavefront w: output tile w (outputs 16 w .. 16 w + 15; kOut .. kOutP - 1 are padding)
            v4f acc;
#pragma unroll
            for (int r = 0; r < 4; r++) { const int o = 16 * w + 4 * q + r; acc[r] = (kOut % 16 == 0 || o < kOut) ? B3[o] : 0.0f; }
#pragma unroll
            for (int st = 0; st < kH2 / 4; st++) { const int k = 4 * st + q; acc = mfma16(s.w3[(16 * w + nj) * kTW3 + k], s.h2[nj * kS2 + k], acc); }
            float l = 0.0f;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int o = 16 * w + 4 * q + r;
                float dv = 0.0f;
                if (kOut % 16 == 0 || o < kOut) {
                    const float m = s.m[nj * kST + o], e = (acc[r] - s.t[nj * kST + o]) * m;   // pred * mask - target * mask
                    l += e * e;
                    dv = e * dscale * m;                                                       // d/dpred of (e e) carries the mask a second time (fractional masks)
                }
                s.d[nj * kSD + o] = dv;                                                        // (0 at the padded outputs: they reach no gradient)
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) l += __shfl_xor(l, off, 64);
            loss += l;
        }
        __syncthreads();
        {   // ---- dW3[out][unit2] += sum_row d[row][out] h2[row][unit2]   (wavefront w: unit2 tile w, every output tile);   dz2 = (W3^T d) * (h2 > 0)   (wavefront w: unit2 tile w)
#pragma unroll
            for (int st = 0; st < 4; st++) {
                const int k = 4 * st + q;                                     // row within the tile
                const float b = s.h2[k * kS2 + 16 * w + nj];
#pragma unroll
                for (int c = 0; c < kOutTiles; c++) a_w3.set(c, mfma16(s.d[k * kSD + 16 * c + nj], b, a_w3.get(c)));
            }
            v4f acc = zero;
#pragma unroll
            for (int st = 0; st < kOutP / 4; st++) {
                const int k = 4 * st + q;                                     // here k is an OUTPUT: A = W3^T[unit2][out], B = d[out][row]
                acc = mfma16(s.w3[k * kTW3 + 16 * w + nj], s.d[nj * kSD + k], acc);
            }
#pragma unroll
            for (int r = 0; r < 4; r++) { const int u = 16 * w + 4 * q + r; s.dz2[nj * kS2 + u] = s.h2[nj * kS2 + u] > 0.0f ? acc[r] : 0.0f; }
        }
        __syncthreads();
        {   // ---- dW2[unit2][unit1] += sum_row dz2[row][unit2] h1[row][unit1]   (wavefront w: unit2 tile w);   dz1 = (W2^T dz2) * (h1 > 0)   (wavefront w: unit1 tiles 2 w, 2 w + 1)
#pragma unroll
            for (int st = 0; st < 4; st++) {
                const int k = 4 * st + q;
                const float a = s.dz2[k * kS2 + 16 * w + nj];
#pragma unroll
                for (int c = 0; c < 8; c++) a_w2.set(c, mfma16(a, s.h1[k * kS1 + 16 * c + nj], a_w2.get(c)));
            }
            v4f acc[2] = {zero, zero};
#pragma unroll 4
            for (int st = 0; st < kH2 / 4; st++) {
                const int k = 4 * st + q;                                     // unit2
                const float b = s.dz2[nj * kS2 + k];
#pragma unroll
                for (int h = 0; h < 2; h++) acc[h] = mfma16(s.w2[k * kTW2 + 16 * (2 * w + h) + nj], b, acc[h]);
            }
#pragma unroll
            for (int h = 0; h < 2; h++)
#pragma unroll
                for (int r = 0; r < 4; r++) { const int u = 16 * (2 * w + h) + 4 * q + r; s.dz1[nj * kS1 + u] = s.h1[nj * kS1 + u] > 0.0f ? acc[h][r] : 0.0f; }
        }
        __syncthreads();
        {   // ---- dW1[unit1][feature] += sum_row dz1[row][unit1] x[row][feature]   (wavefront w: unit1 tiles 2 w, 2 w + 1, every feature tile); bias gradients
#pragma unroll
            for (int st = 0; st < 4; st++) {
                const int k = 4 * st + q;
                const float a0 = s.dz1[k * kS1 + 16 * (2 * w) + nj], a1 = s.dz1[k * kS1 + 16 * (2 * w + 1) + nj];
#pragma unroll
                for (int c = 0; c < kInTiles; c++) {
                    const int f = 16 * c + nj;
                    const float b = (kIn % 16 == 0 || f < kIn) ? s.x[k * kSX + f] : 0.0f;
                    a_w1[0][c] = mfma16(a0, b, a_w1[0][c]);
                    a_w1[1][c] = mfma16(a1, b, a_w1[1][c]);
                }
            }
#pragma unroll
            for (int r = 0; r < 16; r++) {
                if (tid < kH1) db1 += s.dz1[r * kS1 + tid];
                if (tid < kH2) db2 += s.dz2[r * kS2 + tid];
                if (tid < kOut) db3 += s.d[r * kSD + tid];
            }
        }
    }
    // ---- this workgroup's partial gradient (net.parameters() order) and partial loss
    float *out = g_partial + (size_t)blockIdx.x * S::kStride;
#pragma unroll
    for (int h = 0; h < 2; h++)
#pragma unroll
        for (int c = 0; c < kInTiles; c++)
#pragma unroll
            for (int r = 0; r < 4; r++) { const int u = 16 * (2 * w + h) + 4 * q + r, f = 16 * c + nj; if (kIn % 16 == 0 || f < kIn) out[S::kOffW1 + u * kIn + f] = a_w1[h][c][r]; }
#pragma unroll
    for (int c = 0; c < 8; c++)
#pragma unroll
        for (int r = 0; r < 4; r++) out[S::kOffW2 + (16 * w + 4 * q + r) * kH1 + 16 * c + nj] = a_w2.get(c)[r];
#pragma unroll
    for (int c = 0; c < kOutTiles; c++)
#pragma unroll
        for (int r = 0; r < 4; r++) { const int o = 16 * c + 4 * q + r; if (kOut % 16 == 0 || o < kOut) out[S::kOffW3 + o * kH2 + 16 * w + nj] = a_w3.get(c)[r]; }
    if (tid < kH1) out[S::kOffB1 + tid] = db1;
    if (tid < kH2) out[S::kOffB2 + tid] = db2;
    if (tid < kOut) out[S::kOffB3 + tid] = db3;
    if (lane == 0 && w < kOutTiles) out[S::kParams + w] = loss;
}

// clip_grad_norm_(max_norm = 1.0): clip_coef = max_norm / (total_norm + 1e-6), clamped to 1
__device__ __forceinline__ float train_clip_coef(float norm) {
    const float inv = 1.0f / (norm + 1e-6f);
    return inv < 1.0f ? inv : 1.0f;
}

// torch.optim.Adam's update (bias-corrected, eps outside the square root) of parameter i of the flat order, from its clipped gradient gr
template <class S>
__device__ __forceinline__ void train_adam_element(int i, float gr, const TrainParams &t, float *__restrict__ g_state /* [2][kParams] */, const AdamScalars &a) {
    float *p = i < S::kOffB1 ? t.w1 + (i - S::kOffW1) : i < S::kOffW2 ? t.b1 + (i - S::kOffB1) : i < S::kOffB2 ? t.w2 + (i - S::kOffW2) : i < S::kOffW3 ? t.b2 + (i - S::kOffB2)
             : i < S::kOffB3 ? t.w3 + (i - S::kOffW3) : t.b3 + (i - S::kOffB3);
    const float m = g_state[i] + (gr - g_state[i]) * a.one_minus_beta1;                        // exp_avg.lerp_(grad, 1 - beta1)
    const float v = g_state[S::kParams + i] * a.beta2 + a.one_minus_beta2 * gr * gr;           // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
    g_state[i] = m;
    g_state[S::kParams + i] = v;
    *p = *p - a.step_size * (m / (sqrtf(v) / a.bc2_sqrt + a.eps));                             // param.addcdiv_(exp_avg, denom, value = -step_size)
}

// ---- host ----
struct TrainArgs {   // what scopa_sdcfr_train_steps and scopa_full_sdcfr_train_steps take after the context (include/scopa.h)
    const int64_t *d_rows; int32_t n_rows, n_steps; const float *d_feat, *d_regret, *d_mask; int64_t capacity; TrainParams p; float *d_state; int32_t first_step; float lr; float *d_loss;
};

// What both entry points refuse, in their order: SCOPA_OK, or the code with the message in ctx->err under the entry point's name
template <class S>
inline int32_t train_check_args(scopa_ctx *ctx, const char *name, const TrainArgs &a) {
    if (!ctx || !a.d_rows || !a.d_feat || !a.d_regret || !a.p.w1 || !a.p.b1 || !a.p.w2 || !a.p.b2 || !a.p.w3 || !a.p.b3 || !a.d_state || !a.d_loss) return SCOPA_EINVAL;
    char msg[256];
    const auto refuse = [&](const char *what) { snprintf(msg, sizeof msg, "%s: %s", name, what); return scopa::fail(ctx, SCOPA_EINVAL, msg); };
    if (!(a.n_rows >= 16 && a.n_rows % 16 == 0 && a.n_rows <= (1 << 20))) return refuse("the batch must be a multiple of 16 rows (16 .. 2^20)");
    if (!(a.capacity >= 1 && a.first_step >= 1 && a.n_steps >= 0 && a.n_steps <= 4096 && a.lr > 0.0f))
        return refuse("capacity, first_step (1-based) and lr must be positive, n_steps in 0 .. 4096");
    constexpr uintptr_t w1_align = S::kIn % 4 ? 7 : 15;
    if (!(((uintptr_t)a.p.w1 & w1_align) == 0 && ((uintptr_t)a.p.w2 & 15) == 0 && ((uintptr_t)a.p.w3 & 15) == 0))
        return refuse(S::kIn % 4 ? "the weight tensors are staged 8 / 16 bytes at a time: d_w1 must be 8-byte, d_w2 / d_w3 16-byte aligned"
                                 : "the weight tensors are staged 16 bytes at a time: d_w1, d_w2 and d_w3 must be 16-byte aligned");
    return SCOPA_OK;
}

// torch.optim.Adam's scalars (_single_tensor_adam) for step e of a call: bias_correction1 = 1 - beta1 ** step, step_size = lr / bias_correction1,
// bias_correction2_sqrt = sqrt(1 - beta2 ** step) in Python floats (float64), rounded to float32 only where they meet the tensors -- computed the same way here
// (in-kernel powf on float32 betas was ~1e-5 off at small steps); so are 1 - beta1 and 1 - beta2 (1 - 0.999f in float32 is 1.3e-5 below 0.001: exp_avg_sq that
// much low, every update 6.5e-6 too large)
inline AdamScalars train_adam_scalars(int32_t first_step, int e, float lr) {
    const double step = (double)first_step + (double)e, bc1 = 1.0 - std::pow(0.9, step), bc2 = 1.0 - std::pow(0.999, step);
    return {(float)((double)lr / bc1), (float)std::sqrt(bc2), 0.999f, (float)(1.0 - 0.9), (float)(1.0 - 0.999), 1e-8f};
}

}  // namespace
