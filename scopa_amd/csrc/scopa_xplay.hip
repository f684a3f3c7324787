// scopa_xplay.hip -- what two tabular policies do to each other on the deal's tree: the exact cross-play matrix of K policies, the best
// responses themselves (the table k_exploitability computes and discards), and the sampled seat-swapped match with a policy in both seats.
//
// Policies are [n_infosets][4] float64 tables in hand order, used as given (no normalisation; a non-finite entry propagates by IEEE rules).
// Every float64 sum runs in a fixed order -- children left to right from 0.0; an infoset's nodes in ply order from 0.0 -- the orders of
// k_exploitability (scopa_eval.hip: the passes themselves are scopa_tree_passes.h's, one definition for both files) and of the oracle, so results
// are bit-identical from run to run and to tests/xplay_ref.py.
#include <algorithm>

#include "scopa_ctx.h"
#include "scopa_philox.h"
#include "scopa_tree_passes.h"

using namespace scopa;

// =====================================================================================================================
// Cross-play: workgroup (a, b) = blockIdx.x / n_pol, blockIdx.x % n_pol plays policy a in seat 0 against policy b in seat 1.  The combined table
// (a's rows at player-0 infosets, b's at player-1 infosets) sits in LDS; four quantities -- seat 0's reward, its square, the scopas of either
// seat -- are set at the 576 terminals and carried up the eight plies, v = 0.0; v += row[c] * child[c], children left to right: pass 2 of
// k_exploitability, four times over.  No reach pass: only two adjacent levels are alive at a time, [quantity][node] each.
__global__ void __launch_bounds__(kXWidth)
k_cross_play(const uint16_t *__restrict__ g_infoset, const int8_t *__restrict__ g_payoff, const uint64_t *__restrict__ g_key,
             const scopa_state *__restrict__ tree_states, const double *__restrict__ g_policies /*[n_pol][I][4]*/, int n_pol, int n_infosets,
             double *__restrict__ g_out /*[n_pol][n_pol][4]*/) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int I = n_infosets, tid = threadIdx.x, nt = blockDim.x;
    const int pa = (int)blockIdx.x / n_pol, pb = (int)blockIdx.x - pa * n_pol;
    double *s_pol = reinterpret_cast<double *>(smem);          // [I][4]
    double *s_lvl = s_pol + (size_t)I * 4;                     // [2][4][kXWidth]
    uint16_t *s_inf = reinterpret_cast<uint16_t *>(s_lvl + 2 * 4 * kXWidth);   // [kDecision]
    const double *pol_a = g_policies + (size_t)pa * I * 4, *pol_b = g_policies + (size_t)pb * I * 4;
    for (int cell = tid; cell < I * 4; cell += nt) s_pol[cell] = (g_key[cell >> 2] & 1) ? pol_b[cell] : pol_a[cell];
    for (int i = tid; i < kDecision; i += nt) s_inf[i] = g_infoset[i];
    const int cur = cross_play_levels(s_pol, s_lvl, s_inf, g_payoff, tree_states, tid, nt);
    if (tid < 4) g_out[(size_t)blockIdx.x * 4 + tid] = s_lvl[cur * 4 * kXWidth + tid * kXWidth];
}

// =====================================================================================================================
// Best responses: workgroup (k, p) = blockIdx.x / 2, blockIdx.x % 2 runs best_response_pass(p) on policy k -- the function k_exploitability runs
// three times -- and keeps the choices: g_br[k][p] is policy k with player p's rows replaced by the one-hot rows of the choices.  Workgroup (k, 0)
// also runs the plain value pass.  out4[k][1 + p] = BR_p, out4[k][3] = value; k_best_response_mean then fills out4[k][0].
__global__ void __launch_bounds__(1024)
k_best_response(const uint16_t *__restrict__ g_infoset, const int8_t *__restrict__ g_payoff, const uint64_t *__restrict__ g_key,
                const double *__restrict__ g_policies /*[n_pol][I][4]*/, int n_infosets, double *__restrict__ g_br /*[n_pol][2][I][4] or null*/,
                double *__restrict__ g_out4 /*[n_pol][4]*/) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int I = n_infosets, tid = threadIdx.x, nt = blockDim.x;
    const int k = (int)blockIdx.x >> 1, br_player = (int)blockIdx.x & 1;
    double *s_pol = reinterpret_cast<double *>(smem);   // [I][4]
    double *s_q = s_pol + (size_t)I * 4;                // [I][4]
    double *s_reach = s_q + (size_t)I * 4;              // [kNodes] BFS order
    double *s_val = s_reach + kNodes;                   // [kNodes]
    int *s_choice = reinterpret_cast<int *>(s_val + kNodes);  // [I]
    uint16_t *s_inf = reinterpret_cast<uint16_t *>(s_choice + I);  // [kDecision]
    const double *policy = g_policies + (size_t)k * I * 4;
    double *out4 = g_out4 + (size_t)k * 4;
    for (int cell = tid; cell < I * 4; cell += nt) s_pol[cell] = policy[cell];
    for (int i = tid; i < kDecision; i += nt) s_inf[i] = g_infoset[i];
    __syncthreads();

    for (int pass = br_player; pass < 3; pass += 2) {   // workgroup 0: passes 0 and 2 (nobody best-responds); workgroup 1: pass 1
        const int br = pass;
        best_response_pass(br, g_payoff, g_key, I, s_pol, s_q, s_reach, s_val, s_choice, s_inf, tid, nt);
        if (tid == 0) out4[1 + pass] = s_val[0];
        if (pass < 2 && g_br) {   // every infoset of the responder belongs to exactly one of its plies: all its choices are set
            double *tab = g_br + ((size_t)k * 2 + pass) * I * 4;
            for (int cell = tid; cell < I * 4; cell += nt) {
                const int r = cell >> 2;
                tab[cell] = (int)(g_key[r] & 1) == br ? ((cell & 3) == s_choice[r] ? 1.0 : 0.0) : s_pol[cell];
            }
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) k_best_response_mean(double *__restrict__ g_out4, int n_pol) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n_pol) g_out4[k * 4] = 0.5 * (g_out4[k * 4 + 1] + g_out4[k * 4 + 2]);
}

// =====================================================================================================================
// Pair match.  Thresholds of both tables in one launch: policy_thresholds (scopa_tree_passes.h) per row, as in k_eval_thresholds (scopa_eval.hip).
__global__ void __launch_bounds__(256)
k_pair_thresholds(const uint64_t *__restrict__ g_key, const double *__restrict__ policy_a, const double *__restrict__ policy_b, int n_infosets,
                  unsigned long long *__restrict__ thr /*[2][I][3]*/) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2 * n_infosets) return;
    const int which = t >= n_infosets, r = t - which * n_infosets;
    policy_thresholds((int)((g_key[r] >> 1) & 7), (which ? policy_b : policy_a) + (size_t)r * 4, thr + (size_t)t * 3);
}

// The seat-swapped match of k_eval_tabular_match with a policy in both seats: the same walk over node indices, the same Philox stream (episode, ply,
// stream_id; seed), every ply sampled by integer compares.  A workgroup serves ONE seat half -- workgroups [0, blocks0) the episodes [0, n_seat0) with
// policy a in seat 0, the others the rest with a in seat 1 -- so the table it stages is the half's combined one (the seat-h policy's thresholds at
// player-h infosets): one table in LDS, as in the sibling, and no per-episode choice between two.  stats[half][0..4] from a's point of view.
__global__ void __launch_bounds__(256)
k_eval_pair_match(long long n, long long n_seat0, int blocks0, const uint16_t *__restrict__ g_infoset, const uint64_t *__restrict__ g_key,
                  const unsigned long long *__restrict__ g_thr /*[2][I][3]*/, int n_infosets, const scopa_state *__restrict__ tree_states,
                  uint32_t seed_lo, uint32_t seed_hi, uint32_t stream, int32_t *__restrict__ out_idx, unsigned long long *__restrict__ stats /*[2][5]*/) {
    extern __shared__ __align__(16) unsigned char smem[];
    unsigned long long *s_thr = reinterpret_cast<unsigned long long *>(smem);                 // [n_infosets][3]
    uint16_t *s_inf = reinterpret_cast<uint16_t *>(smem + (size_t)n_infosets * 24);           // [kDecision]
    __shared__ unsigned long long s_stats[5];
    const int seat = (int)blockIdx.x >= blocks0;    // a's seat in this workgroup's half
    for (int t = threadIdx.x; t < n_infosets * 3; t += blockDim.x) {
        const int player = (int)(g_key[t / 3] & 1);
        s_thr[t] = g_thr[(player == seat ? (size_t)0 : (size_t)n_infosets * 3) + t];
    }
    for (int t = threadIdx.x; t < kDecision; t += blockDim.x) s_inf[t] = g_infoset[t];
    if (threadIdx.x < 5) s_stats[threadIdx.x] = 0ull;
    __syncthreads();
    const long long first = seat ? n_seat0 : 0, end = seat ? n : n_seat0;
    const long long block = seat ? (long long)blockIdx.x - blocks0 : (long long)blockIdx.x;
    const long long stride = (long long)(seat ? (int)gridDim.x - blocks0 : blocks0) * blockDim.x;
    long long acc[5] = {0, 0, 0, 0, 0};
    for (long long i = first + block * blockDim.x + threadIdx.x; i < end; i += stride) {
        int idx = 0;
#pragma unroll
        for (int ply = 0; ply < 6; ply++) {   // plies 6 and 7 have one legal card and draw nothing
            const int nl = nlegal_at(ply);
            const philox_out x = philox4x32_10((uint32_t)i, (uint32_t)(i >> 32), (uint32_t)ply, stream, seed_lo, seed_hi);
            const unsigned long long *t = s_thr + (size_t)s_inf[level_offset(ply) + idx] * 3;
            const unsigned long long N = ((unsigned long long)(x.x0 >> 5) << 26) | (unsigned long long)(x.x1 >> 6);   // u = N * 2^-53
            const int a = (int)(t[0] <= N) + (int)(t[1] <= N) + (int)(t[2] <= N);
            idx = idx * nl + (a < nl - 1 ? a : nl - 1);
        }
        const uint32_t tw = reinterpret_cast<const uint4 *>(tree_states)[kDecision + idx].w;
        const int r0 = (int)(tw & 255u) + 2 * (int)((tw >> 16) & 255u), r1 = (int)((tw >> 8) & 255u) + 2 * (int)(tw >> 24);
        const int mine = seat ? r1 - r0 : r0 - r1;
        acc[0] += 1; acc[1] += mine; acc[2] += mine * mine;
        acc[3] += (int)((tw >> (16 + 8 * seat)) & 255u); acc[4] += (int)((tw >> (24 - 8 * seat)) & 255u);
        if (out_idx) out_idx[i] = idx;
    }
#pragma unroll
    for (int j = 0; j < 5; j++) {
        long long v = acc[j];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if ((threadIdx.x & 63) == 0 && v != 0) atomicAdd(&s_stats[j], (unsigned long long)v);
    }
    __syncthreads();
    if (threadIdx.x < 5 && s_stats[threadIdx.x] != 0ull) atomicAdd(&stats[seat * 5 + threadIdx.x], s_stats[threadIdx.x]);
}

extern "C" {

int32_t scopa_cross_play(scopa_ctx *ctx, int32_t n_pol, const double *d_policies, double *d_out) {
    if (!ctx || !d_policies || !d_out || n_pol < 1 || n_pol > 256) return SCOPA_EINVAL;
    SC_REQUIRE(ctx, ctx->has_deal, SCOPA_ESTATE, "scopa_cross_play: no deal set");
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t lds = cross_play_lds(ctx->n_infosets);
    SC_REQUIRE(ctx, lds <= (size_t)ctx->lds_limit, SCOPA_ELIMIT, "scopa_cross_play: tables do not fit in LDS");
    SC_LDS_ATTR(ctx, scopa::kLdsCrossPlay, k_cross_play, ctx->lds_limit);
    hipLaunchKernelGGL(k_cross_play, dim3((unsigned)(n_pol * n_pol)), dim3(kXWidth), lds, ctx->stream, ctx->d_infoset, ctx->d_payoff, ctx->d_key,
                       ctx->d_states, d_policies, (int)n_pol, ctx->n_infosets, d_out);
    SC_HIP(ctx, hipGetLastError());
    return SCOPA_OK;
}

int32_t scopa_best_response(scopa_ctx *ctx, int32_t n_pol, const double *d_policies, double *d_br, double *d_out4) {
    if (!ctx || !d_policies || !d_out4 || n_pol < 1 || n_pol > 256) return SCOPA_EINVAL;
    SC_REQUIRE(ctx, ctx->has_deal, SCOPA_ESTATE, "scopa_best_response: no deal set");
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t lds = best_response_lds(ctx->n_infosets);
    SC_REQUIRE(ctx, lds <= (size_t)ctx->lds_limit, SCOPA_ELIMIT, "scopa_best_response: tables do not fit in LDS");
    SC_LDS_ATTR(ctx, scopa::kLdsBestResponse, k_best_response, ctx->lds_limit);
    hipLaunchKernelGGL(k_best_response, dim3((unsigned)(n_pol * 2)), dim3(1024), lds, ctx->stream, ctx->d_infoset, ctx->d_payoff, ctx->d_key,
                       d_policies, ctx->n_infosets, d_br, d_out4);
    SC_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_best_response_mean, dim3((unsigned)((n_pol + 255) / 256)), dim3(256), 0, ctx->stream, d_out4, (int)n_pol);
    SC_HIP(ctx, hipGetLastError());
    return SCOPA_OK;
}

int32_t scopa_eval_pair_match(scopa_ctx *ctx, const double *d_policy_a, const double *d_policy_b, int64_t n, int64_t n_seat0, uint32_t stream_id,
                              int32_t *d_node_idx_out, int64_t h_stats[10]) {
    if (!ctx || !d_policy_a || !d_policy_b || !h_stats || n < 0 || n_seat0 < 0 || n_seat0 > n) return SCOPA_EINVAL;
    SC_REQUIRE(ctx, ctx->has_deal, SCOPA_ESTATE, "scopa_eval_pair_match: no deal set");
    for (int j = 0; j < 10; j++) h_stats[j] = 0;
    if (!n) return SCOPA_OK;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    // thresholds [2][kDecision][3] and the ten sums: this entry point's own buffer (the prepared table of scopa_eval_tabular_prepare stays as it is)
    const size_t thr_bytes = sizeof(unsigned long long) * 2 * 3 * (size_t)kDecision;
    if (!ctx->d_pair_thr) SC_HIP(ctx, hipMalloc(&ctx->d_pair_thr, thr_bytes + sizeof(unsigned long long) * 16));
    unsigned long long *d_thr = reinterpret_cast<unsigned long long *>(ctx->d_pair_thr);
    unsigned long long *d_stats = d_thr + 2 * 3 * (size_t)kDecision;
    const int I = ctx->n_infosets;
    hipLaunchKernelGGL(k_pair_thresholds, dim3((unsigned)((2 * I + 255) / 256)), dim3(256), 0, ctx->stream, ctx->d_key, d_policy_a, d_policy_b, I, d_thr);
    SC_HIP(ctx, hipGetLastError());
    SC_HIP(ctx, hipMemsetAsync(d_stats, 0, sizeof(unsigned long long) * 10, ctx->stream));
    const long long n1 = n - n_seat0;
    const int blocks0 = (int)std::min<long long>((n_seat0 + 255) / 256, 2048), blocks1 = (int)std::min<long long>((n1 + 255) / 256, 2048);
    const size_t lds = (size_t)I * 24 + sizeof(uint16_t) * kDecision;
    hipLaunchKernelGGL(k_eval_pair_match, dim3((unsigned)(blocks0 + blocks1)), dim3(256), lds, ctx->stream, (long long)n, (long long)n_seat0, blocks0,
                       ctx->d_infoset, ctx->d_key, (const unsigned long long *)d_thr, I, ctx->d_states, (uint32_t)ctx->seed, (uint32_t)(ctx->seed >> 32),
                       stream_id, d_node_idx_out, d_stats);
    SC_HIP(ctx, hipGetLastError());
    SC_HIP(ctx, hipMemcpyAsync(h_stats, d_stats, sizeof(int64_t) * 10, hipMemcpyDeviceToHost, ctx->stream));
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SCOPA_OK;
}

}  // extern "C"
