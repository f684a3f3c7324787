// scopa_xplay.hip -- what two tabular policies do to each other on the deal's tree: the exact cross-play matrix of K policies, the best
// responses themselves (the table k_exploitability computes and discards), and the sampled seat-swapped match with a policy in both seats.
//
// Policies are [n_infosets][4] float64 tables in hand order, used as given (no normalisation; a non-finite entry propagates by IEEE rules).
// Every float64 sum runs in a fixed order -- children left to right from 0.0; an infoset's nodes in ply order from 0.0 -- the orders of
// k_exploitability (scopa_eval.hip) and of the oracle, so results are bit-identical from run to run and to tests/xplay_ref.py.
#include <algorithm>

#include "scopa_ctx.h"
#include "scopa_philox.h"

using namespace scopa;

namespace {
constexpr int kXWidth = 576;   // the widest ply (level_width(6..8)): one lane per node of a level
constexpr size_t kInfBytes = 1656 * 2;   // d_infoset staged in LDS, rounded up to 8 bytes
// dynamic LDS of k_cross_play: the combined table, two adjacent levels of four quantities, the infoset map (include/scopa.h quotes this)
inline size_t cross_play_lds(int n_infosets) { return (size_t)n_infosets * 32 + sizeof(double) * 2 * 4 * kXWidth + kInfBytes; }
// ... and of k_best_response: k_exploitability's carving
inline size_t best_response_lds(int n_infosets) {
    return (size_t)n_infosets * 32 * 2 + sizeof(double) * kNodes * 2 + sizeof(int) * (size_t)n_infosets + kInfBytes;
}
}  // namespace

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
    for (int j = tid; j < kTerminal; j += nt) {
        const int p0 = g_payoff[j];
        const uint32_t w = reinterpret_cast<const uint4 *>(tree_states)[kDecision + j].w;   // ncap[2] | scopas[2]
        s_lvl[0 * kXWidth + j] = 0.5 * (double)p0;
        s_lvl[1 * kXWidth + j] = 0.25 * (double)p0 * (double)p0;
        s_lvl[2 * kXWidth + j] = (double)((w >> 16) & 255u);
        s_lvl[3 * kXWidth + j] = (double)(w >> 24);
    }
    __syncthreads();
    int cur = 0;   // the buffer that holds ply d + 1
    for (int d = kPlies - 1; d >= 0; d--) {
        const int n = nlegal_at(d), w = level_width(d), off = level_offset(d);
        const double *child = s_lvl + cur * 4 * kXWidth;
        double *mine = s_lvl + (cur ^ 1) * 4 * kXWidth;
        for (int j = tid; j < w; j += nt) {
            const double *row = s_pol + (size_t)s_inf[off + j] * 4;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                double v = 0.0;
                for (int c = 0; c < n; c++) v += row[c] * child[q * kXWidth + j * n + c];
                mine[q * kXWidth + j] = v;
            }
        }
        cur ^= 1;
        __syncthreads();
    }
    if (tid < 4) g_out[(size_t)blockIdx.x * 4 + tid] = s_lvl[cur * 4 * kXWidth + tid * kXWidth];
}

// =====================================================================================================================
// Best responses: workgroup (k, p) = blockIdx.x / 2, blockIdx.x % 2 runs pass p of k_exploitability on policy k -- the same reach, the same
// per-(infoset, action) sums over the ply's nodes in ascending order from 0.0, the same strict `>` (ties to the lowest action) -- and keeps the
// choices: g_br[k][p] is policy k with player p's rows replaced by the one-hot rows of the choices.  Workgroup (k, 0) also runs the plain
// value pass.  out4[k][1 + p] = BR_p, out4[k][3] = value; k_best_response_mean then fills out4[k][0].
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
        if (tid == 0) s_reach[0] = 1.0;
        __syncthreads();
        for (int d = 0; d < kPlies; d++) {  // top-down: reach of everyone but the best responder
            const int n = nlegal_at(d), w1 = level_width(d + 1), p = d & 1;
            for (int j = tid; j < w1; j += nt) {
                const int par = j / n, a = j - par * n;
                const double r = s_reach[level_offset(d) + par];
                s_reach[level_offset(d + 1) + j] = p == br ? r : r * s_pol[s_inf[level_offset(d) + par] * 4 + a];
            }
            __syncthreads();
        }
        for (int j = tid; j < kTerminal; j += nt) {
            const int p0 = g_payoff[j];
            s_val[level_offset(8) + j] = 0.5 * (double)(br == 1 ? -p0 : p0);
        }
        __syncthreads();
        for (int d = kPlies - 1; d >= 0; d--) {  // bottom-up
            const int n = nlegal_at(d), w = level_width(d), off = level_offset(d), p = d & 1;
            if (p == br) {
                for (int cell = tid; cell < I * 4; cell += nt) {
                    const int r = cell >> 2, a = cell & 3;
                    if ((int)(g_key[r] & 1) != p || (int)((g_key[r] >> 1) & 7) != n || a >= n) continue;
                    double q = 0.0;
                    for (int j = 0; j < w; j++)
                        if (s_inf[off + j] == r) q += s_reach[off + j] * s_val[level_offset(d + 1) + j * n + a];
                    s_q[cell] = q;
                }
                __syncthreads();
                for (int r = tid; r < I; r += nt) {
                    if ((int)(g_key[r] & 1) != p || (int)((g_key[r] >> 1) & 7) != n) continue;
                    int best = 0;
                    for (int a = 1; a < n; a++) if (s_q[r * 4 + a] > s_q[r * 4 + best]) best = a;
                    s_choice[r] = best;
                }
                __syncthreads();
                for (int j = tid; j < w; j += nt) s_val[off + j] = s_val[level_offset(d + 1) + j * n + s_choice[s_inf[off + j]]];
            } else {
                for (int j = tid; j < w; j += nt) {
                    const int r = s_inf[off + j];
                    double v = 0.0;
                    for (int a = 0; a < n; a++) v += s_pol[r * 4 + a] * s_val[level_offset(d + 1) + j * n + a];
                    s_val[off + j] = v;
                }
            }
            __syncthreads();
        }
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
// Pair match.  Thresholds of both tables, k_eval_thresholds' formula (scopa_eval.hip): thr[t][r][k] = ceil(cdf_k / cdf_last * 2^53) for
// k < n - 1, 0 where the quotient is <= 0, 2^53 (never counted) beyond and where it is >= 1 or NaN.
// A COPY of that kernel's arithmetic for two tables in one launch (scopa_eval.hip keeps its kernel to itself): whoever changes one changes the
// other.  tests/test_gpu_xplay.py pins them to each other: a pair match against the uniform table walks the episodes of scopa_eval_tabular_match.
__global__ void __launch_bounds__(256)
k_pair_thresholds(const uint64_t *__restrict__ g_key, const double *__restrict__ policy_a, const double *__restrict__ policy_b, int n_infosets,
                  unsigned long long *__restrict__ thr /*[2][I][3]*/) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2 * n_infosets) return;
    const int which = t >= n_infosets, r = t - which * n_infosets;
    const int n = (int)((g_key[r] >> 1) & 7);
    const double *row = (which ? policy_b : policy_a) + (size_t)r * 4;
    double c = 0.0, cdf[4] = {0.0, 0.0, 0.0, 0.0};
    for (int q = 0; q < n; q++) { c = q ? c + row[q] : row[0]; cdf[q] = c; }
    const double last = n > 0 ? cdf[n - 1] : 0.0;
    for (int k = 0; k < 3; k++) {
        unsigned long long v = 1ull << 53;
        if (k < n - 1) {
            const double x = cdf[k] / last;
            if (x <= 0.0) v = 0ull;
            else if (x < 1.0) v = (unsigned long long)ceil(x * 9007199254740992.0);
        }
        thr[(size_t)t * 3 + k] = v;
    }
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
