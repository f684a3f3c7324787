// scopa_chance_xplay.hip -- what tabular policies do to each other on the chance game over a set of deals (scopa_chance.hip): the exact cross-play
// matrix of K policies averaged over the deals, the best responses across deals themselves (the choices scopa_chance_exploitability computes and
// discards), and the sampled seat-swapped match that draws the deal per episode.  The single-deal forms are in scopa_xplay.hip.
//
// Policies are [G][4] float64 tables over global ids in hand order, used as given (no normalisation; a non-finite entry propagates by IEEE rules).
// Every float64 sum runs in a fixed order and no float64 atomic is used, so results are bit-identical from run to run and to
// tests/chance_xplay_ref.py:
//   cross-play      per deal k_cross_play's order (children left to right from 0.0); across deals s = img[0]; s += img[1]; ... in deal order, s / n
//   best response   scopa_chance_exploitability's: q over a ply's nodes ascending from 0.0, then over the key's occurrences in ascending
//                   (deal, local id) order from the first; a strict `>` (ties to the lowest action); each figure summed in deal order, / n
//   match           integers only
#include <algorithm>

#include "scopa_chance.h"
#include "scopa_philox.h"
#include "scopa_tree_passes.h"

using namespace scopa;

namespace {
// best-response scratch of ONE policy: reach and values [n][2229], q rows [n][1653][8], choices [G] (rounded up to 8 bytes)
inline size_t xbr_policy_bytes(int n, long long G) {
    return (size_t)n * kNodes * 16 + (size_t)n * kDecision * 64 + (((size_t)G * 4 + 7) & ~(size_t)7);
}
}  // namespace

// =====================================================================================================================
// Cross-play, launch 1: workgroup (deal, a, b) = blockIdx.x / n_pol^2, (blockIdx.x / n_pol) % n_pol, blockIdx.x % n_pol runs k_cross_play's levels
// (cross_play_levels, scopa_tree_passes.h) on that deal's tree: the combined table -- a's rows at player-0 infosets, b's at player-1 infosets -- is gathered into LDS through
// the deal's map row from the two global tables, four quantities are set at the 576 terminals and carried up the eight plies,
// v = 0.0; v += row[c] * child[c], children left to right.  img[deal][a][b][4] receives the root's four.
__global__ void __launch_bounds__(kXWidth)
k_chance_cross_play(const uint16_t *__restrict__ g_infoset /*[n][1653]*/, const int8_t *__restrict__ g_payoff /*[n][576]*/,
                    const int32_t *__restrict__ g_map /*[n][1653]*/, const uint64_t *__restrict__ gkey /*[G]*/, const int32_t *__restrict__ g_meta /*[n][8]*/,
                    const scopa_state *__restrict__ g_states /*[n][2229]*/, const double *__restrict__ g_policies /*[n_pol][G][4]*/, int n_pol, long long G,
                    double *__restrict__ g_img /*[n][n_pol][n_pol][4]*/) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, nt = blockDim.x;
    const unsigned pairs = (unsigned)(n_pol * n_pol);
    const size_t deal = blockIdx.x / pairs;
    const int pair = (int)(blockIdx.x - (unsigned)deal * pairs), pa = pair / n_pol, pb = pair - pa * n_pol;
    g_infoset += deal * kDecision; g_payoff += deal * kTerminal; g_map += deal * kDecision; g_states += deal * kNodes;
    const int I = g_meta[deal * 8];
    double *s_pol = reinterpret_cast<double *>(smem);          // [I][4]
    double *s_lvl = s_pol + (size_t)I * 4;                     // [2][4][kXWidth]
    uint16_t *s_inf = reinterpret_cast<uint16_t *>(s_lvl + 2 * 4 * kXWidth);   // [kDecision]
    const double *pol_a = g_policies + (size_t)pa * (size_t)G * 4, *pol_b = g_policies + (size_t)pb * (size_t)G * 4;
    for (int cell = tid; cell < I * 4; cell += nt) {
        const size_t g = (size_t)g_map[cell >> 2];
        s_pol[cell] = ((gkey[g] & 1) ? pol_b : pol_a)[g * 4 + (cell & 3)];
    }
    for (int i = tid; i < kDecision; i += nt) s_inf[i] = g_infoset[i];
    const int cur = cross_play_levels(s_pol, s_lvl, s_inf, g_payoff, g_states, tid, nt);
    if (tid < 4) g_img[(size_t)blockIdx.x * 4 + tid] = s_lvl[cur * 4 * kXWidth + tid * kXWidth];
}

// launch 2: one lane per (a, b, quantity): the deals' values added in deal order from the first, then / n
__global__ void __launch_bounds__(256) k_chance_cross_mean(const double *__restrict__ g_img, int n, int cells /*n_pol * n_pol * 4*/, double *__restrict__ g_out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= cells) return;
    double s = g_img[t];
    for (int deal = 1; deal < n; deal++) s += g_img[(size_t)deal * cells + t];
    g_out[t] = s / (double)n;
}

// =====================================================================================================================
// Best responses across deals, for scopa_chance_best_response and (one policy, gridDim.y == 1) scopa_chance_exploitability: blockIdx.y = the
// policy's place in the chunk at hand, the policies read in place from the caller's tables.  Reach and node values per deal persist in HBM
// between launches.  Scratch per policy of the chunk: reach, val [n][2229]; q [n][1653][8]; choice [G].
// one workgroup per (deal, policy): reach of everyone but the responder `br` (2: nobody responds), top down, and the terminal values for `br`
__global__ void __launch_bounds__(256)
k_chance_xbr_reach(const uint16_t *__restrict__ g_infoset, const int8_t *__restrict__ g_payoff, const int32_t *__restrict__ g_map,
                   const double *__restrict__ policies /*[chunk][G][4]*/, long long G, int n_deals, double *__restrict__ g_reach, double *__restrict__ g_val, int br) {
    const size_t deal = blockIdx.x, slot = (size_t)blockIdx.y * n_deals + deal;
    const double *pol = policies + (size_t)blockIdx.y * (size_t)G * 4;
    g_infoset += deal * kDecision; g_payoff += deal * kTerminal; g_map += deal * kDecision; g_reach += slot * kNodes; g_val += slot * kNodes;
    const int tid = threadIdx.x, nt = blockDim.x;
    if (tid == 0) g_reach[0] = 1.0;
    __syncthreads();
    for (int d = 0; d < kPlies; d++) {
        const int n = nlegal_at(d), w1 = level_width(d + 1), p = d & 1;
        for (int j = tid; j < w1; j += nt) {
            const int par = j / n, a = j - par * n;
            const double r = g_reach[level_offset(d) + par];
            g_reach[level_offset(d + 1) + j] = p == br ? r : r * pol[(size_t)g_map[g_infoset[level_offset(d) + par]] * 4 + a];
        }
        __syncthreads();   // the workgroup's own global writes are visible to it after the barrier
    }
    for (int j = tid; j < kTerminal; j += nt) {
        const int p0 = g_payoff[j];
        g_val[level_offset(8) + j] = 0.5 * (double)(br == 1 ? -p0 : p0);
    }
}

// ply d of (deal, policy).  mode 0: policy-weighted values; 1: q of the deal's rows of this ply (nodes ascending from 0.0) into q rows [deal][local][8];
// 2: values selected by the responder's choice
__global__ void __launch_bounds__(256)
k_chance_xbr_ply(const uint16_t *__restrict__ g_infoset, const int32_t *__restrict__ g_map, const uint16_t *__restrict__ g_order, const int32_t *__restrict__ g_plyoff,
                 const double *__restrict__ policies, long long G, int n_deals, const int32_t *__restrict__ g_choice /*[chunk][G]*/, const double *__restrict__ g_reach,
                 double *__restrict__ g_val, double *__restrict__ g_q, int d, int mode) {
    __shared__ uint16_t s_inf[kTerminal];
    __shared__ double s_reach[kTerminal];
    const size_t deal = blockIdx.x, slot = (size_t)blockIdx.y * n_deals + deal;
    const double *pol = policies + (size_t)blockIdx.y * (size_t)G * 4;
    const int32_t *choice = g_choice + (size_t)blockIdx.y * (size_t)G;
    g_infoset += deal * kDecision; g_map += deal * kDecision; g_order += deal * 1656; g_plyoff += deal * 12; g_reach += slot * kNodes; g_val += slot * kNodes;
    g_q += slot * kDecision * 8;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int n = nlegal_at(d), w = level_width(d), off = level_offset(d), off1 = level_offset(d + 1);
    if (mode == 0) {
        for (int j = tid; j < w; j += nt) {
            const size_t g = (size_t)g_map[g_infoset[off + j]];
            double v = 0.0;
            for (int a = 0; a < n; a++) v += pol[g * 4 + a] * g_val[off1 + j * n + a];
            g_val[off + j] = v;
        }
    } else if (mode == 1) {
        for (int j = tid; j < w; j += nt) { s_inf[j] = g_infoset[off + j]; s_reach[j] = g_reach[off + j]; }
        __syncthreads();
        const int row0 = g_plyoff[d], cells = (g_plyoff[d + 1] - row0) * 4;
        for (int cell = tid; cell < cells; cell += nt) {
            const int r = g_order[row0 + (cell >> 2)], a = cell & 3;
            if (a >= n) continue;
            double q = 0.0;
            for (int j = 0; j < w; j++)
                if (s_inf[j] == r) q += s_reach[j] * g_val[off1 + j * n + a];
            g_q[(size_t)r * 8 + a] = q;
        }
    } else {
        for (int j = tid; j < w; j += nt) g_val[off + j] = g_val[off1 + j * n + choice[g_map[g_infoset[off + j]]]];
    }
}

// the responder's rows of ply d, per policy of the chunk: q summed over the occurrences in CSR order from the first, argmax with ties to the lowest action
__global__ void __launch_bounds__(256)
k_chance_xbr_choose(const uint64_t *__restrict__ gkey, const int32_t *__restrict__ occ_off, const int32_t *__restrict__ occ, const double *__restrict__ g_q,
                    int n_deals, int32_t *__restrict__ g_choice, long long G, int d) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    const int n = nlegal_at(d);
    if ((int)(gkey[g] & 1) != (d & 1) || (int)((gkey[g] >> 1) & 7) != n) return;
    const double *q = g_q + (size_t)blockIdx.y * n_deals * kDecision * 8;
    const int b = occ_off[g], e = occ_off[g + 1];
    double best_q = 0.0;
    int best = 0;
    for (int a = 0; a < n; a++) {
        double s = q[(size_t)occ[b] * 8 + a];
        for (int i = b + 1; i < e; i++) s += q[(size_t)occ[i] * 8 + a];
        if (a == 0) best_q = s;
        else if (s > best_q) { best_q = s; best = a; }
    }
    g_choice[(size_t)blockIdx.y * (size_t)G + g] = best;
}

// one lane per policy of the chunk: out4[k][1 + pass] = (v_deal0 + v_deal1 + ...) / n in deal order; after the last pass out4[k][0] = (BR0 + BR1) / 2
__global__ void __launch_bounds__(64) k_chance_xbr_sum(const double *__restrict__ g_val, int n, int pass, int chunk, double *__restrict__ out4 /*[chunk][4]*/) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= chunk) return;
    const double *val = g_val + (size_t)k * n * kNodes;
    double s = val[0];
    for (int deal = 1; deal < n; deal++) s += val[(size_t)deal * kNodes];
    out4[k * 4 + 1 + pass] = s / (double)n;
    if (pass == 2) out4[k * 4] = 0.5 * (out4[k * 4 + 1] + out4[k * 4 + 2]);
}

// after pass p < 2 every key of player p has its choice (a key belongs to exactly one ply): br[k][p] = policy k with player p's rows one-hot
__global__ void __launch_bounds__(256)
k_chance_xbr_table(const uint64_t *__restrict__ gkey, const double *__restrict__ policies, const int32_t *__restrict__ g_choice, long long G, int br,
                   double *__restrict__ g_br /*[chunk][2][G][4]*/) {
    const long long cell = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (cell >= G * 4) return;
    const long long r = cell >> 2;
    const size_t k = blockIdx.y;
    const double *pol = policies + k * (size_t)G * 4;
    double *tab = g_br + (k * 2 + (size_t)br) * (size_t)G * 4;
    tab[cell] = (int)(gkey[r] & 1) == br ? ((int)(cell & 3) == g_choice[k * (size_t)G + (size_t)r] ? 1.0 : 0.0) : pol[cell];
}

// =====================================================================================================================
// The match.  Thresholds of both tables per GLOBAL row, the legal count taken from the global key: policy_thresholds (scopa_tree_passes.h) per row, as
// in k_pair_thresholds (scopa_xplay.hip), so an episode that drew deal d ends where scopa_eval_pair_match ends it on a context holding d.
__global__ void __launch_bounds__(256)
k_chance_pair_thresholds(const uint64_t *__restrict__ gkey, const double *__restrict__ policy_a, const double *__restrict__ policy_b, long long G,
                         unsigned long long *__restrict__ thr /*[2][G][3]*/) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2 * G) return;
    const int which = t >= G;
    const long long r = t - which * G;
    policy_thresholds((int)((gkey[r] >> 1) & 7), (which ? policy_b : policy_a) + (size_t)r * 4, thr + (size_t)t * 3);
}

// k_eval_pair_match (scopa_xplay.hip) with the deal drawn per episode: one lane per episode, deal = umulhi(x0, n) of the Philox word of counter
// (episode, episode >> 32, 8, stream_id) -- the plies use tags 0..5 -- then the same walk over node indices of that deal's tree with the same counters
// (episode, ply, stream_id; seed), the same 53-bit N and the same three compares.  The tables of a set do not fit in LDS (3.8 MB of thresholds per policy
// at 495 deals), so a ply gathers three things from global memory: the node's infoset, its global id, the threshold row.  A workgroup serves ONE
// seat half, as there; stats[half][0..4] from a's point of view.
__global__ void __launch_bounds__(256)
k_chance_match(long long n, long long n_seat0, int blocks0, int n_deals, const uint16_t *__restrict__ g_infoset /*[n_deals][1653]*/,
               const int32_t *__restrict__ g_map /*[n_deals][1653]*/, const unsigned long long *__restrict__ g_thr /*[2][G][3]*/, long long G,
               const scopa_state *__restrict__ g_states /*[n_deals][2229]*/, uint32_t seed_lo, uint32_t seed_hi, uint32_t stream,
               int32_t *__restrict__ out_deal, int32_t *__restrict__ out_idx, unsigned long long *__restrict__ stats /*[2][5]*/) {
    __shared__ unsigned long long s_stats[5];
    const int seat = (int)blockIdx.x >= blocks0;    // a's seat in this workgroup's half
    if (threadIdx.x < 5) s_stats[threadIdx.x] = 0ull;
    __syncthreads();
    const long long first = seat ? n_seat0 : 0, end = seat ? n : n_seat0;
    const long long block = seat ? (long long)blockIdx.x - blocks0 : (long long)blockIdx.x;
    const long long stride = (long long)(seat ? (int)gridDim.x - blocks0 : blocks0) * blockDim.x;
    long long acc[5] = {0, 0, 0, 0, 0};
    for (long long i = first + block * blockDim.x + threadIdx.x; i < end; i += stride) {
        const philox_out xd = philox4x32_10((uint32_t)i, (uint32_t)(i >> 32), 8u, stream, seed_lo, seed_hi);
        const size_t deal = (size_t)__umulhi(xd.x0, (uint32_t)n_deals);   // < n_deals
        const uint16_t *inf = g_infoset + deal * kDecision;
        const int32_t *map = g_map + deal * kDecision;
        int idx = 0;
#pragma unroll
        for (int ply = 0; ply < 6; ply++) {   // plies 6 and 7 have one legal card and draw nothing
            const int nl = nlegal_at(ply);
            const philox_out x = philox4x32_10((uint32_t)i, (uint32_t)(i >> 32), (uint32_t)ply, stream, seed_lo, seed_hi);
            const size_t g = (size_t)map[inf[level_offset(ply) + idx]];
            const unsigned long long *t = g_thr + (((ply & 1) == seat ? (size_t)0 : (size_t)G) + g) * 3;   // the mover's table: a's where a sits
            const unsigned long long N = ((unsigned long long)(x.x0 >> 5) << 26) | (unsigned long long)(x.x1 >> 6);   // u = N * 2^-53
            const int a = (int)(t[0] <= N) + (int)(t[1] <= N) + (int)(t[2] <= N);
            idx = idx * nl + (a < nl - 1 ? a : nl - 1);
        }
        const uint32_t tw = reinterpret_cast<const uint4 *>(g_states)[deal * kNodes + kDecision + idx].w;
        const int r0 = (int)(tw & 255u) + 2 * (int)((tw >> 16) & 255u), r1 = (int)((tw >> 8) & 255u) + 2 * (int)(tw >> 24);
        const int mine = seat ? r1 - r0 : r0 - r1;
        acc[0] += 1; acc[1] += mine; acc[2] += mine * mine;
        acc[3] += (int)((tw >> (16 + 8 * seat)) & 255u); acc[4] += (int)((tw >> (24 - 8 * seat)) & 255u);
        if (out_deal) out_deal[i] = (int32_t)deal;
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

// The three passes of `chunk` policies (0: best response of player 0, 1: of player 1, 2: the plain value for player 0) on the caller's buffers --
// reach, val [chunk][n][2229]; q [chunk][n][1653][8]; choice [chunk][G] -- into out4[chunk][4] and, where d_br is given, the tables
// d_br[chunk][2][G][4].  Launches only, on the context's stream.
void scopa::chance_br_passes(scopa_chance *g, int chunk, const double *policies, double *reach, double *val, double *q, int32_t *choice, double *out4, double *d_br) {
    scopa_ctx *ctx = g->ctx;
    scopa_multi *m = g->m;
    const unsigned row_blocks = (unsigned)((g->G + 255) / 256), cell_blocks = (unsigned)((g->G * 4 + 255) / 256);
    for (int pass = 0; pass < 3; pass++) {
        hipLaunchKernelGGL(k_chance_xbr_reach, dim3(g->n, chunk), dim3(256), 0, ctx->stream, m->d_infoset, m->d_payoff, g->d_map, policies, g->G, g->n, reach, val, pass);
        for (int d = kPlies - 1; d >= 0; d--) {
            auto ply = [&](int mode) {
                hipLaunchKernelGGL(k_chance_xbr_ply, dim3(g->n, chunk), dim3(256), 0, ctx->stream, m->d_infoset, g->d_map, g->d_order, g->d_plyoff, policies, g->G, g->n,
                                   (const int32_t *)choice, (const double *)reach, val, q, d, mode);
            };
            if ((d & 1) == pass) {
                ply(1);
                hipLaunchKernelGGL(k_chance_xbr_choose, dim3(row_blocks, chunk), dim3(256), 0, ctx->stream, g->d_gkey, g->d_occ_off, g->d_occ, (const double *)q, g->n,
                                   choice, g->G, d);
                ply(2);
            } else {
                ply(0);
            }
        }
        hipLaunchKernelGGL(k_chance_xbr_sum, dim3((unsigned)((chunk + 63) / 64)), dim3(64), 0, ctx->stream, (const double *)val, g->n, pass, chunk, out4);
        if (pass < 2 && d_br)
            hipLaunchKernelGGL(k_chance_xbr_table, dim3(cell_blocks, chunk), dim3(256), 0, ctx->stream, g->d_gkey, policies, (const int32_t *)choice, g->G, pass, d_br);
    }
}

extern "C" {

int32_t scopa_chance_cross_play(scopa_chance *g, int32_t n_pol, const double *d_policies, double *d_per_deal, double *d_out) {
    if (!g || !d_policies || !d_out || n_pol < 1 || n_pol > 256) return SCOPA_EINVAL;
    scopa_ctx *ctx = g->ctx;
    scopa_multi *m = g->m;
    const unsigned long long groups = (unsigned long long)g->n * (unsigned long long)n_pol * (unsigned long long)n_pol;
    SC_REQUIRE(ctx, groups < (1ull << 31), SCOPA_ELIMIT, "scopa_chance_cross_play: n * n_pol * n_pol must stay below 2^31 workgroups");
    const size_t lds = cross_play_lds(m->max_infosets);   // k_cross_play's carving at the largest deal of the set
    SC_REQUIRE(ctx, lds <= (size_t)ctx->lds_limit, SCOPA_ELIMIT, "scopa_chance_cross_play: the largest deal's tables do not fit in LDS");
    SC_HIP(ctx, hipSetDevice(ctx->device));
    double *img = d_per_deal;
    if (!img) {
        const size_t bytes = (size_t)groups * 32;
        if (bytes > g->xp_img_bytes) {
            SC_HIP(ctx, hipStreamSynchronize(ctx->stream));   // an earlier call's launches may still use the old image
            if (g->d_xp_img) { (void)hipFree(g->d_xp_img); g->d_xp_img = nullptr; g->xp_img_bytes = 0; }
            if (hipMalloc(&g->d_xp_img, bytes) != hipSuccess) { g->d_xp_img = nullptr; return fail(ctx, SCOPA_ENOMEM, "scopa_chance_cross_play: no device memory for the per-deal image"); }
            g->xp_img_bytes = bytes;
        }
        img = g->d_xp_img;
    }
    SC_LDS_ATTR(ctx, scopa::kLdsChanceCrossPlay, k_chance_cross_play, ctx->lds_limit);
    hipLaunchKernelGGL(k_chance_cross_play, dim3((unsigned)groups), dim3(kXWidth), lds, ctx->stream, m->d_infoset, m->d_payoff, g->d_map, g->d_gkey, m->d_meta,
                       m->d_states, d_policies, (int)n_pol, g->G, img);
    SC_HIP(ctx, hipGetLastError());
    const int cells = n_pol * n_pol * 4;
    hipLaunchKernelGGL(k_chance_cross_mean, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, ctx->stream, (const double *)img, g->n, cells, d_out);
    SC_HIP(ctx, hipGetLastError());
    return SCOPA_OK;
}

int32_t scopa_chance_debug_scratch_budget(scopa_chance *g, int64_t bytes) {
    // test hook: the best-response scratch budget, so that the chunked route can be exercised with a handful of policies; 0 restores 1 GiB
    if (!g || bytes < 0) return SCOPA_EINVAL;
    g->xbr_budget = bytes ? (size_t)bytes : (size_t)1 << 30;
    return SCOPA_OK;
}

int32_t scopa_chance_best_response(scopa_chance *g, int32_t n_pol, const double *d_policies, double *d_br, double *d_out4) {
    if (!g || !d_policies || !d_out4 || n_pol < 1 || n_pol > 256) return SCOPA_EINVAL;
    scopa_ctx *ctx = g->ctx;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    // policies go through in chunks whose scratch stays below the budget (a single policy is always taken): chunks share nothing but the
    // scratch, so chunking changes no bit
    const size_t per = xbr_policy_bytes(g->n, g->G);
    const int chunk = (int)std::min<size_t>((size_t)n_pol, std::max<size_t>((size_t)1, g->xbr_budget / per));
    if ((size_t)chunk * per > g->xbr_bytes) {
        SC_HIP(ctx, hipStreamSynchronize(ctx->stream));   // an earlier call's launches may still use the old scratch
        if (g->d_xbr) { (void)hipFree(g->d_xbr); g->d_xbr = nullptr; g->xbr_bytes = 0; }
        if (hipMalloc(&g->d_xbr, (size_t)chunk * per) != hipSuccess) { g->d_xbr = nullptr; return fail(ctx, SCOPA_ENOMEM, "scopa_chance_best_response: no device memory for the scratch"); }
        g->xbr_bytes = (size_t)chunk * per;
    }
    const size_t Gs = (size_t)g->G;
    double *d_reach = reinterpret_cast<double *>(g->d_xbr);                      // [chunk][n][2229]
    double *d_val = d_reach + (size_t)chunk * g->n * kNodes;                     // [chunk][n][2229]
    double *d_q = d_val + (size_t)chunk * g->n * kNodes;                         // [chunk][n][1653][8]
    int32_t *d_choice = reinterpret_cast<int32_t *>(d_q + (size_t)chunk * g->n * kDecision * 8);   // [chunk][G]
    for (int k0 = 0; k0 < n_pol; k0 += chunk) {
        chance_br_passes(g, std::min(chunk, n_pol - k0), d_policies + (size_t)k0 * Gs * 4, d_reach, d_val, d_q, d_choice, d_out4 + (size_t)k0 * 4,
                         d_br ? d_br + (size_t)k0 * 2 * Gs * 4 : nullptr);
        SC_HIP(ctx, hipGetLastError());
    }
    return SCOPA_OK;
}

int32_t scopa_chance_match(scopa_chance *g, const double *d_policy_a, const double *d_policy_b, int64_t n, int64_t n_seat0, uint32_t stream_id,
                           int32_t *d_deal_out, int32_t *d_node_idx_out, int64_t h_stats[10]) {
    if (!g || !d_policy_a || !d_policy_b || !h_stats || n < 0 || n_seat0 < 0 || n_seat0 > n) return SCOPA_EINVAL;
    scopa_ctx *ctx = g->ctx;
    scopa_multi *m = g->m;
    for (int j = 0; j < 10; j++) h_stats[j] = 0;
    if (!n) return SCOPA_OK;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t Gs = (size_t)g->G;
    if (!g->d_xmatch && hipMalloc(&g->d_xmatch, sizeof(unsigned long long) * (2 * 3 * Gs + 16)) != hipSuccess) {
        g->d_xmatch = nullptr;
        return fail(ctx, SCOPA_ENOMEM, "scopa_chance_match: no device memory for the thresholds");
    }
    unsigned long long *d_thr = reinterpret_cast<unsigned long long *>(g->d_xmatch);
    unsigned long long *d_stats = d_thr + 2 * 3 * Gs;
    hipLaunchKernelGGL(k_chance_pair_thresholds, dim3((unsigned)((2 * g->G + 255) / 256)), dim3(256), 0, ctx->stream, g->d_gkey, d_policy_a, d_policy_b, g->G, d_thr);
    SC_HIP(ctx, hipGetLastError());
    SC_HIP(ctx, hipMemsetAsync(d_stats, 0, sizeof(unsigned long long) * 10, ctx->stream));
    const long long n1 = n - n_seat0;
    const int blocks0 = (int)std::min<long long>((n_seat0 + 255) / 256, 2048), blocks1 = (int)std::min<long long>((n1 + 255) / 256, 2048);
    hipLaunchKernelGGL(k_chance_match, dim3((unsigned)(blocks0 + blocks1)), dim3(256), 0, ctx->stream, (long long)n, (long long)n_seat0, blocks0, g->n, m->d_infoset,
                       g->d_map, (const unsigned long long *)d_thr, g->G, m->d_states, (uint32_t)ctx->seed, (uint32_t)(ctx->seed >> 32), stream_id, d_deal_out,
                       d_node_idx_out, d_stats);
    SC_HIP(ctx, hipGetLastError());
    SC_HIP(ctx, hipMemcpyAsync(h_stats, d_stats, sizeof(int64_t) * 10, hipMemcpyDeviceToHost, ctx->stream));
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SCOPA_OK;
}

}  // extern "C"
