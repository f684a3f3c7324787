// scopa_team_xplay.hip -- what tabular policies do to each other on Team MiniScopa: the exact cross-play matrix of K policies and the sampled
// seat-swapped match, on a context's deal (scopa_team_cross_play, scopa_team_match) and on a set of deals with the deal as a chance move
// (scopa_team_chance_cross_play, scopa_team_chance_match).  The sweep and the episode walk are defined once in scopa_team_xplay.h and instantiated
// here with the two addressing policies.
//
// Policies are [rows][4] float64 DEVICE tables, used as given (no normalisation; a non-finite entry propagates by IEEE rules; the padding slots are
// never read into a sum).  Policy a plays team 0's depths and policy b team 1's.
//   k_team_cross_play      grid (K^2, 256, n) = (a * K + b, subtree, deal), the pair index fastest: the workgroups that share a deal's map row,
//                          its leaves and a subtree's rows are neighbours, and no grid dimension times 256 lanes comes near 2^32.  One upward pass over the subtree's 1 255 rows: every row is loaded once,
//                          a 32-byte vector straight from the mover's team's table through the addressing policy -- a lane asks for its at most
//                          11 rows before the first level -- and only the VALUES live in LDS: 1 255 x 4 float64 = 40 160 bytes (static), four
//                          workgroups of 256 lanes per compute unit by LDS (72 VGPRs).  The depth-12 quantities are made where depth 11 reads
//                          them, from the int8 payoff and the leaf scopa byte.  The four root values go to sub[deal][a * K + b][subtree][4]
//   k_team_cross_top       grid (K^2, n): depths 3..0 from the 256 x 4 subtree values -> img[deal][a][b][4]
//   k_team_cross_mean      chance form: one lane per (a, b, quantity), s = img[0]; s += img[1]; ... in deal order, s / (double)n
//   k_team_match           one lane per episode, a workgroup serves one seat half; the ten sums are integers
// No float64 atomics, every sum in a fixed order: cross-play is bit-identical from run to run and to tests/team_xplay_ref.py.  The cross-play calls
// launch on the context's stream and do not synchronise it; the match calls return host sums and do.
//
// The leaf scopas (uint8 per depth-12 node, team 0 in the low nibble) are built at the first call that needs them -- set_deal and create do not pay
// for them -- and scopa_team_set_deal invalidates the context's copy.
#include <algorithm>

#include "scopa_team_chance.h"
#include "scopa_team_xplay.h"

using scopa::fail;

namespace {

__global__ void __launch_bounds__(256)
k_team_leaf_scopas(scopa_team_state root, uint8_t *__restrict__ g_sc) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < kTLeaves) g_sc[i] = team_leaf_scopas(root, i);
}

__global__ void __launch_bounds__(256)
k_team_chance_leaf_scopas(const scopa_team_state *__restrict__ g_roots, uint8_t *__restrict__ g_sc, long long total) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int deal = (int)(i / kTLeaves);
    g_sc[i] = team_leaf_scopas(g_roots[deal], (int)(i - (long long)deal * kTLeaves));
}

template <class Addr>
__global__ void __launch_bounds__(kSubThreads)
k_team_cross_play(const double *__restrict__ g_policies, size_t table /* doubles per policy */, int n_pol, const int32_t *__restrict__ g_map,
                  const int8_t *__restrict__ g_r2, const uint8_t *__restrict__ g_sc, double *__restrict__ g_sub /*[n][K^2][256][4]*/) {
    __shared__ __align__(32) double s_val[kXQ * kSubRows];
    const unsigned pairs = gridDim.x, pair = blockIdx.x;
    const size_t deal = blockIdx.z;
    const int g = (int)blockIdx.y, pa = (int)(pair / (unsigned)n_pol), pb = (int)(pair - (unsigned)pa * (unsigned)n_pol), tid = threadIdx.x;
    const Addr addr = xaddr<Addr>(g_map, deal);
    xsub_sweep(g, addr, g_policies + (size_t)pa * table, g_policies + (size_t)pb * table, g_r2 + deal * kTLeaves, g_sc + deal * kTLeaves, s_val, tid);
    if (tid < kXQ) g_sub[((deal * pairs + pair) * kSubtrees + g) * kXQ + tid] = s_val[tid];
}

template <class Addr>
__global__ void __launch_bounds__(kSubThreads)
k_team_cross_top(const double *__restrict__ g_policies, size_t table, int n_pol, const int32_t *__restrict__ g_map, const double *__restrict__ g_sub,
                 double *__restrict__ g_img /*[n][K][K][4]*/) {
    __shared__ __align__(32) double s_val[kXQ * (kTopRows + kSubtrees)];
    const unsigned pairs = gridDim.x, pair = blockIdx.x;
    const size_t deal = blockIdx.y, slot = deal * pairs + pair;
    const int pa = (int)(pair / (unsigned)n_pol), pb = (int)(pair - (unsigned)pa * (unsigned)n_pol), tid = threadIdx.x;
    for (int k = tid; k < kSubtrees * kXQ; k += kSubThreads) s_val[kTopRows * kXQ + k] = g_sub[slot * kSubtrees * kXQ + k];
    __syncthreads();
    xtop_sweep(xaddr<Addr>(g_map, deal), g_policies + (size_t)pa * table, g_policies + (size_t)pb * table, s_val, tid);
    if (tid < kXQ) g_img[slot * kXQ + tid] = s_val[tid];
}

__global__ void __launch_bounds__(256) k_team_cross_mean(const double *__restrict__ g_img, int n, int cells /* K * K * 4 */, double *__restrict__ g_out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= cells) return;
    double s = g_img[t];
    for (int deal = 1; deal < n; deal++) s += g_img[(size_t)deal * cells + t];
    g_out[t] = s / (double)n;
}

// Workgroups [0, blocks0) serve the episodes [0, n_team0) with policy a as team 0, the others the rest with a as team 1.  kDraw: the deal is drawn per
// episode, (x0 * n_deals) >> 32 of the first Philox word of counter (i, i >> 32, 44, stream).  stats[half][0..4] from a's side.
template <class Addr, bool kDraw>
__global__ void __launch_bounds__(256)
k_team_match(long long n, long long n_team0, int blocks0, int n_deals, const int32_t *__restrict__ g_map, const double *__restrict__ pol_a,
             const double *__restrict__ pol_b, const int8_t *__restrict__ g_r2, const uint8_t *__restrict__ g_sc, uint32_t seed_lo, uint32_t seed_hi, uint32_t stream,
             int32_t *__restrict__ out_deal, int32_t *__restrict__ out_leaf, unsigned long long *__restrict__ stats /*[2][5]*/) {
    __shared__ unsigned long long s_stats[5];
    const int half = (int)blockIdx.x >= blocks0;    // a's team in this workgroup's half
    if (threadIdx.x < 5) s_stats[threadIdx.x] = 0ull;
    __syncthreads();
    const long long first = half ? n_team0 : 0, end = half ? n : n_team0;
    const long long block = half ? (long long)blockIdx.x - blocks0 : (long long)blockIdx.x;
    const long long stride = (long long)(half ? (int)gridDim.x - blocks0 : blocks0) * blockDim.x;
    long long acc[5] = {0, 0, 0, 0, 0};
    for (long long i = first + block * blockDim.x + threadIdx.x; i < end; i += stride) {
        size_t deal = 0;
        if constexpr (kDraw) {
            const scopa::philox_out xd = scopa::philox4x32_10((uint32_t)i, (uint32_t)((unsigned long long)i >> 32), kXDealTag, stream, seed_lo, seed_hi);
            deal = (size_t)__umulhi(xd.x0, (uint32_t)n_deals);   // < n_deals
        }
        const int leaf = xmatch_walk(xaddr<Addr>(g_map, deal), pol_a, pol_b, half, i, stream, seed_lo, seed_hi);
        const int r2 = g_r2[deal * kTLeaves + leaf];
        const uint32_t sc = g_sc[deal * kTLeaves + leaf];
        const int mine = half ? -r2 : r2;
        acc[0] += 1; acc[1] += mine; acc[2] += mine * mine;
        acc[3] += (int)(half ? sc >> 4 : sc & 15u); acc[4] += (int)(half ? sc & 15u : sc >> 4);
        if (kDraw && out_deal) out_deal[i] = (int32_t)deal;
        if (out_leaf) out_leaf[i] = leaf;
    }
#pragma unroll
    for (int j = 0; j < 5; j++) {
        long long v = acc[j];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if ((threadIdx.x & 63) == 0 && v != 0) atomicAdd(&s_stats[j], (unsigned long long)v);
    }
    __syncthreads();
    if (threadIdx.x < 5 && s_stats[threadIdx.x] != 0ull) atomicAdd(&stats[half * 5 + threadIdx.x], s_stats[threadIdx.x]);
}

// a scratch buffer that grows on demand; an earlier call's launches may still use the old one
int32_t xp_grow(scopa_ctx *ctx, double *&buf, size_t &have, size_t bytes, const char *what) {
    if (bytes <= have) return SCOPA_OK;
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (buf) { (void)hipFree(buf); buf = nullptr; have = 0; }
    if (hipMalloc(&buf, bytes) != hipSuccess) { buf = nullptr; (void)hipGetLastError(); return fail(ctx, SCOPA_ENOMEM, what); }
    have = bytes;
    return SCOPA_OK;
}

// both scratch images of a cross-play call, or neither
int32_t xp_images(scopa_ctx *ctx, scopa_team_xplay_scratch *xp, size_t sub_bytes, size_t img_bytes, const char *what) {
    int32_t rc = xp_grow(ctx, xp->d_sub, xp->sub_bytes, sub_bytes, what);
    if (rc == SCOPA_OK) rc = xp_grow(ctx, xp->d_img, xp->img_bytes, img_bytes, what);
    if (rc == SCOPA_ENOMEM) {
        if (xp->d_sub) (void)hipFree(xp->d_sub);
        if (xp->d_img) (void)hipFree(xp->d_img);
        xp->d_sub = xp->d_img = nullptr; xp->sub_bytes = xp->img_bytes = 0;
    }
    return rc;
}

int32_t xp_leaf_buffer(scopa_ctx *ctx, scopa_team_xplay_scratch *xp, size_t bytes, const char *what) {
    if (xp->d_leaf_sc) return SCOPA_OK;
    if (hipMalloc(&xp->d_leaf_sc, bytes) != hipSuccess) { xp->d_leaf_sc = nullptr; (void)hipGetLastError(); return fail(ctx, SCOPA_ENOMEM, what); }
    xp->leaf_sc_valid = false;
    return SCOPA_OK;
}

int32_t xp_leaves(scopa_ctx *ctx, scopa_team_solver *t) {
    scopa_team_xplay_scratch *xp = &t->xp;
    if (int32_t rc = xp_leaf_buffer(ctx, xp, kTLeaves, "scopa_team cross-play / match: no device memory for the leaf scopas")) return rc;
    if (xp->leaf_sc_valid) return SCOPA_OK;
    hipLaunchKernelGGL(k_team_leaf_scopas, dim3((kTLeaves + 255) / 256), dim3(256), 0, ctx->stream, t->root, xp->d_leaf_sc);
    SC_HIP(ctx, hipGetLastError());
    xp->leaf_sc_valid = true;
    return SCOPA_OK;
}

int32_t xp_leaves(scopa_team_chance *g) {
    scopa_ctx *ctx = g->ctx;
    scopa_team_xplay_scratch *xp = &g->xp;
    const size_t leaves = (size_t)g->n * kTLeaves;
    if (int32_t rc = xp_leaf_buffer(ctx, xp, leaves, "scopa_team_chance cross-play / match: no device memory for the leaf scopas")) return rc;
    if (xp->leaf_sc_valid) return SCOPA_OK;
    scopa_team_state *d_roots = nullptr;
    if (hipMalloc(&d_roots, (size_t)g->n * sizeof(scopa_team_state)) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(xp->d_leaf_sc); xp->d_leaf_sc = nullptr;
        return fail(ctx, SCOPA_ENOMEM, "scopa_team_chance cross-play / match: no device memory for the leaf scopas");
    }
    bool ok = hipMemcpyAsync(d_roots, g->h_roots.data(), (size_t)g->n * sizeof(scopa_team_state), hipMemcpyHostToDevice, ctx->stream) == hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(k_team_chance_leaf_scopas, dim3((unsigned)((leaves + 255) / 256)), dim3(256), 0, ctx->stream, (const scopa_team_state *)d_roots, xp->d_leaf_sc,
                           (long long)leaves);
        ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(ctx->stream) == hipSuccess;   // the roots are freed below: once per handle
    }
    (void)hipFree(d_roots);
    if (!ok) return fail(ctx, SCOPA_EHIP, "scopa_team_chance cross-play / match: building the leaf scopas failed");
    xp->leaf_sc_valid = true;
    return SCOPA_OK;
}

bool xp_aligned(const void *p) { return ((uintptr_t)p & 31) == 0; }

unsigned long long xp_group_limit(const scopa_ctx *ctx) { return ctx->team_xplay_group_limit > 0 ? (unsigned long long)ctx->team_xplay_group_limit : 1ull << 31; }

// the launches of a cross-play over n deals: the subtrees, the tops, and (mean) the deal-order mean of img into d_out; without it the tops write d_out
template <class Addr>
int32_t xp_cross_launch(scopa_ctx *ctx, int n, int n_pol, const double *d_policies, size_t table, const int32_t *d_map, const int8_t *d_r2, const uint8_t *d_sc,
                        double *d_sub, double *d_img, double *d_out, bool mean) {
    const unsigned pairs = (unsigned)(n_pol * n_pol);
    // a 3-D grid: HIP launches no dimension whose workgroups x 256 lanes reach 2^32, which a flat index would at 2^24 workgroups (n_pol = 256 on one deal);
    // here x <= 65 536 pairs, y = 256 subtrees, z = n deals (n * 321 365 < 2^31 at create, so n <= 6 682)
    hipLaunchKernelGGL(k_team_cross_play<Addr>, dim3(pairs, kSubtrees, (unsigned)n), dim3(kSubThreads), 0, ctx->stream, d_policies, table, n_pol, d_map, d_r2, d_sc, d_sub);
    SC_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_team_cross_top<Addr>, dim3(pairs, (unsigned)n), dim3(kSubThreads), 0, ctx->stream, d_policies, table, n_pol, d_map, (const double *)d_sub,
                       mean ? d_img : d_out);
    SC_HIP(ctx, hipGetLastError());
    if (mean) {
        const int cells = (int)pairs * kXQ;
        hipLaunchKernelGGL(k_team_cross_mean, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, ctx->stream, (const double *)d_img, n, cells, d_out);
        SC_HIP(ctx, hipGetLastError());
    }
    return SCOPA_OK;
}

template <class Addr, bool kDraw>
int32_t xp_match_launch(scopa_ctx *ctx, scopa_team_xplay_scratch *xp, int n_deals, const int32_t *d_map, const double *d_policy_a, const double *d_policy_b,
                        const int8_t *d_r2, int64_t n, int64_t n_team0, uint32_t stream_id, int32_t *d_deal_out, int32_t *d_leaf_out, int64_t *h_stats) {
    if (!xp->d_stats && hipMalloc(&xp->d_stats, sizeof(unsigned long long) * 16) != hipSuccess) {
        xp->d_stats = nullptr; (void)hipGetLastError();
        return fail(ctx, SCOPA_ENOMEM, "scopa_team match: no device memory for the sums");
    }
    SC_HIP(ctx, hipMemsetAsync(xp->d_stats, 0, sizeof(unsigned long long) * 10, ctx->stream));
    const long long n1 = n - n_team0;
    const int blocks0 = (int)std::min<long long>((n_team0 + 255) / 256, 2048), blocks1 = (int)std::min<long long>((n1 + 255) / 256, 2048);
    hipLaunchKernelGGL((k_team_match<Addr, kDraw>), dim3((unsigned)(blocks0 + blocks1)), dim3(256), 0, ctx->stream, (long long)n, (long long)n_team0, blocks0, n_deals, d_map,
                       d_policy_a, d_policy_b, d_r2, (const uint8_t *)xp->d_leaf_sc, (uint32_t)ctx->seed, (uint32_t)(ctx->seed >> 32), stream_id, d_deal_out, d_leaf_out,
                       xp->d_stats);
    SC_HIP(ctx, hipGetLastError());
    SC_HIP(ctx, hipMemcpyAsync(h_stats, xp->d_stats, sizeof(int64_t) * 10, hipMemcpyDeviceToHost, ctx->stream));
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SCOPA_OK;
}

}  // namespace

namespace scopa {
void team_xplay_release(scopa_team_xplay_scratch *xp) {
    void *bufs[] = {xp->d_leaf_sc, xp->d_sub, xp->d_img, xp->d_stats};
    for (void *b : bufs) if (b) (void)hipFree(b);
    *xp = scopa_team_xplay_scratch();
}
}  // namespace scopa

extern "C" {

int32_t scopa_team_debug_xplay_group_limit(scopa_ctx *ctx, int64_t groups) {
    if (!ctx || groups < 0) return SCOPA_EINVAL;
    ctx->team_xplay_group_limit = groups;
    return SCOPA_OK;
}

int32_t scopa_team_cross_play(scopa_ctx *ctx, int32_t n_pol, const double *d_policies, double *d_out) {
    if (!ctx || !d_policies || !d_out || n_pol < 1 || n_pol > 256) return SCOPA_EINVAL;
    SC_TEAM_READY(ctx, "scopa_team_cross_play");
    SC_REQUIRE(ctx, xp_aligned(d_policies), SCOPA_EINVAL, "scopa_team_cross_play: tables must be 32-byte aligned");
    const unsigned long long groups = (unsigned long long)kSubtrees * (unsigned long long)n_pol * (unsigned long long)n_pol;
    SC_REQUIRE(ctx, groups < xp_group_limit(ctx), SCOPA_ELIMIT, "scopa_team_cross_play: 256 * n_pol * n_pol must stay below 2^31 workgroups");
    if (int32_t rc = xp_leaves(ctx, t)) return rc;   // before the scratch: a refusal here leaves no scratch behind
    if (int32_t rc = xp_images(ctx, &t->xp, (size_t)groups * kXQ * sizeof(double), 0, "scopa_team_cross_play: no device memory for the subtree image")) return rc;
    return xp_cross_launch<OwnRows>(ctx, 1, n_pol, d_policies, (size_t)kTChoice * 4, nullptr, t->d_r2, t->xp.d_leaf_sc, t->xp.d_sub, nullptr, d_out, false);
}

int32_t scopa_team_match(scopa_ctx *ctx, const double *d_policy_a, const double *d_policy_b, int64_t n, int64_t n_team0, uint32_t stream_id, int32_t *d_leaf_out,
                         int64_t h_stats[10]) {
    if (!ctx || !d_policy_a || !d_policy_b || !h_stats || n < 0 || n_team0 < 0 || n_team0 > n) return SCOPA_EINVAL;
    SC_TEAM_READY(ctx, "scopa_team_match");
    SC_REQUIRE(ctx, xp_aligned(d_policy_a) && xp_aligned(d_policy_b), SCOPA_EINVAL, "scopa_team_match: tables must be 32-byte aligned");
    for (int j = 0; j < 10; j++) h_stats[j] = 0;
    if (!n) return SCOPA_OK;
    if (int32_t rc = xp_leaves(ctx, t)) return rc;
    return xp_match_launch<OwnRows, false>(ctx, &t->xp, 1, nullptr, d_policy_a, d_policy_b, t->d_r2, n, n_team0, stream_id, nullptr, d_leaf_out, h_stats);
}

int32_t scopa_team_chance_cross_play(scopa_team_chance *g, int32_t n_pol, const double *d_policies, double *d_per_deal, double *d_out) {
    if (!g || !d_policies || !d_out || n_pol < 1 || n_pol > 256) return SCOPA_EINVAL;
    scopa_ctx *ctx = g->ctx;
    SC_REQUIRE(ctx, xp_aligned(d_policies), SCOPA_EINVAL, "scopa_team_chance_cross_play: tables must be 32-byte aligned");
    const unsigned long long groups = (unsigned long long)kSubtrees * (unsigned long long)g->n * (unsigned long long)n_pol * (unsigned long long)n_pol;
    SC_REQUIRE(ctx, groups < xp_group_limit(ctx), SCOPA_ELIMIT, "scopa_team_chance_cross_play: 256 * n * n_pol * n_pol must stay below 2^31 workgroups");
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t img_bytes = d_per_deal ? 0 : (size_t)g->n * n_pol * n_pol * kXQ * sizeof(double);
    if (int32_t rc = xp_leaves(g)) return rc;   // before the scratch: a refusal here leaves no scratch behind
    if (int32_t rc = xp_images(ctx, &g->xp, (size_t)groups * kXQ * sizeof(double), img_bytes, "scopa_team_chance_cross_play: no device memory for the scratch images")) return rc;
    return xp_cross_launch<MappedRows>(ctx, g->n, n_pol, d_policies, (size_t)g->G * 4, g->d_map, g->d_r2, g->xp.d_leaf_sc, g->xp.d_sub, d_per_deal ? d_per_deal : g->xp.d_img,
                                       d_out, true);
}

int32_t scopa_team_chance_match(scopa_team_chance *g, const double *d_policy_a, const double *d_policy_b, int64_t n, int64_t n_team0, uint32_t stream_id,
                                int32_t *d_deal_out, int32_t *d_leaf_out, int64_t h_stats[10]) {
    if (!g || !d_policy_a || !d_policy_b || !h_stats || n < 0 || n_team0 < 0 || n_team0 > n) return SCOPA_EINVAL;
    scopa_ctx *ctx = g->ctx;
    SC_REQUIRE(ctx, xp_aligned(d_policy_a) && xp_aligned(d_policy_b), SCOPA_EINVAL, "scopa_team_chance_match: tables must be 32-byte aligned");
    for (int j = 0; j < 10; j++) h_stats[j] = 0;
    if (!n) return SCOPA_OK;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    if (int32_t rc = xp_leaves(g)) return rc;
    return xp_match_launch<MappedRows, true>(ctx, &g->xp, g->n, g->d_map, d_policy_a, d_policy_b, g->d_r2, n, n_team0, stream_id, d_deal_out, d_leaf_out, h_stats);
}

}  // extern "C"
