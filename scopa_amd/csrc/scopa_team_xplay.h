// scopa_team_xplay.h -- the ONE definition of what scopa_team_xplay.hip runs on Team MiniScopa: the four-quantity upward sweep of a depth-4 subtree,
// the finish of depths 3..0, and the episode walk of a sampled match.  Two kernels run each: one on a context's deal, one on a set of deals whose
// rows are shared by key.  They differ in where a deal's local row lives in a policy table, and that is the ADDRESSING POLICY of
// scopa_team_mccfr_walk.h, a template parameter here as there:
//
//   OwnRows      a local row is its own table row (policies [SCOPA_TEAM_N_CHOICE][4])
//   MappedRows   a local row goes through the deal's map row (policies [G][4])
//
// Four float64 quantities per node: the reward of team 0, its square, the scopas of team 0 and of team 1; at a depth-12 node, after its four forced
// plies, they are 0.5 * r2, 0.25 * r2 * r2 and the two nibbles of the leaf scopa byte.  Per node and quantity the arithmetic is value_node's kFollow
// (scopa_team_passes.h): v = 0.0; v += row[c] * child[c], children left to right, rows as given, the padding slots c >= b not read into the sum.
#pragma once
#include <string.h>

#include "scopa_philox.h"
#include "scopa_team_mccfr_walk.h"
#include "scopa_team_passes.h"
#include "scopa_tree_passes.h"

namespace {

constexpr int kXQ = 4;   // quantities per node

// ---- leaf scopas -----------------------------------------------------------------------------------------------------------------------------
// depth-12 node i of the deal, its four forced plies played out: scopas of team 0's two seats in the low nibble, of team 1's in the high nibble
// (a team plays 8 cards, so neither sum exceeds 8)
__device__ __forceinline__ uint8_t team_leaf_scopas(const scopa_team_state &root, int i) {
    uint32_t w[10];
    memcpy(w, &root, 40);
    team_walk(w, 12, i, scopa_team::kPlies);
    const uint32_t sc = w[8];
    const uint32_t t0 = (sc & 255u) + ((sc >> 8) & 255u), t1 = ((sc >> 16) & 255u) + (sc >> 24);
    return (uint8_t)((t0 & 15u) | ((t1 & 15u) << 4));
}

struct Quad { double q[kXQ]; };
__device__ __forceinline__ Quad leaf_quad(int r2, uint32_t sc) {
    return Quad{{0.5 * (double)r2, 0.25 * (double)(r2 * r2), (double)(sc & 15u), (double)(sc >> 4)}};
}

// one node with B legal slots: the four quantities from its children's, under the row of the table of the team that moves
template <int B>
__device__ __forceinline__ Quad follow_quad(const Row4 &row, const Quad *child) {
    Quad v;
#pragma unroll
    for (int q = 0; q < kXQ; q++) {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < B; c++) s += row.x[c] * child[c].q[q];
        v.q[q] = s;
    }
    return v;
}

__device__ __forceinline__ Quad lds_quad(const double *s_val, int node) {
    const double4 v = *reinterpret_cast<const double4 *>(s_val + (size_t)node * kXQ);
    return Quad{{v.x, v.y, v.z, v.w}};
}
__device__ __forceinline__ void lds_quad_store(double *s_val, int node, const Quad &v) {
    *reinterpret_cast<double4 *>(s_val + (size_t)node * kXQ) = make_double4(v.q[0], v.q[1], v.q[2], v.q[3]);
}

// ---- the sweep of depth-4 subtree g: s_val[kSubRows][4], the subtree's rows level-major as in s_offset ---------------------------------------------
// Every row is read once, straight from the table of the team that moves, through the addressing policy.  A lane owns at most 3 + 2 + 1 x 6 = 11 rows of
// the eight levels (648, 324, 162, 81, 27, 9, 3, 1 rows over 256 lanes); it asks for all of them before the first level is computed, so the map -> row
// round trips to memory overlap instead of standing in front of each of the eight barriers.
template <int D> __host__ __device__ constexpr int x_rounds() { return (s_width(D) + kSubThreads - 1) / kSubThreads; }

template <int D, class Addr>
__device__ __forceinline__ void xsub_rows(int g, const Addr &addr, const double *pol_a, const double *pol_b, int tid, Row4 (&rows)[x_rounds<D>()]) {
    constexpr int w = s_width(D);
    const double *tab = t_team(D) == 0 ? pol_a : pol_b;
#pragma unroll
    for (int r = 0; r < x_rounds<D>(); r++) {
        const int j = tid + r * kSubThreads;
        rows[r] = Row4{{0.0, 0.0, 0.0, 0.0}};
        if (j < w) rows[r] = load_row(tab + addr.at((size_t)t_offset(D) + (size_t)g * w + j) * 4);
    }
}

template <int D>
__device__ __forceinline__ void xsub_level(int g, const Row4 (&rows)[x_rounds<D>()], const int8_t *g_r2 /* the deal's */, const uint8_t *g_sc /* the deal's */, double *s_val,
                                           int tid) {
    constexpr int b = t_branch(D), w = s_width(D), lo = s_offset(D);
#pragma unroll
    for (int r = 0; r < x_rounds<D>(); r++) {
        const int j = tid + r * kSubThreads;
        if (j >= w) break;
        Quad child[b];
        if constexpr (D == 11) {
            const size_t leaf = (size_t)g * kSubLeaves + (size_t)j * b;
#pragma unroll
            for (int c = 0; c < b; c++) child[c] = leaf_quad(g_r2[leaf + c], g_sc[leaf + c]);
        } else {
#pragma unroll
            for (int c = 0; c < b; c++) child[c] = lds_quad(s_val, s_offset(D + 1) + j * b + c);
        }
        lds_quad_store(s_val, lo + j, follow_quad<b>(rows[r], child));
    }
    __syncthreads();
}

template <class Addr>
__device__ __forceinline__ void xsub_sweep(int g, const Addr &addr, const double *pol_a, const double *pol_b, const int8_t *g_r2, const uint8_t *g_sc, double *s_val,
                                           int tid) {
    Row4 r11[x_rounds<11>()], r10[x_rounds<10>()], r9[x_rounds<9>()], r8[x_rounds<8>()], r7[x_rounds<7>()], r6[x_rounds<6>()], r5[x_rounds<5>()], r4[x_rounds<4>()];
#define SC_XROWS(D, rows) xsub_rows<D>(g, addr, pol_a, pol_b, tid, rows)
    SC_XROWS(11, r11); SC_XROWS(10, r10); SC_XROWS(9, r9); SC_XROWS(8, r8); SC_XROWS(7, r7); SC_XROWS(6, r6); SC_XROWS(5, r5); SC_XROWS(4, r4);
#undef SC_XROWS
#define SC_XSUB(D, rows) xsub_level<D>(g, rows, g_r2, g_sc, s_val, tid)
    SC_XSUB(11, r11); SC_XSUB(10, r10); SC_XSUB(9, r9); SC_XSUB(8, r8); SC_XSUB(7, r7); SC_XSUB(6, r6); SC_XSUB(5, r5); SC_XSUB(4, r4);
#undef SC_XSUB
}

// ---- depths 3..0 from the 256 subtree values: s_val[kTopRows + kSubtrees][4], the subtree values behind the 85 rows -----------------------------------
template <class Addr>
__device__ __forceinline__ void xtop_sweep(const Addr &addr, const double *pol_a, const double *pol_b, double *s_val, int tid) {
#pragma unroll
    for (int d = kCutDepth - 1; d >= 0; d--) {
        const double *tab = t_team(d) == 0 ? pol_a : pol_b;
        for (int j = tid; j < t_width(d); j += kSubThreads) {
            const Row4 row = load_row(tab + addr.at((size_t)(t_offset(d) + j)) * 4);
            Quad child[4];
#pragma unroll
            for (int c = 0; c < 4; c++) child[c] = lds_quad(s_val, t_offset(d + 1) + j * 4 + c);
            lds_quad_store(s_val, t_offset(d) + j, follow_quad<4>(row, child));
        }
        __syncthreads();
    }
}

// ---- the episode walk of a match -------------------------------------------------------------------------------------------------------------
// Episode i with policy a as team `a_team`: ply d draws at Philox counter (i, i >> 32, 32 + d, stream) under the key; N is the 53-bit integer of
// u53(x0, x1); the action is #{k < b - 1 : thr[k] <= N} with thr = policy_thresholds(b, row) of the mover's team's table row (a row that sums to 0 or
// NaN plays slot 0).  Returns the depth-12 index the episode ends at.
constexpr uint32_t kXMatchTag = 32u, kXDealTag = 44u;   // tags 32..43 the plies, 44 the deal: clear of the two-player match's 0..8 under one stream id

template <int D, class Addr>
__device__ __forceinline__ void xmatch_ply(const Addr &addr, const double *pol_a, const double *pol_b, int a_team, long long i, uint32_t stream, uint32_t seed_lo,
                                           uint32_t seed_hi, int &idx) {
    constexpr int b = t_branch(D);
    const scopa::philox_out x = scopa::philox4x32_10((uint32_t)i, (uint32_t)((unsigned long long)i >> 32), kXMatchTag + (uint32_t)D, stream, seed_lo, seed_hi);
    const Row4 row = load_row((t_team(D) == a_team ? pol_a : pol_b) + addr.at((size_t)(t_offset(D) + idx)) * 4);
    unsigned long long thr[3];
    scopa::policy_thresholds(b, row.x, thr);
    const unsigned long long N = ((unsigned long long)(x.x0 >> 5) << 26) | (unsigned long long)(x.x1 >> 6);   // u = N * 2^-53
    int a = 0;
#pragma unroll
    for (int k = 0; k < b - 1; k++) a += thr[k] <= N ? 1 : 0;
    idx = idx * b + a;
}

template <class Addr>
__device__ __forceinline__ int xmatch_walk(const Addr &addr, const double *pol_a, const double *pol_b, int a_team, long long i, uint32_t stream, uint32_t seed_lo,
                                           uint32_t seed_hi) {
    int idx = 0;
#define SC_XPLY(D) xmatch_ply<D>(addr, pol_a, pol_b, a_team, i, stream, seed_lo, seed_hi, idx)
    SC_XPLY(0); SC_XPLY(1); SC_XPLY(2); SC_XPLY(3); SC_XPLY(4); SC_XPLY(5); SC_XPLY(6); SC_XPLY(7); SC_XPLY(8); SC_XPLY(9); SC_XPLY(10); SC_XPLY(11);
#undef SC_XPLY
    return idx;
}

// the addressing policy of deal `deal`: the map is not read by OwnRows
template <class Addr> __device__ __forceinline__ Addr xaddr(const int32_t *g_map, size_t deal);
template <> __device__ __forceinline__ OwnRows xaddr<OwnRows>(const int32_t *, size_t) { return OwnRows{}; }
template <> __device__ __forceinline__ MappedRows xaddr<MappedRows>(const int32_t *g_map, size_t deal) { return MappedRows{g_map + deal * kTChoice}; }

}  // namespace
