// scopa_full_eval_passes.h -- the passes of the exact FullScopa sweeps that do not read a deck or a key, ONE definition for the two translation units
// that sweep: scopa_full_eval.hip (one deck, one-word keys) and scopa_full_chance_eval.hip (a forest of one tree per deck, two-word keys).
//
//   shape     Shape / shape_of: the stored levels of `trees` trees of R rounds side by side.  Level k holds trees x (36^r x 1, 3, 9, 18) nodes, tree-major:
//             node g = d * (size[k] / trees) + i is node i of tree d, and since size[k + 1] = size[k] * n_k child a of node g is g n_k + a in the forest
//             exactly as in one tree.  So every pass below is the one-tree pass on longer arrays.
//   policy    full_eval_prob: prob[a] of a store row, by the match kernels' rule (which = 0) or by regret matching (which = 1); the slot type is the
//             caller's (FmSlot, FwSlot: the same row layout).
//   passes    k_full_eval_reach, _up, _weigh, _pick, a lane per node or sorted position, and full_eval_reduce, the body of a reduce kernel: the lane at
//             the head of a key's segment adds the segment's products IN ORDER.  What a key is -- one word or two -- is the caller's `Keys` view.
//   sweeps    full_eval_reach_down and full_eval_sweep_up, the host loops over the levels; the caller passes the launch of its own reduce kernel.
// Node indices and segment bounds are uint32_t: the largest level either caller sweeps has 2^21 nodes (18 x 36^3 = 839 808 in one tree of R = 4;
// 18 x 36^(R-1) x decks <= 2^21 in a forest, whose leaves are capped at 2^22).
#pragma once
#include <algorithm>

#include "scopa_ctx.h"
#include "scopa_mccfr_sigma.h"

namespace scopa_full {
namespace {

constexpr int kMaxRounds = 4;            // 36^4 = 1 679 616 leaves
constexpr int kMaxLevels = 4 * kMaxRounds;
constexpr unsigned kKeySortBits = 59;    // within a level the player and the round are constant: bits 0..58 tell its keys (word A of a pair) apart

// prob[0..2] of the row in `slot` (< 0: the store does not hold the key) for a mover with n cards; slots at and above n are left as the rule leaves
// them and the callers store 0.0 there
template <class Slot>
__device__ __forceinline__ void full_eval_prob(const Slot *__restrict__ tab, int slot, int n, int which, double pr[4]) {
    if (which == 0) {                                             // k_full_mccfr_match's rule
#pragma unroll
        for (int k = 0; k < 3; k++) pr[k] = 1.0 / (double)n;
        if (slot >= 0) {
            double S[3], total = 0.0;
#pragma unroll
            for (int k = 0; k < 3; k++) { S[k] = tab[slot].strategy[k]; if (k < n) total += S[k]; }
            if (total > 1e-12) {
#pragma unroll
                for (int k = 0; k < 3; k++) pr[k] = S[k] / total;
            }
        }
    } else {                                                      // the traversal's sigma: an absent key is a zero row
        double R[4];
#pragma unroll
        for (int k = 0; k < 3; k++) R[k] = slot >= 0 ? tab[slot].regret[k] : 0.0;
        R[3] = 0.0;
        scopa::mc_sigma(R, n, pr);
    }
}

// w of the children of a level; prob = NULL where the level's mover is the responder (or: pass the parent's reach on)
__global__ void __launch_bounds__(256)
k_full_eval_reach(const double *__restrict__ w_parent, const double *__restrict__ prob, uint32_t N, int n, double *__restrict__ w_child, uint32_t n_child) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_child) return;
    const uint32_t i = c / (uint32_t)n, a = c - i * (uint32_t)n;
    double w = w_parent[i];
    if (prob) w = w * prob[(size_t)a * N + i];
    w_child[c] = w;
}

__device__ __forceinline__ double child_value(const double *Vc, uint32_t c, int neg) {
    const double x = Vc[c];
    return neg ? -x : x;
}

__global__ void __launch_bounds__(256)
k_full_eval_up(const double *__restrict__ Vc, int neg, const double *__restrict__ prob, uint32_t N, int n, double *__restrict__ V) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    double v = 0.0;
#pragma unroll
    for (int a = 0; a < 3; a++)
        if (a < n) v += prob[(size_t)a * N + i] * child_value(Vc, i * (uint32_t)n + (uint32_t)a, neg);
    V[i] = v;
}

// the per-key sums of a responder level, in three launches.  weigh, a lane per sorted position k: the products w[node] * V[child a] of the node at k,
// stored in SORTED order (slot-major), so that the gathers run in parallel and the serial part below streams contiguous memory
__global__ void __launch_bounds__(256)
k_full_eval_weigh(const uint32_t *__restrict__ snode, uint32_t N, int n, const double *__restrict__ w, const double *__restrict__ Vc, int neg,
                  double *__restrict__ prod) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= N) return;
    const uint32_t i = snode[k], c = i * (uint32_t)n;
    const double wi = w[i];
    prod[k] = wi * child_value(Vc, c, neg);
    prod[(size_t)N + k] = wi * child_value(Vc, c + 1u, neg);
    if (n > 2) prod[2 * (size_t)N + k] = wi * child_value(Vc, c + 2u, neg);
}

// reduce: the lane at the head of a key's segment finds the segment's end (the keys are sorted: gallop, then bisect), adds the segment's products
// serially IN ORDER -- ascending node index, the sort being stable -- takes the first maximal slot, marks every position of the segment with it and
// appends the row.  Keys: same(x, y) -- do sorted positions x and y hold one key -- and put(r, x) -- write the key at x as row r's
template <class Keys>
__device__ __forceinline__ void full_eval_reduce(const Keys K, uint32_t N, int n, const double *__restrict__ prod, uint8_t *__restrict__ sbest,
                                                 unsigned int *__restrict__ cursor, uint32_t row_cap, int32_t *__restrict__ row_act, double *__restrict__ row_q) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N) return;
    if (j > 0u && K.same(j - 1u, j)) return;
    uint32_t lo = j, hi = N;                                       // position lo holds the key; hi == N or position hi does not
    for (uint32_t stride = 1u;; stride <<= 1) {
        const uint32_t t = lo + stride;                            // (N <= 2^21: no overflow)
        if (t >= N) break;
        if (!K.same(t, j)) { hi = t; break; }
        lo = t;
    }
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (K.same(mid, j)) lo = mid; else hi = mid;
    }
    const double *__restrict__ p0 = prod, *__restrict__ p1 = prod + N, *__restrict__ p2 = prod + 2 * (size_t)N;
    double q0 = 0.0, q1 = 0.0, q2 = 0.0;
    if (n > 2) {
#pragma unroll 8
        for (uint32_t k = j; k < hi; k++) { q0 += p0[k]; q1 += p1[k]; q2 += p2[k]; }
    } else {
#pragma unroll 8
        for (uint32_t k = j; k < hi; k++) { q0 += p0[k]; q1 += p1[k]; }
    }
    uint32_t best = 0u;                                            // the first maximal slot
    double qb = q0;
    if (q1 > qb) { best = 1u; qb = q1; }
    if (n > 2 && q2 > qb) best = 2u;
    for (uint32_t k = j; k < hi; k++) sbest[k] = (uint8_t)best;
    const uint32_t r = atomicAdd(cursor, 1u);
    if (r < row_cap) {
        K.put(r, j);
        row_act[r] = (int32_t)best;
        row_q[3 * (size_t)r] = q0; row_q[3 * (size_t)r + 1] = q1; row_q[3 * (size_t)r + 2] = q2;
    }
}

// pick, a lane per sorted position: the node there takes the value of its key's chosen child
__global__ void __launch_bounds__(256)
k_full_eval_pick(const uint32_t *__restrict__ snode, const uint8_t *__restrict__ sbest, uint32_t N, int n, const double *__restrict__ Vc, int neg,
                 double *__restrict__ V) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= N) return;
    const uint32_t i = snode[k];
    V[i] = child_value(Vc, i * (uint32_t)n + (uint32_t)sbest[k], neg);
}

struct Shape {
    int R = 0, L = 0;
    uint32_t size[kMaxLevels + 1];        // nodes of stored level k; size[L] = the leaves
    size_t off[kMaxLevels + 1];           // nodes before level k; off[L] = T
    uint32_t largest = 0, row_cap[2] = {0, 0};
};

// `trees` trees of R rounds side by side (trees x 36^R <= 2^22)
inline Shape shape_of(int R, uint32_t trees = 1u) {
    static const uint32_t mult[4] = {1u, 3u, 9u, 18u};
    Shape s;
    s.R = R; s.L = 4 * R;
    uint32_t base = trees;
    size_t at = 0;
    for (int k = 0; k < s.L; k++) {
        if (k && k % 4 == 0) base *= 36u;
        s.size[k] = base * mult[k % 4];
        s.off[k] = at;
        at += s.size[k];
        s.largest = std::max(s.largest, s.size[k]);
        s.row_cap[k & 1] += s.size[k];
    }
    s.size[s.L] = base * 36u;
    s.off[s.L] = at;
    return s;
}

inline int mover_of(int k) { return k & 1; }
inline int cards_of(int k) { return (k & 3) < 2 ? 3 : 2; }
inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }
inline dim3 grid_of(uint32_t n) { return dim3((n + 255u) / 256u); }

#define EV_LAUNCHED(ctx, name)                                                        \
    do {                                                                              \
        const hipError_t e__ = hipGetLastError();                                     \
        if (e__ != hipSuccess) return scopa::fail((ctx), SCOPA_EHIP, name, e__);      \
    } while (0)

// the arrays the level loops below run on; level k's part of a per-node array starts at off[k] (prob: 3 off[k], slot-major within the level)
struct EvalArrays {
    uint32_t *d_snode = nullptr;          // per level, the nodes grouped by key
    double *d_prob = nullptr, *d_w = nullptr, *d_V = nullptr, *d_leaf = nullptr;
    double *d_prod = nullptr;             // the largest level's products
    uint8_t *d_sbest = nullptr;           // ... and chosen slots
};

// top down: w of every level below the roots for the response of player p (w of level 0 is the caller's)
inline int32_t full_eval_reach_down(scopa_ctx *ctx, const Shape &s, const EvalArrays &e, int p) {
    for (int k = 0; k + 1 < s.L; k++) {
        hipLaunchKernelGGL(k_full_eval_reach, grid_of(s.size[k + 1]), dim3(256), 0, ctx->stream, (const double *)(e.d_w + s.off[k]),
                           mover_of(k) == p ? (const double *)nullptr : (const double *)(e.d_prob + 3 * s.off[k]), s.size[k], cards_of(k),
                           e.d_w + s.off[k + 1], s.size[k + 1]);
        EV_LAUNCHED(ctx, "k_full_eval_reach");
    }
    return SCOPA_OK;
}

// bottom up: the value pass (responder = -1) or the response pass of `responder`; the roots' values are left at the head of V.
// reduce(k, N, n, p) launches the caller's reduce kernel on level k and returns hipGetLastError()
template <class Reduce>
inline int32_t full_eval_sweep_up(scopa_ctx *ctx, const Shape &s, const EvalArrays &e, int responder, Reduce reduce) {
    hipStream_t st = ctx->stream;
    for (int k = s.L - 1; k >= 0; k--) {
        const bool leaves = k + 1 == s.L;
        const double *Vc = leaves ? e.d_leaf : e.d_V + s.off[k + 1];
        const int neg = leaves && responder == 1, n = cards_of(k), p = mover_of(k);
        const uint32_t N = s.size[k];
        if (p == responder) {
            const uint32_t *snode = e.d_snode + s.off[k];
            hipLaunchKernelGGL(k_full_eval_weigh, grid_of(N), dim3(256), 0, st, snode, N, n, (const double *)(e.d_w + s.off[k]), Vc, neg, e.d_prod);
            EV_LAUNCHED(ctx, "k_full_eval_weigh");
            const hipError_t err = reduce(k, N, n, p);
            if (err != hipSuccess) return scopa::fail(ctx, SCOPA_EHIP, "k_full_eval_reduce", err);
            hipLaunchKernelGGL(k_full_eval_pick, grid_of(N), dim3(256), 0, st, snode, (const uint8_t *)e.d_sbest, N, n, Vc, neg, e.d_V + s.off[k]);
            EV_LAUNCHED(ctx, "k_full_eval_pick");
        } else {
            hipLaunchKernelGGL(k_full_eval_up, grid_of(N), dim3(256), 0, st, Vc, neg, (const double *)(e.d_prob + 3 * s.off[k]), N, n, e.d_V + s.off[k]);
            EV_LAUNCHED(ctx, "k_full_eval_up");
        }
    }
    return SCOPA_OK;
}

}  // namespace
}  // namespace scopa_full
