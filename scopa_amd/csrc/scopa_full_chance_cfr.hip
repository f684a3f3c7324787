// scopa_full_chance_cfr.hip -- FullScopa over a set of decks: the exact, weighted CFR iteration on a sub-game of R <= 4 rounds with the deal a uniform
// chance move over the handle's decks (scopa_full_chance_cfr_iterate in include/scopa.h, where the procedure that defines the bits is stated).
//
// It runs on scopa_full_chance_eval.hip's FOREST -- one tree per deck, deck-major, child a of node g at g n_k + a, slot a the mover's a-th card in
// ascending card id (scopa_full_chance_forest.h: one definition of roots, expand, gather and mean) -- in two parts:
//
//   set-up, once per call
//     expand    the forest, level by level, and the leaf values.
//     keys      k_full_chance_cfr_keys, a lane per node: wide_key.  A level's nodes are then grouped by pair with the two stable radix sorts of the
//               exploitability sweep, so a pair's nodes are contiguous and in ascending g.
//     rows      k_full_chance_cfr_rows, the lane at the head of a pair's segment: gallop and bisect to the segment's end ONCE, claim the pair in the
//               store (fw_claim), copy its regret and strategy row into the call's compact arrays and freeze its first sigma (mc_sigma).  A row of
//               the call is named by the SORTED POSITION of its head: end[j] = the segment's end at a head and 0 elsewhere, rowof[g] = the head of
//               node g's pair (4 bytes a node), slot[j] = the store slot.  The compact rows are slot-major per level ([3][N], 24 bytes a row), so
//               the iteration never probes the store and never touches a 128-byte slot.
//     One host synchronisation ends the set-up: a dropped claim makes the call return SCOPA_ENOMEM before anything is computed.
//
//   the loop, per sweep (two an alternating iteration, one a simultaneous one); nothing in it copies to or from the host
//     reach     k_full_chance_cfr_reach, a lane per child, top down: BOTH reaches in one launch -- w0 multiplies by sigma at player 0's levels, w1 at
//               player 1's; sigma gathered through rowof.
//     up        bottom up.  A level whose rows the sweep does not update: k_full_chance_cfr_up, a lane per node, v = 0.0; v += sigma[a] * child[a].
//               A level it updates: k_full_chance_cfr_weigh, a lane per SORTED position, computes the same v for its node, stores it, and writes the
//               node's 2 n products w_opp (x[child a] - x[g]) and w_own sigma[a] in sorted order (slot-major), so the serial part streams; then
//               k_full_chance_cfr_update, the head lane of each pair: adds the segment's products serially IN ORDER (ascending g), applies
//               R <- R + dR; R <- !(R <= 0) ? R pos : R neg; S <- (S + dS) strat, and stores the row's NEXT sigma -- nothing later in the sweep reads
//               this level's sigma, so no separate policy pass runs.  The head is the row's only writer: plain vector stores, no atomic.
//     mean      k_full_chance_eval_mean of the roots' values into the call's value array.
//   store     after the last iteration k_full_chance_cfr_store, the head lanes again: the compact rows back into their slots, plain stores.
// No float64 atomic anywhere: the same handle state gives the same bits.  Launches an iteration at R rounds, L = 4 R levels: alternating
// 2 (L - 1 + L + L / 2 + 1) = 5 L (60 at R = 3), simultaneous L - 1 + 2 L + 2 = 3 L + 1.
//
// Bytes a sweep moves, with T stored nodes, leaves = n 36^R and U the nodes of the levels it updates (T / 2 alternating on average, T simultaneous):
// reach 44 T (two parents, a row id and a sigma per child, two stores), up 8 leaves + 40 T, weigh and update another 2 x 48 U + 100 U.  The small
// forests are bound by the launch count, not by this.
//
// IMPERFECT RECALL, as in scopa_full_chance_eval.hip: the pair forgets the player's own plays of earlier rounds, so for R > 1 CFR has no convergence
// proof on these rows; the figure to watch is the lower bound (BR0 + BR1) / 2 of scopa_full_chance_exploitability.
//
// Scratch (one allocation, kept in the handle, grown when a call needs more, freed by destroy), with n decks, T = 31 n (36^R - 1) / 35 stored nodes,
// n 36^R leaves, M = 18 n 36^(R-1) nodes in the largest level and I = n_iters:
//   192 T + 8 n 36^R + 80 M + 40 I bytes + the sort's own (every part rounded up to 256 bytes):
//   states 64 T, sorted pairs 16 T, sorted nodes 4 T, rowof 4 T, end 4 T, slot 4 T, regret, strategy and sigma rows 72 T, w0 and w1 16 T, V 8 T, leaf
//   values, for the largest level its unsorted pairs and nodes (20 bytes a node), the passes' intermediate keys and permutation (12) and the products
//   (48), the weights (24 I) and the sweep values (16 I).
#include <string.h>

#include <algorithm>
#include <new>

#include <rocprim/device/device_radix_sort.hpp>

#include "scopa_ctx.h"
#include "scopa_full_chance_forest.h"
#include "scopa_full_eval_passes.h"
#include "scopa_full_store_host.h"
#include "scopa_full_wide.h"

using namespace scopa_full;
using scopa::fail;

namespace {

constexpr int32_t kMaxIters = 1 << 20;

__global__ void __launch_bounds__(256)
k_full_chance_cfr_keys(const scopa_full_state *__restrict__ st, uint32_t N, int p, unsigned long long *__restrict__ a_out,
                       unsigned long long *__restrict__ b_out, uint32_t *__restrict__ node_out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const scopa_full_state s = st[i];
    const WideKey key = wide_key(s, p);
    a_out[i] = key.a;
    b_out[i] = key.b;
    node_out[i] = i;
}

// the head of a pair's segment (the pairs are sorted: gallop, then bisect, as full_eval_reduce) claims the pair, names every node of the segment its
// row and loads the row; rows are [3][N] slot-major.  snode[k] < N: a permutation of the level's nodes
__global__ void __launch_bounds__(256)
k_full_chance_cfr_rows(const unsigned long long *__restrict__ sa, const unsigned long long *__restrict__ sb, const uint32_t *__restrict__ snode, uint32_t N,
                       int n, FwSlot *__restrict__ tab, uint32_t mask, unsigned long long *__restrict__ cnt, uint32_t *__restrict__ rowof,
                       uint32_t *__restrict__ end, int32_t *__restrict__ slot_of, double *__restrict__ Rc, double *__restrict__ Sc, double *__restrict__ sig) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N) return;
    const unsigned long long a = sa[j], b = sb[j];
    if (j > 0u && sa[j - 1u] == a && sb[j - 1u] == b) { end[j] = 0u; return; }
    uint32_t lo = j, hi = N;                                       // position lo holds the pair; hi == N or position hi does not
    for (uint32_t stride = 1u;; stride <<= 1) {
        const uint32_t t = lo + stride;                            // (N <= 2^21: no overflow)
        if (t >= N) break;
        if (!(sa[t] == a && sb[t] == b)) { hi = t; break; }
        lo = t;
    }
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (sa[mid] == a && sb[mid] == b) lo = mid; else hi = mid;
    }
    end[j] = hi;
    for (uint32_t k = j; k < hi; k++) rowof[snode[k]] = j;
    const int slot = fw_claim(tab, mask, a, b, cnt);
    slot_of[j] = slot;
    double R[4], pr[4];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        R[c] = slot >= 0 ? tab[slot].regret[c] : 0.0;
        Rc[(size_t)c * N + j] = R[c];
        Sc[(size_t)c * N + j] = slot >= 0 ? tab[slot].strategy[c] : 0.0;
    }
    R[3] = 0.0;
    scopa::mc_sigma(R, n, pr);
#pragma unroll
    for (int c = 0; c < 3; c++) sig[(size_t)c * N + j] = c < n ? pr[c] : 0.0;
}

// both reaches of the children of a level: w_mover multiplies by sigma, the other passes the parent's on
__global__ void __launch_bounds__(256)
k_full_chance_cfr_reach(const double *__restrict__ w0_parent, const double *__restrict__ w1_parent, const double *__restrict__ sig,
                        const uint32_t *__restrict__ rowof, uint32_t N, int n, int mover, double *__restrict__ w0_child, double *__restrict__ w1_child,
                        uint32_t n_child) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_child) return;
    const uint32_t i = c / (uint32_t)n, a = c - i * (uint32_t)n;
    const double pr = sig[(size_t)a * N + rowof[i]];
    double w0 = w0_parent[i], w1 = w1_parent[i];
    if (mover == 0) w0 = w0 * pr; else w1 = w1 * pr;
    w0_child[c] = w0;
    w1_child[c] = w1;
}

__global__ void __launch_bounds__(256)
k_full_chance_cfr_up(const double *__restrict__ Vc, const double *__restrict__ sig, const uint32_t *__restrict__ rowof, uint32_t N, int n,
                     double *__restrict__ V) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const uint32_t r = rowof[i];
    double v = 0.0;
#pragma unroll
    for (int a = 0; a < 3; a++)
        if (a < n) v += sig[(size_t)a * N + r] * Vc[i * (uint32_t)n + (uint32_t)a];
    V[i] = v;
}

// a lane per sorted position k of a level the sweep updates: the value of the node there, and its products in SORTED order, prod [6][N]:
// rows 0..2 w_opp (x[child a] - x[g]), rows 3..5 w_own sigma[a]; x = V for p = 0, -V for p = 1
__global__ void __launch_bounds__(256)
k_full_chance_cfr_weigh(const uint32_t *__restrict__ snode, const uint32_t *__restrict__ rowof, uint32_t N, int n, int p, const double *__restrict__ sig,
                        const double *__restrict__ w_opp, const double *__restrict__ w_own, const double *__restrict__ Vc, double *__restrict__ V,
                        double *__restrict__ prod) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= N) return;
    const uint32_t i = snode[k], r = rowof[i];
    double pr[3], c[3], v = 0.0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        pr[a] = a < n ? sig[(size_t)a * N + r] : 0.0;
        c[a] = a < n ? Vc[i * (uint32_t)n + (uint32_t)a] : 0.0;
        if (a < n) v += pr[a] * c[a];
    }
    V[i] = v;
    const double xg = p ? -v : v, wo = w_opp[i], ws = w_own[i];
#pragma unroll
    for (int a = 0; a < 3; a++)
        if (a < n) {
            const double xc = p ? -c[a] : c[a];
            prod[(size_t)a * N + k] = wo * (xc - xg);
            prod[(size_t)(3 + a) * N + k] = ws * pr[a];
        }
}

// the head of each pair's segment: the serial in-order sums, the weighted update of its row and the row's next sigma.  wt = (pos, neg, strat) of the
// iteration, NULL = all 1.0
__global__ void __launch_bounds__(256)
k_full_chance_cfr_update(const uint32_t *__restrict__ end, uint32_t N, int n, const double *__restrict__ prod, const double *__restrict__ wt,
                         double *__restrict__ Rc, double *__restrict__ Sc, double *__restrict__ sig) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N) return;
    const uint32_t hi = end[j];                                    // (0 where j is not a head; else j < hi <= N)
    if (hi == 0u) return;
    const double *__restrict__ r0 = prod, *__restrict__ r1 = prod + N, *__restrict__ r2 = prod + 2 * (size_t)N;
    const double *__restrict__ s0 = prod + 3 * (size_t)N, *__restrict__ s1 = prod + 4 * (size_t)N, *__restrict__ s2 = prod + 5 * (size_t)N;
    double dR[3] = {0.0, 0.0, 0.0}, dS[3] = {0.0, 0.0, 0.0};
    if (n > 2) {
#pragma unroll 4
        for (uint32_t k = j; k < hi; k++) { dR[0] += r0[k]; dR[1] += r1[k]; dR[2] += r2[k]; dS[0] += s0[k]; dS[1] += s1[k]; dS[2] += s2[k]; }
    } else {
#pragma unroll 4
        for (uint32_t k = j; k < hi; k++) { dR[0] += r0[k]; dR[1] += r1[k]; dS[0] += s0[k]; dS[1] += s1[k]; }
    }
    const double w_pos = wt ? wt[0] : 1.0, w_neg = wt ? wt[1] : 1.0, w_strat = wt ? wt[2] : 1.0;
    double R[4], pr[4];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        R[a] = 0.0;
        if (a < n) {
            double r = Rc[(size_t)a * N + j] + dR[a];
            r = !(r <= 0.0) ? r * w_pos : r * w_neg;
            R[a] = r;
            Rc[(size_t)a * N + j] = r;
            Sc[(size_t)a * N + j] = (Sc[(size_t)a * N + j] + dS[a]) * w_strat;
        }
    }
    R[3] = 0.0;
    scopa::mc_sigma(R, n, pr);
#pragma unroll
    for (int a = 0; a < 3; a++)
        if (a < n) sig[(size_t)a * N + j] = pr[a];
}

// the compact rows back into their slots: the head lane is the slot's only writer (n_slots: the store's size, the bound of slot_of)
__global__ void __launch_bounds__(256)
k_full_chance_cfr_store(const uint32_t *__restrict__ end, const int32_t *__restrict__ slot_of, uint32_t N, int n, const double *__restrict__ Rc,
                        const double *__restrict__ Sc, FwSlot *__restrict__ tab, uint32_t n_slots) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N || end[j] == 0u) return;
    const int32_t slot = slot_of[j];
    if (slot < 0 || (uint32_t)slot >= n_slots) return;
#pragma unroll
    for (int a = 0; a < 3; a++)
        if (a < n) {
            tab[slot].regret[a] = Rc[(size_t)a * N + j];
            tab[slot].strategy[a] = Sc[(size_t)a * N + j];
        }
}

}  // namespace

namespace scopa_full {

struct FwCfr {
    char *d_buf = nullptr;
    size_t bytes = 0, sort_bytes = 0;
    scopa_full_state *d_state = nullptr;
    unsigned long long *d_sa = nullptr, *d_sb = nullptr;                  // per level, the pairs in grouped order
    uint32_t *d_snode = nullptr, *d_rowof = nullptr, *d_end = nullptr;
    int32_t *d_slot = nullptr;
    double *d_R = nullptr, *d_S = nullptr, *d_sig = nullptr;              // the call's rows: level k at 3 off[k], [3][size[k]]
    double *d_w[2] = {nullptr, nullptr}, *d_V = nullptr, *d_leaf = nullptr;
    unsigned long long *d_ain = nullptr, *d_bin = nullptr, *d_ktmp = nullptr;
    uint32_t *d_nin = nullptr, *d_perm = nullptr;
    double *d_prod = nullptr, *d_wt = nullptr, *d_val = nullptr;
    void *d_sort = nullptr;
};

void chance_cfr_free(FwCfr *c) {
    if (!c) return;
    if (c->d_buf) (void)hipFree(c->d_buf);
    delete c;
}

}  // namespace scopa_full

namespace {

int32_t ensure(scopa_full_chance *h, const Shape &s, size_t n_iters) {
    if (!h->cfr) {
        h->cfr = new (std::nothrow) FwCfr;
        if (!h->cfr) return fail(h->ctx, SCOPA_ENOMEM, "scopa_full_chance_cfr_iterate: host record");
    }
    FwCfr *c = h->cfr;
    const size_t T = s.off[s.L], M = s.largest;
    size_t sort_bytes = 256;
    for (int k = 0; k < s.L; k++) {
        size_t b = 0;
        SC_HIP(h->ctx, rocprim::radix_sort_pairs(nullptr, b, (unsigned long long *)nullptr, (unsigned long long *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr,
                                                 (size_t)s.size[k], 0u, kHandSortBits, h->ctx->stream));
        sort_bytes = std::max(sort_bytes, b);
        SC_HIP(h->ctx, rocprim::radix_sort_pairs(nullptr, b, (unsigned long long *)nullptr, (unsigned long long *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr,
                                                 (size_t)s.size[k], 0u, kKeySortBits, h->ctx->stream));
        sort_bytes = std::max(sort_bytes, b);
    }
    size_t at = 0;
    auto take = [&at](size_t b) { const size_t o = at; at += up256(b); return o; };
    const size_t o_state = take(64 * T), o_sa = take(8 * T), o_sb = take(8 * T), o_snode = take(4 * T), o_rowof = take(4 * T), o_end = take(4 * T),
                 o_slot = take(4 * T), o_R = take(24 * T), o_S = take(24 * T), o_sig = take(24 * T), o_w0 = take(8 * T), o_w1 = take(8 * T), o_V = take(8 * T),
                 o_leaf = take(8 * (size_t)s.size[s.L]), o_ain = take(8 * M), o_bin = take(8 * M), o_nin = take(4 * M), o_ktmp = take(8 * M),
                 o_perm = take(4 * M), o_prod = take(48 * M), o_wt = take(24 * n_iters), o_val = take(16 * n_iters), o_sort = take(sort_bytes);
    if (!c->d_buf || c->bytes < at) {
        SC_HIP(h->ctx, hipStreamSynchronize(h->ctx->stream));
        if (c->d_buf) { (void)hipFree(c->d_buf); c->d_buf = nullptr; c->bytes = 0; }
        char *buf = nullptr;
        const hipError_t err = hipMalloc((void **)&buf, at);
        if (err != hipSuccess) return fail(h->ctx, SCOPA_ENOMEM, "scopa_full_chance_cfr_iterate: scratch of the forest", err);
        c->d_buf = buf; c->bytes = at;
    }
    char *buf = c->d_buf;
    c->sort_bytes = sort_bytes;
    c->d_state = (scopa_full_state *)(buf + o_state);
    c->d_sa = (unsigned long long *)(buf + o_sa); c->d_sb = (unsigned long long *)(buf + o_sb);
    c->d_snode = (uint32_t *)(buf + o_snode); c->d_rowof = (uint32_t *)(buf + o_rowof); c->d_end = (uint32_t *)(buf + o_end);
    c->d_slot = (int32_t *)(buf + o_slot);
    c->d_R = (double *)(buf + o_R); c->d_S = (double *)(buf + o_S); c->d_sig = (double *)(buf + o_sig);
    c->d_w[0] = (double *)(buf + o_w0); c->d_w[1] = (double *)(buf + o_w1);
    c->d_V = (double *)(buf + o_V);
    c->d_leaf = (double *)(buf + o_leaf);
    c->d_ain = (unsigned long long *)(buf + o_ain); c->d_bin = (unsigned long long *)(buf + o_bin);
    c->d_nin = (uint32_t *)(buf + o_nin);
    c->d_ktmp = (unsigned long long *)(buf + o_ktmp);
    c->d_perm = (uint32_t *)(buf + o_perm);
    c->d_prod = (double *)(buf + o_prod);
    c->d_wt = (double *)(buf + o_wt);
    c->d_val = (double *)(buf + o_val);
    c->d_sort = buf + o_sort;
    return SCOPA_OK;
}

// steps 1, 2: the forest, each level's nodes grouped by pair, the pairs claimed and their rows loaded
int32_t set_up(scopa_full_chance *h, const Shape &s, uint32_t n, const scopa_full_state &root) {
    FwCfr *c = h->cfr;
    hipStream_t st = h->ctx->stream;
    const uint32_t mask = (1u << h->capacity_log2) - 1u;
    hipLaunchKernelGGL(k_full_chance_eval_roots, grid_of(n), dim3(256), 0, st, root, (const uint8_t *)h->d_decks, n, c->d_state, c->d_w[0]);
    EV_LAUNCHED(h->ctx, "k_full_chance_eval_roots");
    SC_HIP(h->ctx, hipMemcpyAsync(c->d_w[1], c->d_w[0], 8 * (size_t)n, hipMemcpyDeviceToDevice, st));
    for (int lv = 0; lv < s.L; lv++) {
        const int n_act = cards_of(lv), p = mover_of(lv);
        const bool leaf = lv + 1 == s.L;
        const uint32_t N = s.size[lv];
        const size_t o = s.off[lv];
        hipLaunchKernelGGL(k_full_chance_eval_expand, grid_of(s.size[lv + 1]), dim3(256), 0, st, (const scopa_full_state *)(c->d_state + o), s.size[lv + 1],
                           s.size[lv + 1] / n, p, n_act, (int)((lv & 3) == 3), (const uint8_t *)h->d_decks,
                           leaf ? (scopa_full_state *)nullptr : c->d_state + s.off[lv + 1], leaf ? c->d_leaf : (double *)nullptr);
        EV_LAUNCHED(h->ctx, "k_full_chance_eval_expand");
        hipLaunchKernelGGL(k_full_chance_cfr_keys, grid_of(N), dim3(256), 0, st, (const scopa_full_state *)(c->d_state + o), N, p, c->d_ain, c->d_bin, c->d_nin);
        EV_LAUNCHED(h->ctx, "k_full_chance_cfr_keys");
        size_t b = c->sort_bytes;
        SC_HIP(h->ctx, rocprim::radix_sort_pairs(c->d_sort, b, c->d_bin, c->d_ktmp, c->d_nin, c->d_perm, (size_t)N, 0u, kHandSortBits, st));
        hipLaunchKernelGGL(k_full_chance_eval_gather, grid_of(N), dim3(256), 0, st, (const unsigned long long *)c->d_ain, (const uint32_t *)c->d_perm, N, c->d_ktmp);
        EV_LAUNCHED(h->ctx, "k_full_chance_eval_gather");
        b = c->sort_bytes;
        SC_HIP(h->ctx, rocprim::radix_sort_pairs(c->d_sort, b, c->d_ktmp, c->d_sa + o, c->d_perm, c->d_snode + o, (size_t)N, 0u, kKeySortBits, st));
        hipLaunchKernelGGL(k_full_chance_eval_gather, grid_of(N), dim3(256), 0, st, (const unsigned long long *)c->d_bin, (const uint32_t *)(c->d_snode + o), N, c->d_sb + o);
        EV_LAUNCHED(h->ctx, "k_full_chance_eval_gather");
        hipLaunchKernelGGL(k_full_chance_cfr_rows, grid_of(N), dim3(256), 0, st, (const unsigned long long *)(c->d_sa + o), (const unsigned long long *)(c->d_sb + o),
                           (const uint32_t *)(c->d_snode + o), N, n_act, h->d_tab, mask, h->d_cnt, c->d_rowof + o, c->d_end + o, c->d_slot + o, c->d_R + 3 * o,
                           c->d_S + 3 * o, c->d_sig + 3 * o);
        EV_LAUNCHED(h->ctx, "k_full_chance_cfr_rows");
    }
    return SCOPA_OK;
}

// steps 3, 4: one sweep with sigma frozen and the update of the rows of `trav` (-1: of both players); its value into val[0] (and val[1] where given)
int32_t sweep(scopa_full_chance *h, const Shape &s, uint32_t n, int trav, const double *wt, double *val, double *val2) {
    FwCfr *c = h->cfr;
    hipStream_t st = h->ctx->stream;
    for (int k = 0; k + 1 < s.L; k++) {
        const size_t o = s.off[k], oc = s.off[k + 1];
        hipLaunchKernelGGL(k_full_chance_cfr_reach, grid_of(s.size[k + 1]), dim3(256), 0, st, (const double *)(c->d_w[0] + o), (const double *)(c->d_w[1] + o),
                           (const double *)(c->d_sig + 3 * o), (const uint32_t *)(c->d_rowof + o), s.size[k], cards_of(k), mover_of(k), c->d_w[0] + oc,
                           c->d_w[1] + oc, s.size[k + 1]);
        EV_LAUNCHED(h->ctx, "k_full_chance_cfr_reach");
    }
    for (int k = s.L - 1; k >= 0; k--) {
        const size_t o = s.off[k];
        const double *Vc = k + 1 == s.L ? c->d_leaf : c->d_V + s.off[k + 1];
        const int n_act = cards_of(k), p = mover_of(k);
        const uint32_t N = s.size[k];
        if (trav < 0 || p == trav) {
            hipLaunchKernelGGL(k_full_chance_cfr_weigh, grid_of(N), dim3(256), 0, st, (const uint32_t *)(c->d_snode + o), (const uint32_t *)(c->d_rowof + o), N, n_act, p,
                               (const double *)(c->d_sig + 3 * o), (const double *)(c->d_w[1 - p] + o), (const double *)(c->d_w[p] + o), Vc, c->d_V + o, c->d_prod);
            EV_LAUNCHED(h->ctx, "k_full_chance_cfr_weigh");
            hipLaunchKernelGGL(k_full_chance_cfr_update, grid_of(N), dim3(256), 0, st, (const uint32_t *)(c->d_end + o), N, n_act, (const double *)c->d_prod, wt,
                               c->d_R + 3 * o, c->d_S + 3 * o, c->d_sig + 3 * o);
            EV_LAUNCHED(h->ctx, "k_full_chance_cfr_update");
        } else {
            hipLaunchKernelGGL(k_full_chance_cfr_up, grid_of(N), dim3(256), 0, st, Vc, (const double *)(c->d_sig + 3 * o), (const uint32_t *)(c->d_rowof + o), N, n_act,
                               c->d_V + o);
            EV_LAUNCHED(h->ctx, "k_full_chance_cfr_up");
        }
    }
    hipLaunchKernelGGL(k_full_chance_eval_mean, dim3(1), dim3(64), 0, st, (const double *)c->d_V, n, val);
    EV_LAUNCHED(h->ctx, "k_full_chance_eval_mean");
    if (val2) {
        hipLaunchKernelGGL(k_full_chance_eval_mean, dim3(1), dim3(64), 0, st, (const double *)c->d_V, n, val2);
        EV_LAUNCHED(h->ctx, "k_full_chance_eval_mean");
    }
    return SCOPA_OK;
}

}  // namespace

extern "C" {

int32_t scopa_full_chance_cfr_iterate(scopa_full_chance *h, const scopa_full_state *root_state, int32_t n_iters, const double *h_w, int32_t alternating,
                                      double *h_values) {
    if (!h) return SCOPA_EINVAL;
    SC_REQUIRE(h->ctx, n_iters >= 0 && n_iters <= kMaxIters, SCOPA_EINVAL, "scopa_full_chance_cfr_iterate: n_iters outside [0, 1 << 20]");
    SC_REQUIRE(h->ctx, alternating == 0 || alternating == 1, SCOPA_EINVAL, "scopa_full_chance_cfr_iterate: alternating outside {0, 1}");
    SC_REQUIRE(h->ctx, !h_w || scopa::cfr_weights_ok(h_w, n_iters), SCOPA_EINVAL, "scopa_full_chance_cfr_iterate: a weight that is not finite or lies outside [0, 1]");
    scopa_full_state root = root_state ? *root_state : h->root;
    SC_REQUIRE(h->ctx, root_ok(root), SCOPA_EINVAL, "scopa_full_chance_cfr_iterate: the root must be a non-terminal state at a round boundary (step % 6 == 0)");
    root.game = 0u;
    const int R = 6 - (int)root.round;
    SC_REQUIRE(h->ctx, R <= kMaxRounds, SCOPA_ELIMIT, "scopa_full_chance_cfr_iterate: more than 4 rounds from the root (36^R histories a deck are swept whole)");
    uint64_t leaves = (uint64_t)h->n_decks;
    for (int r = 0; r < R; r++) leaves *= 36ull;                  // (n_decks <= 2^20, 36^4 < 2^21: no overflow)
    SC_REQUIRE(h->ctx, leaves <= kMaxLeaves, SCOPA_ELIMIT, "scopa_full_chance_cfr_iterate: decks x 36^R above 1 << 22 (89 decks at R = 3, 2 at R = 4)");
    for (int32_t d = 0; d < h->n_decks; d++)
        SC_REQUIRE(h->ctx, deck_fits(h->decks + 40 * (size_t)d, root), SCOPA_EINVAL,
                   "scopa_full_chance_cfr_iterate: a deck of the handle does not pass create's check against the root of the call");
    if (!n_iters) return SCOPA_OK;
    SC_HIP(h->ctx, hipSetDevice(h->ctx->device));
    const uint32_t n = (uint32_t)h->n_decks;
    const Shape s = shape_of(R, n);
    int32_t rc = ensure(h, s, (size_t)n_iters);
    if (rc != SCOPA_OK) return rc;
    FwCfr *c = h->cfr;
    hipStream_t st = h->ctx->stream;
    if ((rc = set_up(h, s, n, root)) != SCOPA_OK) return rc;
    // the claims are counted before anything is computed: the one synchronisation of the set-up
    if ((rc = check_dropped(h, "scopa_full_chance_cfr_iterate: the store is full along a probe (claims dropped, no row changed): create a larger one and tables_set")) != SCOPA_OK) return rc;
    if (h_w) SC_HIP(h->ctx, hipMemcpyAsync(c->d_wt, h_w, 24 * (size_t)n_iters, hipMemcpyHostToDevice, st));
    for (int32_t t = 0; t < n_iters; t++) {
        const double *wt = h_w ? c->d_wt + 3 * (size_t)t : (const double *)nullptr;
        double *val = c->d_val + 2 * (size_t)t;
        if (alternating) {
            if ((rc = sweep(h, s, n, 0, wt, val, nullptr)) != SCOPA_OK) return rc;
            if ((rc = sweep(h, s, n, 1, wt, val + 1, nullptr)) != SCOPA_OK) return rc;
        } else if ((rc = sweep(h, s, n, -1, wt, val, val + 1)) != SCOPA_OK) return rc;
    }
    for (int lv = 0; lv < s.L; lv++) {
        const size_t o = s.off[lv];
        hipLaunchKernelGGL(k_full_chance_cfr_store, grid_of(s.size[lv]), dim3(256), 0, st, (const uint32_t *)(c->d_end + o), (const int32_t *)(c->d_slot + o), s.size[lv],
                           cards_of(lv), (const double *)(c->d_R + 3 * o), (const double *)(c->d_S + 3 * o), h->d_tab, 1u << h->capacity_log2);
        EV_LAUNCHED(h->ctx, "k_full_chance_cfr_store");
    }
    if (h_values) SC_HIP(h->ctx, hipMemcpyAsync(h_values, c->d_val, 16 * (size_t)n_iters, hipMemcpyDeviceToHost, st));
    SC_HIP(h->ctx, hipStreamSynchronize(st));
    h->iteration += 2u * (uint32_t)n_iters;
    return SCOPA_OK;
}

}  // extern "C"
