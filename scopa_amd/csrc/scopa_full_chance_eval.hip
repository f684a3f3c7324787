// scopa_full_chance_eval.hip -- FullScopa over a set of decks: the exact value of the stored policy with the deal as a uniform chance move, and an exact
// pure response to it for either player ACROSS the decks: the responder plays one action at all histories that share the pair (A, B), on every deck
// (scopa_full_chance_exploitability, scopa_full_chance_response_get in include/scopa.h, where the procedure that defines the bits is stated).
//
// It is scopa_full_eval.hip's sweep over a FOREST, one tree per evaluated deck, and the passes that read neither a deck nor a key are that file's own
// (scopa_full_eval_passes.h: one definition).
//
//   forest    with n decks stored level k has n x size[k] nodes, deck-major: node g = d size[k] + i is node i of deck d's tree, and because
//             size[k + 1] = size[k] n_k child a of g is g n_k + a, as in one tree.  The deck of a node is g / size[k].
//   roots     k_full_chance_eval_roots, a lane per deck: root_on(root, deck d), and w = 1.0 for the response passes (the uniform chance weight 1 / n
//             is applied once, at the end).
//   expand    k_full_chance_eval_expand, a lane per child: the deck from the child's index, the mover's a-th card in ASCENDING CARD ID (sorted_hand) --
//             slot a then means the same card on every deck that shares the pair -- one step, three at a round's last choice level.
//   policy    k_full_chance_eval_policy, a lane per node: wide_key, the read-only probe fw_find, prob by full_eval_prob.
//   grouping  a level's nodes are grouped by pair with two stable rocPRIM radix_sort_pairs passes: by B over bits 0..39, then by A over bits 0..58
//             with A gathered through the first pass's permutation (k_full_chance_eval_gather); B is gathered through the final order.  Both passes
//             being stable, a pair's nodes stay in ascending g: deck by deck, and within a deck in node order.
//   response  reach, up, weigh and pick are the shared kernels; k_full_chance_eval_reduce is the shared body with a segment test on both words.  A
//             pair's segment adds nodes of several decks: the serial part is a plain loop of one vector lane over contiguous products.
//   means     k_full_chance_eval_mean, one lane: (0.0 + V[root 0] + V[root 1] + ...) / n in deck order.
// roots, expand, gather and mean are in scopa_full_chance_forest.h, one definition shared with scopa_full_chance_cfr.hip.
// No float64 atomic anywhere: the same decks in the same order give the same bits.  A permuted deck list regroups the adds and may change the last bits.
//
// IMPERFECT RECALL, as in scopa_full_eval.hip: for R > 1 the level-by-level argmax is A pure response whose value is exact, and (BR0 + BR1) / 2 is a
// lower bound.  At R = 1 all six remaining cards are dealt, so a hand fixes the opponent's: decks that share a pair are one game up to hand order, and
// the response across decks is the per-split best response.  Hidden hands begin to matter at R >= 2.
//
// Scratch (one allocation, kept in the handle, grown when a call needs more, freed by destroy), with n decks, T = 31 n (36^R - 1) / 35 stored nodes,
// n 36^R leaves and M = 18 n 36^(R-1) nodes in the largest level:
//   168 T + 8 n 36^R + 57 M + 40 n bytes + the sort's own (every part rounded up to 256 bytes, one more 256 for the cursors and results):
//   states 64 T, sorted pairs 16 T, sorted nodes 4 T, prob 24 T, w 8 T, V 8 T, response rows 44 T, leaf values, for the largest level its unsorted
//   pairs and nodes (20 bytes a node), the passes' intermediate keys and permutation (12), products (24) and chosen slots (1), and the decks.
#include <string.h>

#include <algorithm>
#include <new>
#include <numeric>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>

#include "scopa_ctx.h"
#include "scopa_full_chance_forest.h"
#include "scopa_full_eval_passes.h"
#include "scopa_full_wide.h"

using namespace scopa_full;
using scopa::fail;

namespace {

__global__ void __launch_bounds__(256)
k_full_chance_eval_policy(const scopa_full_state *__restrict__ st, uint32_t N, int p, int n, const FwSlot *__restrict__ tab, uint32_t mask, int which,
                          unsigned long long *__restrict__ a_out, unsigned long long *__restrict__ b_out, uint32_t *__restrict__ node_out,
                          double *__restrict__ prob) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const scopa_full_state s = st[i];
    const WideKey key = wide_key(s, p);
    const int slot = fw_find(tab, mask, key.a, key.b);
    double pr[4];
    full_eval_prob(tab, slot, n, which, pr);
    a_out[i] = key.a;
    b_out[i] = key.b;
    node_out[i] = i;
#pragma unroll
    for (int k = 0; k < 3; k++) prob[(size_t)k * N + i] = k < n ? pr[k] : 0.0;
}

struct TwoWords {                         // full_eval_reduce's view of a level's sorted pairs
    const unsigned long long *sa, *sb;
    unsigned long long *row_a, *row_b;
    __device__ __forceinline__ bool same(uint32_t x, uint32_t y) const { return sa[x] == sa[y] && sb[x] == sb[y]; }
    __device__ __forceinline__ void put(uint32_t r, uint32_t x) const { row_a[r] = sa[x]; row_b[r] = sb[x]; }
};

__global__ void __launch_bounds__(256)
k_full_chance_eval_reduce(const unsigned long long *__restrict__ sa, const unsigned long long *__restrict__ sb, uint32_t N, int n,
                          const double *__restrict__ prod, uint8_t *__restrict__ sbest, unsigned int *__restrict__ cursor, uint32_t row_cap,
                          unsigned long long *__restrict__ row_a, unsigned long long *__restrict__ row_b, int32_t *__restrict__ row_act,
                          double *__restrict__ row_q) {
    full_eval_reduce(TwoWords{sa, sb, row_a, row_b}, N, n, prod, sbest, cursor, row_cap, row_act, row_q);
}

}  // namespace

namespace scopa_full {

struct FwEval : EvalArrays {
    char *d_buf = nullptr;
    size_t bytes = 0, sort_bytes = 0;
    scopa_full_state *d_state = nullptr;
    unsigned long long *d_sa = nullptr, *d_sb = nullptr;                  // per level, the pairs in grouped order
    unsigned long long *d_ain = nullptr, *d_bin = nullptr, *d_ktmp = nullptr;
    uint32_t *d_nin = nullptr, *d_perm = nullptr;
    unsigned long long *d_row_a[2] = {nullptr, nullptr}, *d_row_b[2] = {nullptr, nullptr};
    int32_t *d_row_act[2] = {nullptr, nullptr};
    double *d_row_q[2] = {nullptr, nullptr};
    unsigned int *d_cursor = nullptr;                                     // 2 cursors, then (at byte 64) BR0, BR1, value
    double *d_res = nullptr;
    uint8_t *d_decks = nullptr;                                           // a call's own decks
    void *d_sort = nullptr;
    // host words the stream copies to
    double res[3] = {0.0, 0.0, 0.0};
    unsigned int n_rows[2] = {0u, 0u};
    bool have_rows = false;
};

void chance_eval_free(FwEval *e) {
    if (!e) return;
    if (e->d_buf) (void)hipFree(e->d_buf);
    delete e;
}

}  // namespace scopa_full

namespace {

// the scratch of a forest of shape s over n decks: laid out anew for every call, allocated anew only when the call needs more than the handle holds
int32_t ensure(scopa_full_chance *h, const Shape &s, uint32_t n) {
    if (!h->eval) {
        h->eval = new (std::nothrow) FwEval;
        if (!h->eval) return fail(h->ctx, SCOPA_ENOMEM, "scopa_full_chance_exploitability: host record");
    }
    FwEval *e = h->eval;
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
    const size_t o_state = take(64 * T), o_sa = take(8 * T), o_sb = take(8 * T), o_snode = take(4 * T), o_prob = take(24 * T), o_w = take(8 * T),
                 o_V = take(8 * T), o_leaf = take(8 * (size_t)s.size[s.L]), o_ain = take(8 * M), o_bin = take(8 * M), o_nin = take(4 * M),
                 o_ktmp = take(8 * M), o_perm = take(4 * M), o_prod = take(24 * M), o_sbest = take(M),
                 o_ra0 = take(8 * (size_t)s.row_cap[0]), o_ra1 = take(8 * (size_t)s.row_cap[1]), o_rb0 = take(8 * (size_t)s.row_cap[0]),
                 o_rb1 = take(8 * (size_t)s.row_cap[1]), o_rc0 = take(4 * (size_t)s.row_cap[0]), o_rc1 = take(4 * (size_t)s.row_cap[1]),
                 o_rq0 = take(24 * (size_t)s.row_cap[0]), o_rq1 = take(24 * (size_t)s.row_cap[1]), o_cursor = take(256),
                 o_decks = take(40 * (size_t)n + 24), o_sort = take(sort_bytes);
    if (!e->d_buf || e->bytes < at) {
        SC_HIP(h->ctx, hipStreamSynchronize(h->ctx->stream));
        if (e->d_buf) { (void)hipFree(e->d_buf); e->d_buf = nullptr; e->bytes = 0; }
        e->have_rows = false;
        char *buf = nullptr;
        const hipError_t err = hipMalloc((void **)&buf, at);
        if (err != hipSuccess) return fail(h->ctx, SCOPA_ENOMEM, "scopa_full_chance_exploitability: scratch of the forest", err);
        e->d_buf = buf; e->bytes = at;
    }
    char *buf = e->d_buf;
    e->sort_bytes = sort_bytes;
    e->d_state = (scopa_full_state *)(buf + o_state);
    e->d_sa = (unsigned long long *)(buf + o_sa); e->d_sb = (unsigned long long *)(buf + o_sb);
    e->d_snode = (uint32_t *)(buf + o_snode);
    e->d_prob = (double *)(buf + o_prob);
    e->d_w = (double *)(buf + o_w);
    e->d_V = (double *)(buf + o_V);
    e->d_leaf = (double *)(buf + o_leaf);
    e->d_ain = (unsigned long long *)(buf + o_ain); e->d_bin = (unsigned long long *)(buf + o_bin);
    e->d_nin = (uint32_t *)(buf + o_nin);
    e->d_ktmp = (unsigned long long *)(buf + o_ktmp);
    e->d_perm = (uint32_t *)(buf + o_perm);
    e->d_prod = (double *)(buf + o_prod);
    e->d_sbest = (uint8_t *)(buf + o_sbest);
    e->d_row_a[0] = (unsigned long long *)(buf + o_ra0); e->d_row_a[1] = (unsigned long long *)(buf + o_ra1);
    e->d_row_b[0] = (unsigned long long *)(buf + o_rb0); e->d_row_b[1] = (unsigned long long *)(buf + o_rb1);
    e->d_row_act[0] = (int32_t *)(buf + o_rc0); e->d_row_act[1] = (int32_t *)(buf + o_rc1);
    e->d_row_q[0] = (double *)(buf + o_rq0); e->d_row_q[1] = (double *)(buf + o_rq1);
    e->d_cursor = (unsigned int *)(buf + o_cursor);
    e->d_res = (double *)(buf + o_cursor + 64);
    e->d_decks = (uint8_t *)(buf + o_decks);
    e->d_sort = buf + o_sort;
    return SCOPA_OK;
}

// bottom up: the value pass (responder = -1) or the response pass of `responder`, then the mean of the roots into res[slot]
int32_t sweep_up(scopa_full_chance *h, const Shape &s, uint32_t n, int responder, int slot) {
    FwEval *e = h->eval;
    hipStream_t st = h->ctx->stream;
    const int32_t rc = full_eval_sweep_up(h->ctx, s, *e, responder, [&](int k, uint32_t N, int n_act, int p) {
        hipLaunchKernelGGL(k_full_chance_eval_reduce, grid_of(N), dim3(256), 0, st, (const unsigned long long *)(e->d_sa + s.off[k]),
                           (const unsigned long long *)(e->d_sb + s.off[k]), N, n_act, (const double *)e->d_prod, e->d_sbest, e->d_cursor + p, s.row_cap[p],
                           e->d_row_a[p], e->d_row_b[p], e->d_row_act[p], e->d_row_q[p]);
        return hipGetLastError();
    });
    if (rc != SCOPA_OK) return rc;
    hipLaunchKernelGGL(k_full_chance_eval_mean, dim3(1), dim3(64), 0, st, (const double *)e->d_V, n, e->d_res + slot);
    EV_LAUNCHED(h->ctx, "k_full_chance_eval_mean");
    SC_HIP(h->ctx, hipMemcpyAsync(&e->res[slot], e->d_res + slot, 8, hipMemcpyDeviceToHost, st));
    return SCOPA_OK;
}

}  // namespace

extern "C" {

int32_t scopa_full_chance_exploitability(scopa_full_chance *h, const scopa_full_state *root_state, const uint8_t *h_decks, int32_t k, int32_t which,
                                         double h_out4[4]) {
    if (!h || !h_out4) return SCOPA_EINVAL;
    SC_REQUIRE(h->ctx, which == 0 || which == 1, SCOPA_EINVAL, "scopa_full_chance_exploitability: which outside {0 (average policy), 1 (current sigma)}");
    const uint8_t *decks = h_decks ? h_decks : h->decks;
    if (!h_decks) k = h->n_decks;
    SC_REQUIRE(h->ctx, k >= 1, SCOPA_EINVAL, "scopa_full_chance_exploitability: k below 1");
    scopa_full_state root = root_state ? *root_state : h->root;
    SC_REQUIRE(h->ctx, root_ok(root), SCOPA_EINVAL, "scopa_full_chance_exploitability: the root must be a non-terminal state at a round boundary (step % 6 == 0)");
    root.game = 0u;
    const int R = 6 - (int)root.round;
    SC_REQUIRE(h->ctx, R <= kMaxRounds, SCOPA_ELIMIT, "scopa_full_chance_exploitability: more than 4 rounds from the root (36^R histories a deck are swept whole)");
    uint64_t leaves = (uint64_t)k;
    for (int r = 0; r < R; r++) leaves *= 36ull;                  // (k < 2^31, 36^4 < 2^21: no overflow)
    SC_REQUIRE(h->ctx, leaves <= kMaxLeaves, SCOPA_ELIMIT, "scopa_full_chance_exploitability: decks x 36^R above 1 << 22 (89 decks at R = 3, 2 at R = 4)");
    for (int32_t d = 0; d < k; d++)
        SC_REQUIRE(h->ctx, deck_fits(decks + 40 * (size_t)d, root), SCOPA_EINVAL,
                   "scopa_full_chance_exploitability: a deck does not pass create's check against the root of the call");
    SC_HIP(h->ctx, hipSetDevice(h->ctx->device));
    const uint32_t n = (uint32_t)k;
    const Shape s = shape_of(R, n);
    int32_t rc = ensure(h, s, n);
    if (rc != SCOPA_OK) return rc;
    FwEval *e = h->eval;
    hipStream_t st = h->ctx->stream;
    const uint32_t mask = (1u << h->capacity_log2) - 1u;
    e->have_rows = false;
    const uint8_t *d_decks = h->d_decks;
    if (h_decks) {
        SC_HIP(h->ctx, hipMemcpyAsync(e->d_decks, h_decks, 40 * (size_t)n, hipMemcpyHostToDevice, st));
        d_decks = e->d_decks;
    }
    SC_HIP(h->ctx, hipMemsetAsync(e->d_cursor, 0, 256, st));
    hipLaunchKernelGGL(k_full_chance_eval_roots, grid_of(n), dim3(256), 0, st, root, d_decks, n, e->d_state, e->d_w);
    EV_LAUNCHED(h->ctx, "k_full_chance_eval_roots");
    // 1, 2: expand, key + policy, group each level's nodes by pair
    for (int lv = 0; lv < s.L; lv++) {
        const int n_act = cards_of(lv), p = mover_of(lv);
        const bool leaf = lv + 1 == s.L;
        const uint32_t N = s.size[lv];
        hipLaunchKernelGGL(k_full_chance_eval_expand, grid_of(s.size[lv + 1]), dim3(256), 0, st, (const scopa_full_state *)(e->d_state + s.off[lv]), s.size[lv + 1],
                           s.size[lv + 1] / n, p, n_act, (int)((lv & 3) == 3), d_decks, leaf ? (scopa_full_state *)nullptr : e->d_state + s.off[lv + 1],
                           leaf ? e->d_leaf : (double *)nullptr);
        EV_LAUNCHED(h->ctx, "k_full_chance_eval_expand");
        hipLaunchKernelGGL(k_full_chance_eval_policy, grid_of(N), dim3(256), 0, st, (const scopa_full_state *)(e->d_state + s.off[lv]), N, p, n_act,
                           (const FwSlot *)h->d_tab, mask, (int)which, e->d_ain, e->d_bin, e->d_nin, e->d_prob + 3 * s.off[lv]);
        EV_LAUNCHED(h->ctx, "k_full_chance_eval_policy");
        size_t b = e->sort_bytes;
        SC_HIP(h->ctx, rocprim::radix_sort_pairs(e->d_sort, b, e->d_bin, e->d_ktmp, e->d_nin, e->d_perm, (size_t)N, 0u, kHandSortBits, st));
        hipLaunchKernelGGL(k_full_chance_eval_gather, grid_of(N), dim3(256), 0, st, (const unsigned long long *)e->d_ain, (const uint32_t *)e->d_perm, N, e->d_ktmp);
        EV_LAUNCHED(h->ctx, "k_full_chance_eval_gather");
        b = e->sort_bytes;
        SC_HIP(h->ctx, rocprim::radix_sort_pairs(e->d_sort, b, e->d_ktmp, e->d_sa + s.off[lv], e->d_perm, e->d_snode + s.off[lv], (size_t)N, 0u, kKeySortBits, st));
        hipLaunchKernelGGL(k_full_chance_eval_gather, grid_of(N), dim3(256), 0, st, (const unsigned long long *)e->d_bin, (const uint32_t *)(e->d_snode + s.off[lv]), N,
                           e->d_sb + s.off[lv]);
        EV_LAUNCHED(h->ctx, "k_full_chance_eval_gather");
    }
    // 3: the policy against itself
    if ((rc = sweep_up(h, s, n, -1, 2)) != SCOPA_OK) return rc;
    // 4: the response of player 0, then of player 1 (w of the roots is 1.0 from k_full_chance_eval_roots: no pass writes level 0 of w)
    for (int p = 0; p < 2; p++) {
        if ((rc = full_eval_reach_down(h->ctx, s, *e, p)) != SCOPA_OK) return rc;
        if ((rc = sweep_up(h, s, n, p, p)) != SCOPA_OK) return rc;
    }
    SC_HIP(h->ctx, hipMemcpyAsync(e->n_rows, e->d_cursor, 8, hipMemcpyDeviceToHost, st));
    SC_HIP(h->ctx, hipStreamSynchronize(st));
    SC_REQUIRE(h->ctx, e->n_rows[0] <= s.row_cap[0] && e->n_rows[1] <= s.row_cap[1], SCOPA_ESTATE, "scopa_full_chance_exploitability: more response rows than nodes");
    h_out4[0] = (e->res[0] + e->res[1]) / 2.0;
    h_out4[1] = e->res[0];
    h_out4[2] = e->res[1];
    h_out4[3] = e->res[2];
    e->have_rows = true;
    return SCOPA_OK;
}

int32_t scopa_full_chance_response_get(scopa_full_chance *h, int32_t player, int64_t *n_rows, uint64_t *keys2, int32_t *n_act, int32_t *action, double *q) {
    if (!h || !n_rows) return SCOPA_EINVAL;
    SC_REQUIRE(h->ctx, player == 0 || player == 1, SCOPA_EINVAL, "scopa_full_chance_response_get: player outside {0, 1}");
    SC_REQUIRE(h->ctx, h->eval && h->eval->have_rows, SCOPA_ESTATE, "scopa_full_chance_response_get: no scopa_full_chance_exploitability call has completed on this handle");
    FwEval *e = h->eval;
    const int64_t room = *n_rows, n = (int64_t)e->n_rows[player];
    *n_rows = n;
    if (!keys2 && !n_act && !action && !q) return SCOPA_OK;              // the count alone
    SC_REQUIRE(h->ctx, room >= n, SCOPA_EINVAL, "scopa_full_chance_response_get: *n_rows is below the rows of the response (now in *n_rows)");
    if (!n) return SCOPA_OK;
    std::vector<uint64_t> ka, kb;
    std::vector<int32_t> a;
    std::vector<double> Q;
    std::vector<uint32_t> order;
    try { ka.resize((size_t)n); kb.resize((size_t)n); a.resize((size_t)n); Q.resize(3 * (size_t)n); order.resize((size_t)n); }
    catch (const std::bad_alloc &) { return fail(h->ctx, SCOPA_ENOMEM, "scopa_full_chance_response_get: host image of the rows"); }
    SC_HIP(h->ctx, hipSetDevice(h->ctx->device));
    SC_HIP(h->ctx, hipMemcpyAsync(ka.data(), e->d_row_a[player], 8 * (size_t)n, hipMemcpyDeviceToHost, h->ctx->stream));
    SC_HIP(h->ctx, hipMemcpyAsync(kb.data(), e->d_row_b[player], 8 * (size_t)n, hipMemcpyDeviceToHost, h->ctx->stream));
    SC_HIP(h->ctx, hipMemcpyAsync(a.data(), e->d_row_act[player], 4 * (size_t)n, hipMemcpyDeviceToHost, h->ctx->stream));
    SC_HIP(h->ctx, hipMemcpyAsync(Q.data(), e->d_row_q[player], 24 * (size_t)n, hipMemcpyDeviceToHost, h->ctx->stream));
    SC_HIP(h->ctx, hipStreamSynchronize(h->ctx->stream));
    std::iota(order.begin(), order.end(), 0u);
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return ka[x] != ka[y] ? ka[x] < ka[y] : kb[x] < kb[y]; });   // (pairs are distinct: one row per pair)
    for (int64_t i = 0; i < n; i++) {
        const uint32_t r = order[(size_t)i];
        if (keys2) { keys2[2 * i] = ka[r]; keys2[2 * i + 1] = kb[r]; }
        if (n_act) n_act[i] = popc64(kb[r]);
        if (action) action[i] = a[r];
        if (q) for (int c = 0; c < 3; c++) q[3 * i + c] = Q[3 * (size_t)r + c];
    }
    return SCOPA_OK;
}

}  // extern "C"
