// scopa_full_eval.hip -- FullScopa: the exact value of the stored policy on a sub-game, and an exact pure response to it for either player
// (scopa_full_mccfr_exploitability, scopa_full_mccfr_response_get in include/scopa.h, where the procedure that defines the bits is stated).
//
// A sub-game from the start of round r0 has R = 6 - r0 rounds, 36^R histories and a regular shape: movers alternate from player 0 and hold
// 3, 3, 2, 2, 1, 1 cards through a round.  So it is laid out level by level and swept by whole-level launches, as the team solvers do.
//
//   levels    only the levels where the mover has a choice are stored: 4 per round (sizes 36^r x 1, 3, 9, 18), 4 R in all, and the 36^R leaves as their
//             terminal value alone (8 bytes, not a 64-byte state).  The two one-card plies that end a round have one child each with the parent's
//             index and value, so the expansion of a round's last choice level plays them on the way: child a of node i is node i n + a of the next
//             stored level in the numbering of the header's procedure, whether or not the one-card levels exist.
//   expand    k_full_eval_expand, a lane per child: the parent's state, one step (three at a round's last choice level), state or leaf value out.
//   policy    k_full_eval_policy, a lane per node: infoset_key, the read-only probe fm_find (scopa_full_store.h), prob[a] by the match kernel's rule
//             (which = 0) or by regret matching of the regret row (which = 1); prob is kept slot-major (prob[a][node]) so that the sweeps read it
//             coalesced.  The level's (key, node) pairs are then grouped by rocPRIM's radix_sort_pairs, which is stable: within a key the nodes stay
//             in ascending index.
//   value     k_full_eval_up, a lane per node, bottom up: v = 0; v += prob[a] * child[a].
//   response  of player p: k_full_eval_reach top down (w of a child = w of its parent, times prob[a] below the other player's nodes), then bottom up
//             k_full_eval_up at the other player's levels and, at p's, three launches: k_full_eval_weigh (a lane per sorted position: the products
//             w[node] * V[child a], stored in sorted order), k_full_eval_reduce (the lane at the head of a key's segment adds the segment's products
//             IN ORDER, Q[a] += ..., takes the first maximal slot, marks the segment with it and appends the row -- an integer cursor: the rows come
//             out in any order and response_get sorts them by key) and k_full_eval_pick (every node takes its key's chosen child's value).  A sub-game
//             holds few keys for its nodes (10 961 rows for 1.5 million nodes from one round-2 root), so segments are thousands of nodes long: the
//             serial part is kept to a chain of adds over contiguous memory, the gathers to the parallel launches around it.
//             No float64 atomic anywhere: every sum has one order, so the results are bit-identical from run to run.
//   shared    the passes that read neither the deck nor the key word (reach, up, weigh, pick, the reduce's body, the prob rule, the level loops and
//             the level sizes) are in scopa_full_eval_passes.h, which scopa_full_chance_eval.hip runs over a forest of one tree per deck.
//
// IMPERFECT RECALL.  The key forgets the player's own plays of earlier rounds, so one key can hold nodes with different pasts of the responder.  Within a
// round the key determines them (the hand), so for R = 1 the level-by-level argmax IS the best response; for R > 1 it is A pure response -- each level
// maximises against the reach w that ignores the responder's own earlier choices -- whose value is computed exactly.  BR_p is always achieved by a real
// responder, (BR0 + BR1) / 2 is a lower bound on the exploitability, and nothing proves BR_p >= the policy's own value for R > 1.
//
// Scratch (one allocation, kept in the handle, grown when a larger R comes, freed by destroy), with T = 31 (36^R - 1) / 35 stored nodes:
// 152 T + 8 * 36^R + 37 * 18 * 36^(R-1) bytes + the sort's own: states 64 T, sorted keys 8 T, sorted nodes 4 T, prob 24 T, w 8 T, V 8 T,
// response rows 36 T, leaf values, and for the largest level its unsorted pairs (12 bytes a node), products (24) and chosen slots (1).
#include <string.h>

#include <algorithm>
#include <new>
#include <numeric>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>

#include "scopa_ctx.h"
#include "scopa_full_eval_passes.h"
#include "scopa_full_key.h"
#include "scopa_full_store.h"

using namespace scopa_full;
using scopa::fail;

namespace {

__global__ void __launch_bounds__(256)
k_full_eval_expand(const scopa_full_state *__restrict__ parent, uint32_t n_child, int p, int n, int round_end, const uint8_t *__restrict__ deck,
                   scopa_full_state *__restrict__ child, double *__restrict__ leaf) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_child) return;
    const uint32_t i = c / (uint32_t)n;
    const int a = (int)(c - i * (uint32_t)n);
    scopa_full_state s = parent[i];
    step(s, deck, hand_get(s, p, a));
    if (round_end) {                                              // the one-card plies: player 0's last card, then player 1's
        step(s, deck, hand_get(s, 0, 0));
        step(s, deck, hand_get(s, 1, 0));
    }
    if (leaf) leaf[c] = (double)s.r2_p0 / 2.0;
    else child[c] = s;
}

__global__ void __launch_bounds__(256)
k_full_eval_policy(const scopa_full_state *__restrict__ st, uint32_t N, int p, int n, const FmSlot *__restrict__ tab, uint32_t mask,
                   const uint8_t *__restrict__ deck, int which, unsigned long long *__restrict__ key_out, uint32_t *__restrict__ node_out,
                   double *__restrict__ prob) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const scopa_full_state s = st[i];
    const uint64_t key = infoset_key(s, deck, p);
    const int slot = fm_find(tab, mask, key);
    double pr[4];
    full_eval_prob(tab, slot, n, which, pr);
    key_out[i] = key;
    node_out[i] = i;
#pragma unroll
    for (int k = 0; k < 3; k++) prob[(size_t)k * N + i] = k < n ? pr[k] : 0.0;
}

struct OneWord {                          // full_eval_reduce's view of a level's sorted one-word keys
    const unsigned long long *skey;
    unsigned long long *row_key;
    __device__ __forceinline__ bool same(uint32_t x, uint32_t y) const { return skey[x] == skey[y]; }
    __device__ __forceinline__ void put(uint32_t r, uint32_t x) const { row_key[r] = skey[x]; }
};

__global__ void __launch_bounds__(256)
k_full_eval_reduce(const unsigned long long *__restrict__ skey, uint32_t N, int n, const double *__restrict__ prod, uint8_t *__restrict__ sbest,
                   unsigned int *__restrict__ cursor, uint32_t row_cap, unsigned long long *__restrict__ row_key, int32_t *__restrict__ row_act,
                   double *__restrict__ row_q) {
    full_eval_reduce(OneWord{skey, row_key}, N, n, prod, sbest, cursor, row_cap, row_act, row_q);
}

}  // namespace

namespace scopa_full {

struct FmEval : EvalArrays {
    int R = 0;                              // the scratch is laid out for sub-games up to R rounds
    char *d_buf = nullptr;
    size_t bytes = 0, sort_bytes = 0;
    scopa_full_state *d_state = nullptr;
    unsigned long long *d_skey = nullptr, *d_kin = nullptr, *d_row_key[2] = {nullptr, nullptr};
    uint32_t *d_nin = nullptr;
    int32_t *d_row_act[2] = {nullptr, nullptr};
    double *d_row_q[2] = {nullptr, nullptr};
    unsigned int *d_cursor = nullptr;
    void *d_sort = nullptr;
    // host words the stream copies from and to
    scopa_full_state root;
    double one = 1.0, res[3] = {0.0, 0.0, 0.0};
    unsigned int n_rows[2] = {0u, 0u};
    bool have_rows = false;
};

void eval_free(FmEval *e) {
    if (!e) return;
    if (e->d_buf) (void)hipFree(e->d_buf);
    delete e;
}

}  // namespace scopa_full

namespace {

// the scratch of a sub-game of R rounds (kept while R does not grow)
int32_t ensure(scopa_full_mccfr *h, int R) {
    if (!h->eval) {
        h->eval = new (std::nothrow) FmEval;
        if (!h->eval) return fail(h->ctx, SCOPA_ENOMEM, "scopa_full_mccfr_exploitability: host record");
    }
    FmEval *e = h->eval;
    if (e->d_buf && e->R >= R) return SCOPA_OK;
    const Shape s = shape_of(R);
    const size_t T = s.off[s.L];
    size_t sort_bytes = 0;
    for (int k = 0; k < s.L; k++) {
        size_t b = 0;
        SC_HIP(h->ctx, rocprim::radix_sort_pairs(nullptr, b, (unsigned long long *)nullptr, (unsigned long long *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr,
                                                 (size_t)s.size[k], 0u, kKeySortBits, h->ctx->stream));
        sort_bytes = std::max(sort_bytes, b);
    }
    size_t at = 0;
    auto take = [&at](size_t b) { const size_t o = at; at += up256(b); return o; };
    const size_t o_state = take(64 * T), o_skey = take(8 * T), o_snode = take(4 * T), o_prob = take(24 * T), o_w = take(8 * T), o_V = take(8 * T),
                 o_leaf = take(8 * (size_t)s.size[s.L]), o_kin = take(8 * (size_t)s.largest), o_nin = take(4 * (size_t)s.largest),
                 o_prod = take(24 * (size_t)s.largest), o_sbest = take((size_t)s.largest),
                 o_rk0 = take(8 * (size_t)s.row_cap[0]), o_rk1 = take(8 * (size_t)s.row_cap[1]), o_ra0 = take(4 * (size_t)s.row_cap[0]),
                 o_ra1 = take(4 * (size_t)s.row_cap[1]), o_rq0 = take(24 * (size_t)s.row_cap[0]), o_rq1 = take(24 * (size_t)s.row_cap[1]),
                 o_cursor = take(256), o_sort = take(std::max(sort_bytes, (size_t)256));
    SC_HIP(h->ctx, hipStreamSynchronize(h->ctx->stream));
    if (e->d_buf) { (void)hipFree(e->d_buf); e->d_buf = nullptr; e->R = 0; e->have_rows = false; }
    char *buf = nullptr;
    const hipError_t err = hipMalloc((void **)&buf, at);
    if (err != hipSuccess) return fail(h->ctx, SCOPA_ENOMEM, "scopa_full_mccfr_exploitability: scratch of the sub-game", err);
    e->d_buf = buf; e->bytes = at; e->sort_bytes = std::max(sort_bytes, (size_t)256); e->R = R;
    e->d_state = (scopa_full_state *)(buf + o_state);
    e->d_skey = (unsigned long long *)(buf + o_skey);
    e->d_snode = (uint32_t *)(buf + o_snode);
    e->d_prob = (double *)(buf + o_prob);
    e->d_w = (double *)(buf + o_w);
    e->d_V = (double *)(buf + o_V);
    e->d_leaf = (double *)(buf + o_leaf);
    e->d_kin = (unsigned long long *)(buf + o_kin);
    e->d_nin = (uint32_t *)(buf + o_nin);
    e->d_prod = (double *)(buf + o_prod);
    e->d_sbest = (uint8_t *)(buf + o_sbest);
    e->d_row_key[0] = (unsigned long long *)(buf + o_rk0); e->d_row_key[1] = (unsigned long long *)(buf + o_rk1);
    e->d_row_act[0] = (int32_t *)(buf + o_ra0); e->d_row_act[1] = (int32_t *)(buf + o_ra1);
    e->d_row_q[0] = (double *)(buf + o_rq0); e->d_row_q[1] = (double *)(buf + o_rq1);
    e->d_cursor = (unsigned int *)(buf + o_cursor);
    e->d_sort = buf + o_sort;
    return SCOPA_OK;
}

// bottom up: the value pass (responder = -1) or the response pass of `responder`; the root's value is left in V[0]
int32_t sweep_up(scopa_full_mccfr *h, const Shape &s, int responder) {
    FmEval *e = h->eval;
    hipStream_t st = h->ctx->stream;
    return full_eval_sweep_up(h->ctx, s, *e, responder, [&](int k, uint32_t N, int n, int p) {
        hipLaunchKernelGGL(k_full_eval_reduce, grid_of(N), dim3(256), 0, st, (const unsigned long long *)(e->d_skey + s.off[k]), N, n,
                           (const double *)e->d_prod, e->d_sbest, e->d_cursor + p, s.row_cap[p], e->d_row_key[p], e->d_row_act[p], e->d_row_q[p]);
        return hipGetLastError();
    });
}

}  // namespace

extern "C" {

int32_t scopa_full_mccfr_exploitability(scopa_full_mccfr *h, const scopa_full_state *root_state, int32_t which, double h_out4[4]) {
    if (!h || !h_out4) return SCOPA_EINVAL;
    SC_REQUIRE(h->ctx, which == 0 || which == 1, SCOPA_EINVAL, "scopa_full_mccfr_exploitability: which outside {0 (average policy), 1 (current sigma)}");
    scopa_full_state root = root_state ? *root_state : h->root;
    const int bad = root_check(root, h->deck);
    SC_REQUIRE(h->ctx, bad != 1, SCOPA_EINVAL, "scopa_full_mccfr_exploitability: the root must be a non-terminal state at a round boundary (step % 6 == 0)");
    SC_REQUIRE(h->ctx, bad != 2, SCOPA_EINVAL, "scopa_full_mccfr_exploitability: the root's hands are not the handle's deck's deal of its round");
    root.game = 0u;
    const int R = 6 - (int)root.round;
    SC_REQUIRE(h->ctx, R <= kMaxRounds, SCOPA_ELIMIT, "scopa_full_mccfr_exploitability: more than 4 rounds from the root (36^R histories are swept whole)");
    SC_HIP(h->ctx, hipSetDevice(h->ctx->device));
    int32_t rc = ensure(h, R);
    if (rc != SCOPA_OK) return rc;
    FmEval *e = h->eval;
    hipStream_t st = h->ctx->stream;
    const Shape s = shape_of(R);
    const uint32_t mask = (1u << h->capacity_log2) - 1u;
    e->have_rows = false;
    e->root = root;
    SC_HIP(h->ctx, hipMemsetAsync(e->d_cursor, 0, 256, st));
    SC_HIP(h->ctx, hipMemcpyAsync(e->d_state, &e->root, sizeof(scopa_full_state), hipMemcpyHostToDevice, st));
    // 1, 2: expand, key + policy, group each level's nodes by key
    for (int k = 0; k < s.L; k++) {
        const int n = cards_of(k), p = mover_of(k);
        const bool leaves = k + 1 == s.L;
        hipLaunchKernelGGL(k_full_eval_expand, grid_of(s.size[k + 1]), dim3(256), 0, st, (const scopa_full_state *)(e->d_state + s.off[k]), s.size[k + 1], p, n,
                           (int)((k & 3) == 3), (const uint8_t *)h->d_deck, leaves ? (scopa_full_state *)nullptr : e->d_state + s.off[k + 1],
                           leaves ? e->d_leaf : (double *)nullptr);
        EV_LAUNCHED(h->ctx, "k_full_eval_expand");
        hipLaunchKernelGGL(k_full_eval_policy, grid_of(s.size[k]), dim3(256), 0, st, (const scopa_full_state *)(e->d_state + s.off[k]), s.size[k], p, n,
                           (const FmSlot *)h->d_tab, mask, (const uint8_t *)h->d_deck, (int)which, e->d_kin, e->d_nin, e->d_prob + 3 * s.off[k]);
        EV_LAUNCHED(h->ctx, "k_full_eval_policy");
        size_t b = e->sort_bytes;
        SC_HIP(h->ctx, rocprim::radix_sort_pairs(e->d_sort, b, e->d_kin, e->d_skey + s.off[k], e->d_nin, e->d_snode + s.off[k], (size_t)s.size[k], 0u, kKeySortBits, st));
    }
    // 3: the policy against itself
    if ((rc = sweep_up(h, s, -1)) != SCOPA_OK) return rc;
    double value = 0.0;
    SC_HIP(h->ctx, hipMemcpyAsync(&e->res[2], e->d_V, 8, hipMemcpyDeviceToHost, st));
    // 4: the response of player 0, then of player 1
    for (int p = 0; p < 2; p++) {
        SC_HIP(h->ctx, hipMemcpyAsync(e->d_w, &e->one, 8, hipMemcpyHostToDevice, st));
        if ((rc = full_eval_reach_down(h->ctx, s, *e, p)) != SCOPA_OK) return rc;
        if ((rc = sweep_up(h, s, p)) != SCOPA_OK) return rc;
        SC_HIP(h->ctx, hipMemcpyAsync(&e->res[p], e->d_V, 8, hipMemcpyDeviceToHost, st));
    }
    SC_HIP(h->ctx, hipMemcpyAsync(e->n_rows, e->d_cursor, 8, hipMemcpyDeviceToHost, st));
    SC_HIP(h->ctx, hipStreamSynchronize(st));
    value = e->res[2];
    SC_REQUIRE(h->ctx, e->n_rows[0] <= s.row_cap[0] && e->n_rows[1] <= s.row_cap[1], SCOPA_ESTATE, "scopa_full_mccfr_exploitability: more response rows than nodes");
    h_out4[0] = (e->res[0] + e->res[1]) / 2.0;
    h_out4[1] = e->res[0];
    h_out4[2] = e->res[1];
    h_out4[3] = value;
    e->have_rows = true;
    return SCOPA_OK;
}

int32_t scopa_full_mccfr_response_get(scopa_full_mccfr *h, int32_t player, int64_t *n_rows, uint64_t *keys, int32_t *n_act, int32_t *action, double *q) {
    if (!h || !n_rows) return SCOPA_EINVAL;
    SC_REQUIRE(h->ctx, player == 0 || player == 1, SCOPA_EINVAL, "scopa_full_mccfr_response_get: player outside {0, 1}");
    SC_REQUIRE(h->ctx, h->eval && h->eval->have_rows, SCOPA_ESTATE, "scopa_full_mccfr_response_get: no scopa_full_mccfr_exploitability call has completed on this handle");
    FmEval *e = h->eval;
    const int64_t room = *n_rows, n = (int64_t)e->n_rows[player];
    *n_rows = n;
    if (!keys && !n_act && !action && !q) return SCOPA_OK;               // the count alone
    SC_REQUIRE(h->ctx, room >= n, SCOPA_EINVAL, "scopa_full_mccfr_response_get: *n_rows is below the rows of the response (now in *n_rows)");
    if (!n) return SCOPA_OK;
    std::vector<uint64_t> k;
    std::vector<int32_t> a;
    std::vector<double> Q;
    std::vector<uint32_t> order;
    try { k.resize((size_t)n); a.resize((size_t)n); Q.resize(3 * (size_t)n); order.resize((size_t)n); }
    catch (const std::bad_alloc &) { return fail(h->ctx, SCOPA_ENOMEM, "scopa_full_mccfr_response_get: host image of the rows"); }
    SC_HIP(h->ctx, hipSetDevice(h->ctx->device));
    SC_HIP(h->ctx, hipMemcpyAsync(k.data(), e->d_row_key[player], 8 * (size_t)n, hipMemcpyDeviceToHost, h->ctx->stream));
    SC_HIP(h->ctx, hipMemcpyAsync(a.data(), e->d_row_act[player], 4 * (size_t)n, hipMemcpyDeviceToHost, h->ctx->stream));
    SC_HIP(h->ctx, hipMemcpyAsync(Q.data(), e->d_row_q[player], 24 * (size_t)n, hipMemcpyDeviceToHost, h->ctx->stream));
    SC_HIP(h->ctx, hipStreamSynchronize(h->ctx->stream));
    std::iota(order.begin(), order.end(), 0u);
    std::sort(order.begin(), order.end(), [&k](uint32_t x, uint32_t y) { return k[x] < k[y]; });   // (keys are distinct: one row per key)
    for (int64_t i = 0; i < n; i++) {
        const uint32_t r = order[(size_t)i];
        if (keys) keys[i] = k[r];
        if (n_act) n_act[i] = key_actions(k[r]);
        if (action) action[i] = a[r];
        if (q) for (int c = 0; c < 3; c++) q[3 * i + c] = Q[3 * (size_t)r + c];
    }
    return SCOPA_OK;
}

}  // extern "C"
