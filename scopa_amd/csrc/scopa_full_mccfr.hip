// scopa_full_mccfr.hip -- external-sampling MCCFR on FullScopa (40 cards) over a device hash table of infosets.
//
// One deal of the full game has 36^6 histories, so the tables cannot be dense arrays over a pre-built index as in every other solver of the library:
// rows live in an open-addressing store keyed by scopa_full::infoset_key and are claimed as the traversals meet them.
//
//   store     2^capacity_log2 slots of 128 bytes (one line each): key | regret[3] | strategy[3] | d_regret[3] | d_strategy[3] | count.  A slot is
//             claimed with ONE 64-bit compare-and-swap on its key word (0 = empty); its other words are zero from reset.  Linear probing from a
//             splitmix hash of the key, at most kMaxProbe slots: a probe that finds neither the key nor an empty slot gives up (`dropped` += 1, the
//             update is skipped, the host call reports SCOPA_ENOMEM).  Nothing is ever deleted between resets, so a read-only probe that meets an
//             empty slot knows the key is absent.  No loop waits for another lane, wavefront or workgroup.
//             The probe sequence: home = fm_hash(key) & (2^capacity_log2 - 1), then the next slot and the next, wrapping at the end of the table,
//             kMaxProbe = 64 slots in all (a smaller store is lapped).  fm_find and fm_claim (scopa_full_store.h, side by side) are two copies of that
//             loop and must agree: with cut > 0 the prefix lanes find what lane 0 claims.  tests/full_mccfr_ref.py restates the sequence (fm_hash,
//             home_slot, MAX_PROBE) to build probe chains out of filler keys, so a change of the hash or of the limit changes both places;
//             tests/test_gpu_full_store.py runs the chains.
//   plumbing  the apply, export and import kernels, the counters, cut, reset, tables_get / delta_get / tables_set and the match call's tail are
//             scopa_full_store_host.h's, one definition shared with scopa_full_chance.hip and instantiated here for FmSlot.  What is left in this
//             file is the one-deck solver's own: create and destroy, the walk's policy and launch, the match kernel.
//   traverse  the walk itself is scopa_full_mccfr_walk.h, shared with scopa_full_chance.hip (a set of decks, two-word keys); OneDeck below is this solver's
//             policy for it: one-word keys, action slots in hand order, one deck and one root for the whole launch.
#include <string.h>

#include <new>

#include "scopa_ctx.h"
#include "scopa_full_key.h"
#include "scopa_full_mccfr_walk.h"
#include "scopa_full_store_host.h"
#include "scopa_mccfr_sigma.h"
#include "scopa_philox.h"

using namespace scopa_full;
using scopa::fail;

namespace {

constexpr uint32_t kWalkTag = 160u;    // Philox counter word 3 of the traversal draws: 160 + traverser
constexpr uint32_t kMatchTag = 176u;   // ... of the match draws

// (FmSlot, kMaxProbe, the counter words, fm_hash, fm_find and fm_claim are in scopa_full_store.h)
struct FmArgs {
    FmSlot *tab;
    unsigned long long *cnt;
    const uint8_t *deck;
    scopa_full_state root;
    uint32_t mask, iteration, b0, nb, seed_lo, seed_hi;
    int traverser, cut;
};

// the walk's policy (scopa_full_mccfr_walk.h): lane or workgroup g is traversal b0 + g of the handle's one deck
struct OneDeck {
    using Args = FmArgs;
    static constexpr bool kRespond = false;
    struct Lane {
        bool exists;
        uint32_t trav_id, tag;
        const uint8_t *deck;
        __device__ __forceinline__ Lane(const FmArgs &A, uint32_t g) : exists(g < A.nb), trav_id(A.b0 + g), tag(kWalkTag + (uint32_t)A.traverser), deck(A.deck) {}
    };
    static __device__ __forceinline__ scopa_full_state root(const FmArgs &A, const uint8_t *) { return A.root; }
    static __device__ __forceinline__ int card(const scopa_full_state &s, int p, int a) { return hand_get(s, p, a); }
    static __device__ __forceinline__ int find(const FmArgs &A, const scopa_full_state &s, const uint8_t *deck, int p) { return fm_find(A.tab, A.mask, infoset_key(s, deck, p)); }
    static __device__ __forceinline__ int claim(const FmArgs &A, const scopa_full_state &s, const uint8_t *deck, int p) { return fm_claim(A.tab, A.mask, infoset_key(s, deck, p), A.cnt); }
};

__global__ void __launch_bounds__(256)
k_full_mccfr_traverse(const FmArgs A) {
    __shared__ double s_vals[216];
    full_mccfr_walk<OneDeck>(A, s_vals);
}

// One lane per episode of the seat-swapped match from the root: the agent plays the average policy of the store, the opponent uniformly.
__global__ void __launch_bounds__(64)
k_full_mccfr_match(const FmSlot *__restrict__ tab, uint32_t mask, const uint8_t *__restrict__ deck, const scopa_full_state root, long long n, uint32_t stream_id,
                   uint32_t seed_lo, uint32_t seed_hi, long long *__restrict__ sums, int8_t *__restrict__ r2_agent) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int seat = 2 * i < n ? 0 : 1;
    scopa_full_state s = root;
    while (!s.terminal) {
        const int p = s.step & 1, nl = nh_of(s, p);
        int a = 0;
        if (nl > 1) {
            double prob[3];
#pragma unroll
            for (int k = 0; k < 3; k++) prob[k] = 1.0 / (double)nl;
            if (p == seat) {
                const int slot = fm_find(tab, mask, infoset_key(s, deck, p));
                if (slot >= 0) {
                    double S[3], total = 0.0;
#pragma unroll
                    for (int k = 0; k < 3; k++) { S[k] = tab[slot].strategy[k]; if (k < nl) total += S[k]; }
                    if (total > 1e-12) {
#pragma unroll
                        for (int k = 0; k < 3; k++) prob[k] = S[k] / total;
                    }
                }
            }
            const scopa::philox_out x = scopa::philox4x32_10((uint32_t)i, (uint32_t)((unsigned long long)i >> 32), (stream_id << 8) | (uint32_t)s.step, kMatchTag, seed_lo, seed_hi);
            a = fm_pick(prob, nl, scopa::u53(x.x0, x.x1));
        }
        step(s, deck, hand_get(s, p, a));
    }
    const long long r2 = seat ? -(long long)s.r2_p0 : (long long)s.r2_p0;
    if (r2_agent) r2_agent[i] = (int8_t)r2;
    atomicAdd((unsigned long long *)sums + seat, (unsigned long long)r2);                      // (two's complement: the sums are signed)
    atomicAdd((unsigned long long *)sums + 2 + seat, (unsigned long long)(r2 * r2));
    atomicAdd((unsigned long long *)sums + 4, (unsigned long long)(seat ? s.scopas[1] : s.scopas[0]));
    atomicAdd((unsigned long long *)sums + 5, (unsigned long long)(seat ? s.scopas[0] : s.scopas[1]));
}

bool deck_ok(const uint8_t *d) {
    uint64_t seen = 0;
    for (int i = 0; i < 40; i++) { if (d[i] > 39) return false; seen |= 1ull << d[i]; }
    return seen == ((1ull << 40) - 1);
}

int32_t launch_traverse(scopa_full_mccfr *h, int traverser, uint32_t iteration, uint32_t b0, uint32_t nb) {
    FmArgs A;
    A.tab = h->d_tab; A.cnt = h->d_cnt; A.deck = h->d_deck; A.root = h->root;
    A.mask = (1u << h->capacity_log2) - 1u; A.iteration = iteration; A.b0 = b0; A.nb = nb;
    A.seed_lo = (uint32_t)h->ctx->seed; A.seed_hi = (uint32_t)(h->ctx->seed >> 32);
    A.traverser = traverser; A.cut = h->cut < 0 ? default_cut(h) : h->cut;
    const unsigned block = A.cut >= 3 ? 256u : 64u;
    const unsigned grid = A.cut ? nb : (nb + 63u) / 64u;
    hipLaunchKernelGGL(k_full_mccfr_traverse, dim3(grid), dim3(block), 0, h->ctx->stream, A);
    SC_HIP(h->ctx, hipGetLastError());
    return SCOPA_OK;
}

}  // namespace

extern "C" {

int32_t scopa_full_infoset_key(const scopa_full_state *s, const uint8_t deck40[40], int32_t player, uint64_t *key) {
    if (!s || !deck40 || !key || player < 0 || player > 1 || s->round > 5 || s->nh[0] > 3 || s->nh[1] > 3 || s->nt > kMaxTable || !deck_ok(deck40)) return SCOPA_EINVAL;
    *key = infoset_key(*s, deck40, player);
    return SCOPA_OK;
}

int32_t scopa_full_mccfr_create(scopa_ctx *ctx, const uint8_t deck40[40], const scopa_full_state *root_state, int32_t capacity_log2, scopa_full_mccfr **out) {
    if (out) *out = nullptr;
    if (!ctx || !deck40 || !out) return SCOPA_EINVAL;
    SC_REQUIRE(ctx, deck_ok(deck40), SCOPA_EINVAL, "scopa_full_mccfr_create: the deck is not a permutation of 0..39");
    SC_REQUIRE(ctx, capacity_log2 >= 4 && capacity_log2 <= 28, SCOPA_EINVAL, "scopa_full_mccfr_create: capacity_log2 outside [4, 28]");
    scopa_full_state root;
    if (root_state) root = *root_state; else state_init(root, deck40, 0u);
    // a round boundary of a game in play: everything else the walk relies on follows from it (three cards each, 6 - round rounds to go)
    const int bad = root_check(root, deck40);
    SC_REQUIRE(ctx, bad != 1, SCOPA_EINVAL, "scopa_full_mccfr_create: the root must be a non-terminal state at a round boundary (step % 6 == 0)");
    SC_REQUIRE(ctx, bad != 2, SCOPA_EINVAL, "scopa_full_mccfr_create: the root's hands are not this deck's deal of its round");
    root.game = 0u;
    scopa_full_mccfr *h = new (std::nothrow) scopa_full_mccfr;
    if (!h) return SCOPA_ENOMEM;
    h->ctx = ctx; h->root = root; h->capacity_log2 = capacity_log2;
    memcpy(h->deck, deck40, 40);
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_tab, sizeof(FmSlot) << capacity_log2);
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_cnt, 2 * kCntWords * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_deck, 64);
    int32_t rc = SCOPA_OK;
    if (e != hipSuccess) rc = fail(ctx, e == hipErrorOutOfMemory ? SCOPA_ENOMEM : SCOPA_EHIP, "scopa_full_mccfr_create: hipMalloc", e);
    if (rc == SCOPA_OK && ((e = hipMemsetAsync(h->d_tab, 0, sizeof(FmSlot) << capacity_log2, ctx->stream)) != hipSuccess ||
                           (e = hipMemsetAsync(h->d_cnt, 0, 2 * kCntWords * 8, ctx->stream)) != hipSuccess ||
                           (e = hipMemcpyAsync(h->d_deck, h->deck, 40, hipMemcpyHostToDevice, ctx->stream)) != hipSuccess ||
                           (e = hipStreamSynchronize(ctx->stream)) != hipSuccess))
        rc = fail(ctx, SCOPA_EHIP, "scopa_full_mccfr_create: initialising the store", e);
    if (rc != SCOPA_OK) {
        if (h->d_tab) (void)hipFree(h->d_tab);
        if (h->d_cnt) (void)hipFree(h->d_cnt);
        if (h->d_deck) (void)hipFree(h->d_deck);
        delete h;
        return rc;
    }
    *out = h;
    return SCOPA_OK;
}

int32_t scopa_full_mccfr_destroy(scopa_full_mccfr *h) {
    if (!h) return SCOPA_EINVAL;
    (void)hipStreamSynchronize(h->ctx->stream);
    (void)hipFree(h->d_tab);
    (void)hipFree(h->d_cnt);
    (void)hipFree(h->d_deck);
    if (h->eval) eval_free(h->eval);
    delete h;
    return SCOPA_OK;
}

int32_t scopa_full_mccfr_root(const scopa_full_mccfr *h, scopa_full_state *root, uint8_t deck40[40], int32_t *capacity_log2) {
    if (!h) return SCOPA_EINVAL;
    if (root) *root = h->root;
    if (deck40) memcpy(deck40, h->deck, 40);
    if (capacity_log2) *capacity_log2 = h->capacity_log2;
    return SCOPA_OK;
}

int32_t scopa_full_mccfr_cut(scopa_full_mccfr *h, int32_t cut) { return set_cut(h, "scopa_full_mccfr_cut", cut); }

int32_t scopa_full_mccfr_reset(scopa_full_mccfr *h) {
    if (!h) return SCOPA_EINVAL;
    SC_HIP(h->ctx, hipSetDevice(h->ctx->device));
    return clear_store(h);
}

int32_t scopa_full_mccfr_traverse(scopa_full_mccfr *h, int32_t traverser, uint32_t iteration, uint32_t b0, uint32_t nb) {
    if (!h) return SCOPA_EINVAL;
    SC_REQUIRE(h->ctx, traverser == 0 || traverser == 1, SCOPA_EINVAL, "scopa_full_mccfr_traverse: traverser outside {0, 1}");
    SC_REQUIRE(h->ctx, nb <= (1u << 24) && (uint64_t)b0 + nb <= (1ull << 32), SCOPA_EINVAL, "scopa_full_mccfr_traverse: nb above 1 << 24 or b0 + nb overflows");
    if (!nb) return SCOPA_OK;
    SC_HIP(h->ctx, hipSetDevice(h->ctx->device));
    const int32_t rc = launch_traverse(h, traverser, iteration, b0, nb);
    if (rc != SCOPA_OK) return rc;
    return check_dropped(h, "scopa_full_mccfr_traverse: the store is full along a probe (updates dropped): create a larger one and tables_set");
}

int32_t scopa_full_mccfr_apply(scopa_full_mccfr *h) {
    if (!h) return SCOPA_EINVAL;
    SC_HIP(h->ctx, hipSetDevice(h->ctx->device));
    return launch_apply(h);
}

int32_t scopa_full_mccfr_iterate(scopa_full_mccfr *h, uint32_t batch, uint32_t n_iters) {
    if (!h) return SCOPA_EINVAL;
    SC_REQUIRE(h->ctx, batch >= 1 && batch <= (1u << 24) && n_iters <= (1u << 20), SCOPA_EINVAL, "scopa_full_mccfr_iterate: batch outside [1, 1 << 24] or n_iters above 1 << 20");
    if (!n_iters) return SCOPA_OK;
    SC_HIP(h->ctx, hipSetDevice(h->ctx->device));
    for (uint32_t t = 0; t < n_iters; t++)
        for (int trav = 0; trav < 2; trav++) {
            int32_t rc = launch_traverse(h, trav, h->iteration, 0u, batch);
            if (rc == SCOPA_OK) rc = launch_apply(h);
            if (rc != SCOPA_OK) return rc;
        }
    return check_dropped(h, "scopa_full_mccfr_iterate: the store is full along a probe (updates dropped): create a larger one and tables_set");
}

int32_t scopa_full_mccfr_counters(scopa_full_mccfr *h, uint64_t *choice_visits, uint64_t *terminal_visits, uint64_t *rows, uint64_t *dropped, uint32_t *iterations) {
    return counters_out(h, choice_visits, terminal_visits, rows, dropped, iterations);
}

int32_t scopa_full_mccfr_tables_get(scopa_full_mccfr *h, int64_t *n_rows, uint64_t *keys, int32_t *n_act, double *regret, double *strategy) {
    return rows_out(h, "scopa_full_mccfr_tables_get", n_rows, keys, n_act, regret, strategy, nullptr, false);
}

int32_t scopa_full_mccfr_delta_get(scopa_full_mccfr *h, int64_t *n_rows, uint64_t *keys, double *d_regret, double *d_strategy, uint32_t *counts) {
    return rows_out(h, "scopa_full_mccfr_delta_get", n_rows, keys, nullptr, d_regret, d_strategy, counts, true);
}

int32_t scopa_full_mccfr_tables_set(scopa_full_mccfr *h, int64_t n_rows, const uint64_t *keys, const int32_t *n_act, const double *regret, const double *strategy) {
    return tables_in(h, "scopa_full_mccfr_tables_set", n_rows, keys, n_act, regret, strategy);
}

int32_t scopa_full_mccfr_match(scopa_full_mccfr *h, int64_t n_episodes, uint32_t stream_id, int64_t h_sums[6], int8_t *h_r2_agent) {
    if (!h) return SCOPA_EINVAL;
    SC_REQUIRE(h->ctx, n_episodes >= 0 && n_episodes <= (1ll << 40) && h_sums && stream_id < (1u << 24), SCOPA_EINVAL,
               "scopa_full_mccfr_match: n_episodes outside [0, 1 << 40], stream_id at or above 1 << 24, or h_sums NULL");
    for (int k = 0; k < 6; k++) h_sums[k] = 0;
    if (!n_episodes) return SCOPA_OK;
    SC_REQUIRE(h->ctx, !h_r2_agent || n_episodes <= (1ll << 31), SCOPA_EINVAL, "scopa_full_mccfr_match: per-episode output asked for more than 1 << 31 episodes");
    SC_HIP(h->ctx, hipSetDevice(h->ctx->device));
    return run_match(h, "scopa_full_mccfr_match", "k_full_mccfr_match", n_episodes, nullptr, 0, h_sums, h_r2_agent, [&](const uint8_t *, long long *d_sums, int8_t *d_r2) {
        hipLaunchKernelGGL(k_full_mccfr_match, dim3((unsigned)((n_episodes + 63) / 64)), dim3(64), 0, h->ctx->stream, (const FmSlot *)h->d_tab, (1u << h->capacity_log2) - 1u,
                           (const uint8_t *)h->d_deck, h->root, (long long)n_episodes, stream_id, (uint32_t)h->ctx->seed, (uint32_t)(h->ctx->seed >> 32), d_sums, d_r2);
    });
}

}  // extern "C"
