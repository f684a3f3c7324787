// scopa_full_chance.hip -- external-sampling MCCFR on FullScopa over a SET of decks, the deal as a chance move: every traversal walks one deck of the
// set from a common root, and all decks add into rows shared by infoset.  The rows are kept by the deck-free two-word key of scopa_full_wide.h, so the
// learned policy is a function of what the mover sees and can be played on decks it was not trained on (scopa_full_chance_match).
//
//   walk      scopa_full_mccfr_walk.h, the ONE definition shared with scopa_full_mccfr.hip; WideDecks below is this solver's policy for it: rows by
//             (A, B), action slots in ascending card id, a deck and a root per lane, the deck index in the draw's tag word.
//   decks     a lane (cut 0) or a workgroup (cut K > 0) per (listed deck, traversal); lane / workgroup g walks deck list[g / nb], traversal b0 + g % nb.
//             The hands of the root are the deck's: deck[4 + 6 round + 3 p + i].
//   draws     Philox counter (state.step << 16 | q, traversal id, iteration, deck_index << 8 | 192 + traverser), deck_index the index in the HANDLE.
//   respond   the same walk with the non-traverser a FIXED policy read from a second store (or uniform play): k_full_chance_respond trains a responder
//             in its own store against it, and touches nothing but the responder's rows there.  Draws at tag deck_index << 8 | 144 + responder.
//             k_full_chance_harden then makes the responder's strategy rows the pure policy of its regrets, which match / pair_match / cross_play play.
//   plumbing  the apply, export and import kernels, the counters, cut, reset, tables_get / delta_get / tables_set and the match call's tail are
//             scopa_full_store_host.h's, one definition shared with scopa_full_mccfr.hip and instantiated here for FwSlot.
#include <string.h>

#include <new>
#include <vector>

#include "scopa_ctx.h"
#include "scopa_full_chance_match.h"
#include "scopa_full_mccfr_walk.h"
#include "scopa_full_store_host.h"
#include "scopa_full_wide.h"

using namespace scopa_full;
using scopa::fail;

namespace {

constexpr uint32_t kWalkTag = 192u;    // Philox counter word 3 of the traversal draws: deck_index << 8 | 192 + traverser (the response walk's: kRespondTag)
constexpr int32_t kMaxDecks = 1 << 20;
constexpr uint64_t kMaxWalks = 1ull << 30;   // listed decks x nb of one launch

struct FwArgs {
    FwSlot *tab;
    unsigned long long *cnt;
    const uint8_t *decks;              // [n_decks][40]
    const int32_t *list;               // [m] deck indices, or NULL = deck g is listed g-th
    scopa_full_state root;
    uint32_t mask, iteration, b0, nb, m, seed_lo, seed_hi;
    int traverser, cut;
    const FwSlot *opp_tab;             // the response walk's fixed opponent: its table (NULL = uniform play), mask, and which policy of it --
    uint32_t opp_mask;                 // 0 the average policy (the match's rule), 1 regret matching of its regrets.  Read by k_full_chance_respond only
    int opp_which;
};

// the walk's policy (scopa_full_mccfr_walk.h): lane or workgroup g is (listed deck, traversal), deck-major -- deck list[g / nb], traversal b0 + g % nb
template <bool kResp>
struct WideDecksT {
    using Args = FwArgs;
    static constexpr bool kRespond = kResp;
    struct Lane {
        bool exists;
        uint32_t trav_id, tag;
        const uint8_t *deck;
        __device__ __forceinline__ Lane(const FwArgs &A, uint32_t g) {
            exists = g < A.m * A.nb;                                       // (m nb <= 1 << 30)
            const uint32_t at = exists ? g / A.nb : 0u;
            const uint32_t di = A.list ? (uint32_t)A.list[at] : at;        // (checked against n_decks on the host)
            trav_id = A.b0 + (g - at * A.nb);
            tag = (di << 8) | ((kResp ? kRespondTag : kWalkTag) + (uint32_t)A.traverser);
            deck = A.decks + 40u * di;
        }
    };
    static __device__ __forceinline__ scopa_full_state root(const FwArgs &A, const uint8_t *deck) { return root_on(A.root, deck); }
    static __device__ __forceinline__ int card(const scopa_full_state &s, int p, int a) {
        int c[3];
        sorted_hand(s, p, c);
        return card_at(c, a);
    }
    static __device__ __forceinline__ int find(const FwArgs &A, const scopa_full_state &s, const uint8_t *, int p) {
        const WideKey k = wide_key(s, p);
        return fw_find(A.tab, A.mask, k.a, k.b);
    }
    static __device__ __forceinline__ int claim(const FwArgs &A, const scopa_full_state &s, const uint8_t *, int p) {
        const WideKey k = wide_key(s, p);
        return fw_claim(A.tab, A.mask, k.a, k.b, A.cnt);
    }
    // the fixed opponent's probabilities at its node of n > 1 slots (kResp): a read-only probe of ITS table, an absent pair a zero row
    static __device__ __forceinline__ void opp_probs(const FwArgs &A, const scopa_full_state &s, int p, int n, double prob[4]) {
        int slot = -1;
        if (A.opp_tab) {
            const WideKey k = wide_key(s, p);
            slot = fw_find(A.opp_tab, A.opp_mask, k.a, k.b);
        }
        if (A.opp_which == 0 || !A.opp_tab) {
            fw_average_probs(A.opp_tab, slot, n, prob);
            prob[3] = 0.0;
        } else {
            double R[4];
            fm_row(A.opp_tab[slot >= 0 ? slot : 0].regret, slot, R);
            scopa::mc_sigma(R, n, prob);
        }
    }
};
using WideDecks = WideDecksT<false>;
using RespondDecks = WideDecksT<true>;

__global__ void __launch_bounds__(256)
k_full_chance_traverse(const FwArgs A) {
    __shared__ double s_vals[216];
    full_mccfr_walk<WideDecks>(A, s_vals);
}

// the sampled response: `traverser` is the responder, whose rows in A.tab are all the launch claims and adds into
__global__ void __launch_bounds__(256)
k_full_chance_respond(const FwArgs A) {
    __shared__ double s_vals[216];
    full_mccfr_walk<RespondDecks>(A, s_vals);
}

// a lane per slot: the strategy row of every occupied slot becomes the pure policy of its regrets -- 1.0 at the FIRST maximal regret over the row's
// popcount(B) slots, 0.0 elsewhere.  Regrets are untouched.  A slot whose word B is unpublished is skipped, as the probes treat it
__global__ void __launch_bounds__(256)
k_full_chance_harden(FwSlot *__restrict__ tab, uint32_t n_slots) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_slots || tab[i].key == 0ull || tab[i].key_b == 0ull) return;
    FwSlot &t = tab[i];
    const int n = popc64(t.key_b);
    int best = 0;
    double top = t.regret[0];
#pragma unroll
    for (int a = 1; a < 3; a++) if (a < n && t.regret[a] > top) { top = t.regret[a]; best = a; }
#pragma unroll
    for (int a = 0; a < 3; a++) t.strategy[a] = a == best ? 1.0 : 0.0;
}

// One lane per episode of the seat-swapped match from the root: the agent plays the average policy of the store, the opponent uniformly
// (scopa_full_chance_match.h: the episode's one definition).
__global__ void __launch_bounds__(64)
k_full_chance_match(const FwSlot *__restrict__ tab, uint32_t mask, const uint8_t *__restrict__ decks, long long k_decks, const scopa_full_state root0, long long n,
                    uint32_t stream_id, uint32_t seed_lo, uint32_t seed_hi, long long *__restrict__ sums, int8_t *__restrict__ r2_agent) {
    full_chance_episode<false>(tab, mask, nullptr, 0u, decks, k_decks, root0, n, stream_id, seed_lo, seed_hi, sums, r2_agent);
}

// [count][m] lists of distinct deck indices in range (NULL: every deck, m ignored) -> false where one is not
bool lists_ok(const scopa_full_chance *h, const int32_t *lists, int64_t count, int64_t m) {
    if (!lists) return true;
    std::vector<int64_t> stamp((size_t)h->n_decks, -1);
    for (int64_t t = 0; t < count; t++)
        for (int64_t i = 0; i < m; i++) {
            const int32_t d = lists[t * m + i];
            if (d < 0 || d >= h->n_decks || stamp[(size_t)d] == t) return false;
            stamp[(size_t)d] = t;
        }
    return true;
}

// one traversal launch; respond: the response walk against `opp`'s store (NULL: uniform play) read by `which`
int32_t launch_traverse(scopa_full_chance *h, int traverser, uint32_t iteration, uint32_t b0, uint32_t nb, const int32_t *d_list, uint32_t m,
                        bool respond = false, const scopa_full_chance *opp = nullptr, int which = 0) {
    FwArgs A;
    A.tab = h->d_tab; A.cnt = h->d_cnt; A.decks = h->d_decks; A.list = d_list; A.root = h->root;
    A.mask = (1u << h->capacity_log2) - 1u; A.iteration = iteration; A.b0 = b0; A.nb = nb; A.m = m;
    A.seed_lo = (uint32_t)h->ctx->seed; A.seed_hi = (uint32_t)(h->ctx->seed >> 32);
    A.traverser = traverser; A.cut = h->cut < 0 ? default_cut(h) : h->cut;
    A.opp_tab = opp ? opp->d_tab : nullptr; A.opp_mask = opp ? (1u << opp->capacity_log2) - 1u : 0u; A.opp_which = which;
    const unsigned block = A.cut >= 3 ? 256u : 64u;
    const unsigned walks = m * nb;
    const unsigned grid = A.cut ? walks : (walks + 63u) / 64u;
    if (respond) hipLaunchKernelGGL(k_full_chance_respond, dim3(grid), dim3(block), 0, h->ctx->stream, A);
    else hipLaunchKernelGGL(k_full_chance_traverse, dim3(grid), dim3(block), 0, h->ctx->stream, A);
    SC_HIP(h->ctx, hipGetLastError());
    return SCOPA_OK;
}

const char *kFull = "the store is full along a probe (updates dropped): create a larger one and tables_set";

// what the response entry points ask of the fixed opponent, before any launch
int32_t opponent_ok(scopa_full_chance *h, const scopa_full_chance *opp, int32_t which, const char *who) {
    if (opp && (opp->ctx != h->ctx || opp == h)) return refuse(h, who, "h_opp is on another context or is h_resp itself");
    if (which != 0 && which != 1) return refuse(h, who, "which outside {0, 1}");
    return SCOPA_OK;
}

// the body of traverse (respond = false) and respond_traverse (respond = true: `traverser` responds to `opp`'s store read by `which`)
int32_t traverse_call(scopa_full_chance *h, const char *who, int32_t traverser, uint32_t iteration, uint32_t b0, uint32_t nb, const int32_t *h_list, int32_t m,
                      bool respond, const scopa_full_chance *opp, int which) {
    if (traverser != 0 && traverser != 1) return refuse(h, who, "traverser outside {0, 1}");
    if (!(nb <= (1u << 24) && (uint64_t)b0 + nb <= (1ull << 32))) return refuse(h, who, "nb above 1 << 24 or b0 + nb overflows");
    if (!h_list) m = h->n_decks;
    if (!(m >= 0 && m <= h->n_decks && lists_ok(h, h_list, 1, m))) return refuse(h, who, "a listed deck out of range or listed twice");
    if ((uint64_t)m * nb > kMaxWalks) return refuse(h, who, "listed decks x nb above 1 << 30");
    if (!nb || !m) return SCOPA_OK;
    SC_HIP(h->ctx, hipSetDevice(h->ctx->device));
    int32_t *d_list = nullptr;
    hipError_t e;
    if (h_list) {
        if ((e = hipMalloc((void **)&d_list, 4 * (size_t)m)) != hipSuccess) return refuse(h, who, "the deck list", SCOPA_ENOMEM, e);
        if ((e = hipMemcpyAsync(d_list, h_list, 4 * (size_t)m, hipMemcpyHostToDevice, h->ctx->stream)) != hipSuccess) {
            (void)hipFree(d_list);
            return fail(h->ctx, SCOPA_EHIP, "hipMemcpyAsync(H2D)", e);
        }
    }
    int32_t rc = launch_traverse(h, traverser, iteration, b0, nb, d_list, (uint32_t)m, respond, opp, which);
    const int32_t rc2 = check_dropped(h, kFull);                          // synchronises: the list may go
    if (d_list) (void)hipFree(d_list);
    return rc != SCOPA_OK ? rc : rc2;
}

// the body of iterate and respond_iterate: per iteration traverser 0, apply, traverser 1, apply; the lists uploaded once, no host synchronisation
// between iterations, one check_dropped at the end
int32_t iterate_call(scopa_full_chance *h, const char *who, uint32_t batch, uint32_t n_iters, const int32_t *h_lists, int32_t m, bool respond,
                     const scopa_full_chance *opp, int which) {
    if (!(batch >= 1 && batch <= (1u << 24) && n_iters <= (1u << 20))) return refuse(h, who, "batch outside [1, 1 << 24] or n_iters above 1 << 20");
    if (!h_lists) m = h->n_decks;
    if (!(m >= 0 && m <= h->n_decks && lists_ok(h, h_lists, n_iters, m))) return refuse(h, who, "a listed deck out of range or twice in one iteration's list");
    if ((uint64_t)m * batch > kMaxWalks) return refuse(h, who, "listed decks x batch above 1 << 30");
    if (!n_iters) return SCOPA_OK;
    SC_HIP(h->ctx, hipSetDevice(h->ctx->device));
    int32_t *d_lists = nullptr;
    hipError_t e;
    const size_t bytes = 4 * (size_t)n_iters * (size_t)m;
    if (h_lists && bytes) {                                               // uploaded once per call
        if ((e = hipMalloc((void **)&d_lists, bytes)) != hipSuccess) return refuse(h, who, "the deck lists", SCOPA_ENOMEM, e);
        if ((e = hipMemcpyAsync(d_lists, h_lists, bytes, hipMemcpyHostToDevice, h->ctx->stream)) != hipSuccess) {
            (void)hipFree(d_lists);
            return fail(h->ctx, SCOPA_EHIP, "hipMemcpyAsync(H2D)", e);
        }
    }
    int32_t rc = SCOPA_OK;
    for (uint32_t t = 0; t < n_iters && rc == SCOPA_OK; t++)
        for (int trav = 0; trav < 2 && rc == SCOPA_OK; trav++) {
            if (m) rc = launch_traverse(h, trav, h->iteration, 0u, batch, d_lists ? d_lists + (size_t)t * m : nullptr, (uint32_t)m, respond, opp, which);
            if (rc == SCOPA_OK) rc = launch_apply(h);
        }
    const int32_t rc2 = check_dropped(h, kFull);                          // synchronises: the lists may go
    if (d_lists) (void)hipFree(d_lists);
    return rc != SCOPA_OK ? rc : rc2;
}

}  // namespace

extern "C" {

int32_t scopa_full_infoset_key_wide(const scopa_full_state *s, int32_t player, uint64_t key2[2]) {
    if (!s || !key2 || player < 0 || player > 1 || s->round > 5 || s->nh[0] > 3 || s->nh[1] > 3 || s->nt > kMaxTable) return SCOPA_EINVAL;
    const WideKey k = wide_key(*s, player);
    key2[0] = k.a;
    key2[1] = k.b;
    return SCOPA_OK;
}

int32_t scopa_full_chance_create(scopa_ctx *ctx, const uint8_t *decks, int32_t n_decks, const scopa_full_state *root_state, int32_t capacity_log2, scopa_full_chance **out) {
    if (out) *out = nullptr;
    if (!ctx || !decks || !out) return SCOPA_EINVAL;
    SC_REQUIRE(ctx, n_decks >= 1 && n_decks <= kMaxDecks, SCOPA_EINVAL, "scopa_full_chance_create: n_decks outside [1, 1 << 20]");
    SC_REQUIRE(ctx, capacity_log2 >= 4 && capacity_log2 <= 28, SCOPA_EINVAL, "scopa_full_chance_create: capacity_log2 outside [4, 28]");
    for (int i = 0; i < 40; i++) SC_REQUIRE(ctx, decks[i] <= 39, SCOPA_EINVAL, "scopa_full_chance_create: a deck is not a permutation of 0..39");
    scopa_full_state root;
    if (root_state) root = *root_state; else state_init(root, decks, 0u);
    SC_REQUIRE(ctx, root_ok(root), SCOPA_EINVAL, "scopa_full_chance_create: the root must be a non-terminal state at a round boundary (step % 6 == 0)");
    for (int32_t d = 0; d < n_decks; d++)
        SC_REQUIRE(ctx, deck_fits(decks + 40 * (size_t)d, root), SCOPA_EINVAL,
                   "scopa_full_chance_create: a deck is no permutation, does not hold exactly the root's unseen cards from position 4 + 6 round on, or (round 0) does not start with the root's table");
    root.game = 0u;
    scopa_full_chance *h = new (std::nothrow) scopa_full_chance;
    if (!h) return SCOPA_ENOMEM;
    const size_t deck_bytes = 40 * (size_t)n_decks;
    h->decks = new (std::nothrow) uint8_t[deck_bytes];
    if (!h->decks) { delete h; return SCOPA_ENOMEM; }
    memcpy(h->decks, decks, deck_bytes);
    h->ctx = ctx; h->root = root; h->capacity_log2 = capacity_log2; h->n_decks = n_decks;
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_tab, sizeof(FwSlot) << capacity_log2);
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_cnt, 2 * kCntWords * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_decks, deck_bytes + 24);
    int32_t rc = SCOPA_OK;
    if (e != hipSuccess) rc = fail(ctx, e == hipErrorOutOfMemory ? SCOPA_ENOMEM : SCOPA_EHIP, "scopa_full_chance_create: hipMalloc", e);
    if (rc == SCOPA_OK && ((e = hipMemsetAsync(h->d_tab, 0, sizeof(FwSlot) << capacity_log2, ctx->stream)) != hipSuccess ||
                           (e = hipMemsetAsync(h->d_cnt, 0, 2 * kCntWords * 8, ctx->stream)) != hipSuccess ||
                           (e = hipMemcpyAsync(h->d_decks, h->decks, deck_bytes, hipMemcpyHostToDevice, ctx->stream)) != hipSuccess ||
                           (e = hipStreamSynchronize(ctx->stream)) != hipSuccess))
        rc = fail(ctx, SCOPA_EHIP, "scopa_full_chance_create: initialising the store", e);
    if (rc != SCOPA_OK) {
        if (h->d_tab) (void)hipFree(h->d_tab);
        if (h->d_cnt) (void)hipFree(h->d_cnt);
        if (h->d_decks) (void)hipFree(h->d_decks);
        delete[] h->decks;
        delete h;
        return rc;
    }
    *out = h;
    return SCOPA_OK;
}

int32_t scopa_full_chance_destroy(scopa_full_chance *h) {
    if (!h) return SCOPA_EINVAL;
    (void)hipStreamSynchronize(h->ctx->stream);
    (void)hipFree(h->d_tab);
    (void)hipFree(h->d_cnt);
    (void)hipFree(h->d_decks);
    chance_eval_free(h->eval);
    chance_cfr_free(h->cfr);
    chance_xplay_free(h->xplay);
    chance_sdcfr_free(h->sd);
    delete[] h->decks;
    delete h;
    return SCOPA_OK;
}

int32_t scopa_full_chance_root(const scopa_full_chance *h, scopa_full_state *root, uint8_t *decks, int32_t *n_decks, int32_t *capacity_log2) {
    if (!h) return SCOPA_EINVAL;
    if (root) *root = h->root;
    if (decks) memcpy(decks, h->decks, 40 * (size_t)h->n_decks);
    if (n_decks) *n_decks = h->n_decks;
    if (capacity_log2) *capacity_log2 = h->capacity_log2;
    return SCOPA_OK;
}

int32_t scopa_full_chance_cut(scopa_full_chance *h, int32_t cut) { return set_cut(h, "scopa_full_chance_cut", cut); }

int32_t scopa_full_chance_reset(scopa_full_chance *h) {
    if (!h) return SCOPA_EINVAL;
    SC_HIP(h->ctx, hipSetDevice(h->ctx->device));
    return clear_store(h);
}

int32_t scopa_full_chance_traverse(scopa_full_chance *h, int32_t traverser, uint32_t iteration, uint32_t b0, uint32_t nb, const int32_t *h_list, int32_t m) {
    if (!h) return SCOPA_EINVAL;
    return traverse_call(h, "scopa_full_chance_traverse", traverser, iteration, b0, nb, h_list, m, false, nullptr, 0);
}

int32_t scopa_full_chance_apply(scopa_full_chance *h) {
    if (!h) return SCOPA_EINVAL;
    SC_HIP(h->ctx, hipSetDevice(h->ctx->device));
    return launch_apply(h);
}

int32_t scopa_full_chance_iterate(scopa_full_chance *h, uint32_t batch, uint32_t n_iters, const int32_t *h_lists, int32_t m) {
    if (!h) return SCOPA_EINVAL;
    return iterate_call(h, "scopa_full_chance_iterate", batch, n_iters, h_lists, m, false, nullptr, 0);
}

int32_t scopa_full_chance_respond_traverse(scopa_full_chance *h_resp, scopa_full_chance *h_opp, int32_t which, int32_t responder, uint32_t iteration, uint32_t b0,
                                           uint32_t nb, const int32_t *h_list, int32_t m) {
    if (!h_resp) return SCOPA_EINVAL;
    const int32_t rc = opponent_ok(h_resp, h_opp, which, "scopa_full_chance_respond_traverse");
    if (rc != SCOPA_OK) return rc;
    return traverse_call(h_resp, "scopa_full_chance_respond_traverse", responder, iteration, b0, nb, h_list, m, true, h_opp, which);
}

int32_t scopa_full_chance_respond_iterate(scopa_full_chance *h_resp, scopa_full_chance *h_opp, int32_t which, uint32_t batch, uint32_t n_iters,
                                          const int32_t *h_lists, int32_t m) {
    if (!h_resp) return SCOPA_EINVAL;
    const int32_t rc = opponent_ok(h_resp, h_opp, which, "scopa_full_chance_respond_iterate");
    if (rc != SCOPA_OK) return rc;
    return iterate_call(h_resp, "scopa_full_chance_respond_iterate", batch, n_iters, h_lists, m, true, h_opp, which);
}

int32_t scopa_full_chance_harden(scopa_full_chance *h) {
    if (!h) return SCOPA_EINVAL;
    SC_HIP(h->ctx, hipSetDevice(h->ctx->device));
    const uint32_t n = 1u << h->capacity_log2;
    hipLaunchKernelGGL(k_full_chance_harden, dim3((n + 255u) / 256u), dim3(256), 0, h->ctx->stream, h->d_tab, n);
    SC_HIP(h->ctx, hipGetLastError());
    return SCOPA_OK;
}

int32_t scopa_full_chance_counters(scopa_full_chance *h, uint64_t *choice_visits, uint64_t *terminal_visits, uint64_t *rows, uint64_t *dropped, uint32_t *iterations) {
    return counters_out(h, choice_visits, terminal_visits, rows, dropped, iterations);
}

int32_t scopa_full_chance_tables_get(scopa_full_chance *h, int64_t *n_rows, uint64_t *keys2, int32_t *n_act, double *regret, double *strategy) {
    return rows_out(h, "scopa_full_chance_tables_get", n_rows, keys2, n_act, regret, strategy, nullptr, false);
}

int32_t scopa_full_chance_delta_get(scopa_full_chance *h, int64_t *n_rows, uint64_t *keys2, double *d_regret, double *d_strategy, uint32_t *counts) {
    return rows_out(h, "scopa_full_chance_delta_get", n_rows, keys2, nullptr, d_regret, d_strategy, counts, true);
}

int32_t scopa_full_chance_tables_set(scopa_full_chance *h, int64_t n_rows, const uint64_t *keys2, const int32_t *n_act, const double *regret, const double *strategy) {
    return tables_in(h, "scopa_full_chance_tables_set", n_rows, keys2, n_act, regret, strategy);
}

int32_t scopa_full_chance_match(scopa_full_chance *h, int64_t n_episodes, uint32_t stream_id, const uint8_t *h_decks, int32_t k, int64_t h_sums[6], int8_t *h_r2_agent) {
    if (!h) return SCOPA_EINVAL;
    SC_REQUIRE(h->ctx, n_episodes >= 0 && n_episodes <= (1ll << 36) && h_sums && stream_id < (1u << 24), SCOPA_EINVAL,      // (one launch: 2^30 workgroups of 64)
               "scopa_full_chance_match: n_episodes outside [0, 1 << 36], stream_id at or above 1 << 24, or h_sums NULL");
    if (!h_decks) k = h->n_decks;
    SC_REQUIRE(h->ctx, k >= 1 && k <= kMaxDecks, SCOPA_EINVAL, "scopa_full_chance_match: k outside [1, 1 << 20]");
    if (h_decks)
        for (int32_t d = 0; d < k; d++)
            SC_REQUIRE(h->ctx, deck_fits(h_decks + 40 * (size_t)d, h->root), SCOPA_EINVAL, "scopa_full_chance_match: a deck does not pass create's check against the handle's root");
    for (int i = 0; i < 6; i++) h_sums[i] = 0;
    if (!n_episodes) return SCOPA_OK;
    SC_REQUIRE(h->ctx, !h_r2_agent || n_episodes <= (1ll << 31), SCOPA_EINVAL, "scopa_full_chance_match: per-episode output asked for more than 1 << 31 episodes");
    SC_HIP(h->ctx, hipSetDevice(h->ctx->device));
    return run_match(h, "scopa_full_chance_match", "k_full_chance_match", n_episodes, h_decks, k, h_sums, h_r2_agent, [&](const uint8_t *d_held, long long *d_sums, int8_t *d_r2) {
        hipLaunchKernelGGL(k_full_chance_match, dim3((unsigned)((n_episodes + 63) / 64)), dim3(64), 0, h->ctx->stream, (const FwSlot *)h->d_tab, (1u << h->capacity_log2) - 1u,
                           (const uint8_t *)(d_held ? d_held : h->d_decks), (long long)k, h->root, (long long)n_episodes, stream_id, (uint32_t)h->ctx->seed,
                           (uint32_t)(h->ctx->seed >> 32), d_sums, d_r2);
    });
}

}  // extern "C"
