// scopa_full_wide.h -- the deck-free, two-word infoset key of FullScopa and the store that keeps rows by it: what scopa_full_chance.hip (the
// sampling solver over a SET of decks) and scopa_full_chance_eval.hip (the exact sweeps across the decks) are built on.  scopa_full_key.h names a
// hand by positions in one deck, so its rows mean nothing on another deck; here the hand is named by card and the key no longer fits one word.
// Also here, for both files: root_on (a root with a deck's deal in hand), root_ok and deck_fits (what create asks of a root and of a deck below it).
// The store's kernels and host plumbing are scopa_full_store_host.h's, shared with the one-word store; SlotKey<FwSlot> below is what they ask of this one,
// and the handle is scopa_full_store.h's StoreHandle<FwSlot> with the decks and the scratch of the exact sweeps.
//
//   key       A = infoset_key with the hand field empty: bit 63 set | player (bit 62) | round (bits 59-61) | bits 56-58 zero | table, a 40-bit card
//             mask (bits 16-55) | cards captured by `player` (bits 10-15) | scopas of player 0 (bits 5-9) | scopas of player 1 (bits 0-4).
//             B = the player's hand as a 40-bit card mask; never 0 at a decision node.  Neither word reads the deck.
//             Over the decision nodes of ANY decks, two (state, mover) pairs have equal (A, B) exactly when scopa_full_state_infoset_string gives
//             equal strings: the string is player, round, hand by card, table by card, the two capture counts and the scopas, and the opponent's
//             capture count follows from the cards dealt so far (4 + 6 (round + 1) = piles + table + hands) as in scopa_full_key.h.
//             Action slot a of a key is its a-th held card in ASCENDING CARD ID -- the a-th set bit of B -- not in hand order: hand order is deal
//             order and differs between decks that share the infoset.  The action count is popcount(B).
//   slot      128 bytes, one line, FmSlot's layout with the second key word in what is padding there:
//             A | regret[3] | strategy[3] | d_regret[3] | d_strategy[3] | count | pad | B | pad.  Word A = 0: empty.  Word B = 0: unpublished.
//   probe     home = fm_hash(A ^ B * 0x9E3779B97F4A7C15) & (2^capacity_log2 - 1), then the next slot and the next, wrapping, kMaxProbe = 64 slots in all.
//   claim     at an empty slot ONE compare-and-swap of word A from 0; whoever then sees word A equal to its own (having won, lost to the same A, or
//             found it) reads word B and, where that is 0, does ONE compare-and-swap of word B from 0.  The lane whose swap publishes B counts the
//             row.  Result 0 or the own B: the slot is ours; any other value: another hand of the same A owns the slot for good, go on.  No loop
//             waits: a lost race is resolved by the value the swap returned.  ("Store with two-word keys", argues the invariants.)
//   find      read-only.  Stops at an empty slot (absent) and at a slot with word A equal and word B still 0: such a slot was claimed in this very
//             launch, its regrets are zero from reset and regrets are frozen per launch, so "absent, zero row" is what its owner reads too.
#pragma once
#include "scopa_full_store.h"

namespace scopa_full {

constexpr uint64_t kWideMul = 0x9E3779B97F4A7C15ull;
constexpr uint64_t kCardMask = (1ull << 40) - 1ull;

struct WideKey { uint64_t a, b; };

SCF_HD WideKey wide_key(const scopa_full_state &s, int player) {
    const int n = nh_of(s, player);
    uint64_t hand = 0ull;
#pragma unroll
    for (int j = 0; j < 3; j++) if (j < n) hand |= 1ull << hand_get(s, player, j);
    uint64_t table = 0ull;
SCF_UNROLL
    for (int i = 0; i < kMaxTable; i++) {
        if (!any_lane(i < s.nt)) break;
        if (i < s.nt) table |= 1ull << tab_get(s, i);
    }
    const uint64_t own = (uint64_t)popc64(player ? s.cap[1] : s.cap[0]);
    WideKey k;
    k.a = (1ull << 63) | ((uint64_t)player << 62) | ((uint64_t)(s.round & 7) << 59) | (table << kKeyTableShift) | (own << 10) |
          ((uint64_t)(s.scopas[0] & 31) << 5) | (uint64_t)(s.scopas[1] & 31);
    k.b = hand;
    return k;
}

// the mover's cards in ascending card id = the action slots of its key; slots at and above the count hold 63
SCF_HD void sorted_hand(const scopa_full_state &s, int player, int c[3]) {
    const int n = nh_of(s, player);
#pragma unroll
    for (int j = 0; j < 3; j++) c[j] = j < n ? hand_get(s, player, j) : 63;
    int t;
    if (c[0] > c[1]) { t = c[0]; c[0] = c[1]; c[1] = t; }
    if (c[1] > c[2]) { t = c[1]; c[1] = c[2]; c[2] = t; }
    if (c[0] > c[1]) { t = c[0]; c[0] = c[1]; c[1] = t; }
}

SCF_HD int card_at(const int c[3], int a) { return a == 0 ? c[0] : (a == 1 ? c[1] : c[2]); }

// the root on `deck`: a root with the deck's deal of its round in hand
SCF_HD scopa_full_state root_on(const scopa_full_state &root, const uint8_t *deck) {
    scopa_full_state s = root;
    const int base = 4 + 6 * (int)root.round;
    s.hand[0] = (uint32_t)deck[base] | ((uint32_t)deck[base + 1] << 6) | ((uint32_t)deck[base + 2] << 12);
    s.hand[1] = (uint32_t)deck[base + 3] | ((uint32_t)deck[base + 4] << 6) | ((uint32_t)deck[base + 5] << 12);
    s.nh[0] = s.nh[1] = 3;
    return s;
}

// what create and the exact sweeps ask of a root (the first clause of root_check: a non-terminal round boundary; the hands are ignored) ...
inline bool root_ok(const scopa_full_state &root) {
    return !root.terminal && root.step % 6 == 0 && root.round <= 5 && root.step == 6 * root.round && root.deck_pos == 10 + 6 * root.round &&
           root.nt <= kMaxTable && !(root.flags & 1u);
}

// ... and of a deck below it: a permutation whose cards from position 4 + 6 round on are exactly the cards not on the root's table or in its capture
// piles; at round 0 the table is the deck's first four cards in order (the table is ordered and the capture rule reads the order)
inline bool deck_fits(const uint8_t *d, const scopa_full_state &root) {
    uint64_t seen = 0ull, rest = 0ull, used = root.cap[0] | root.cap[1];
    const int first = 4 + 6 * (int)root.round;
    for (int i = 0; i < 40; i++) {
        if (d[i] > 39) return false;
        seen |= 1ull << d[i];
        if (i >= first) rest |= 1ull << d[i];
    }
    if (seen != kCardMask || (root.cap[0] & root.cap[1])) return false;
    int n_used = popc64(root.cap[0]) + popc64(root.cap[1]);
    for (int i = 0; i < root.nt; i++) {
        const int c = tab_get(root, i);
        if (c > 39 || ((used >> c) & 1ull)) return false;
        used |= 1ull << c;
        n_used++;
    }
    if (n_used != first || rest != (kCardMask & ~used)) return false;
    if (root.round == 0) {
        if (root.nt != 4) return false;
        for (int i = 0; i < 4; i++) if (tab_get(root, i) != d[i]) return false;
    }
    return true;
}

struct alignas(128) FwSlot {
    unsigned long long key;            // word A
    double regret[3], strategy[3], d_regret[3], d_strategy[3];
    uint32_t count, pad32;
    unsigned long long key_b;          // word B
    uint64_t pad;
};
static_assert(sizeof(FwSlot) == 128, "one slot per 128-byte line");

__host__ __device__ __forceinline__ uint32_t fw_home(uint64_t a, uint64_t b, uint32_t mask) { return fm_hash(a ^ (b * kWideMul)) & mask; }

#if defined(__HIPCC__)
// the slot of (a, b), or -1 where the store does not hold it (an unpublished slot of word a included); never writes
__device__ __forceinline__ int fw_find(const FwSlot *tab, uint32_t mask, uint64_t a, uint64_t b) {
    uint32_t i = fw_home(a, b, mask);
    for (int p = 0; p < kMaxProbe; p++, i = (i + 1u) & mask) {
        const unsigned long long k = __hip_atomic_load(&tab[i].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == 0ull) return -1;
        if (k == a) {
            const unsigned long long w = __hip_atomic_load(&tab[i].key_b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (w == b) return (int)i;
            if (w == 0ull) return -1;
        }
    }
    return -1;
}

// the slot of (a, b), claimed if the store does not hold it yet; -1 (and dropped += 1) where kMaxProbe slots hold other pairs
__device__ __forceinline__ int fw_claim(FwSlot *tab, uint32_t mask, uint64_t a, uint64_t b, unsigned long long *cnt) {
    uint32_t i = fw_home(a, b, mask);
    for (int p = 0; p < kMaxProbe; p++, i = (i + 1u) & mask) {
        unsigned long long k = __hip_atomic_load(&tab[i].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == 0ull) {
            k = atomicCAS(&tab[i].key, 0ull, (unsigned long long)a);      // one attempt: a lost race leaves the winner's word in k
            if (k == 0ull) k = a;
        }
        if (k != a) continue;
        unsigned long long w = __hip_atomic_load(&tab[i].key_b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (w == 0ull) {
            w = atomicCAS(&tab[i].key_b, 0ull, (unsigned long long)b);    // one attempt again; after a won word A this lane always gets here
            if (w == 0ull) { atomicAdd(cnt + kCntRows, 1ull); return (int)i; }
        }
        if (w == b) return (int)i;
    }
    atomicAdd(cnt + kCntDropped, 1ull);
    return -1;
}
#endif

template <> struct SlotKey<FwSlot> {
    static constexpr int kWords = 2;
    static constexpr const char *kWho = "scopa_full_chance";
    static constexpr const char *kExport = "k_full_chance_export", *kImport = "k_full_chance_import";
    static constexpr const char *kBadKey = "a key without the marker bit, a hand word at or above 1 << 40, or an action count that is not the hand's (2 or 3)";
    static constexpr const char *kTwice = "a key pair twice";
    static void set(FwSlot &row, const uint64_t *k) { row.key = k[0]; row.key_b = k[1]; }
    static void get(const FwSlot &row, uint64_t *k) { k[0] = row.key; k[1] = row.key_b; }
    static int actions(const FwSlot &row) { return popc64(row.key_b); }
    static bool key_ok(const FwSlot &row) { return (row.key >> 63) == 1ull && row.key_b <= kCardMask; }
#if defined(__HIPCC__)
    static __device__ __forceinline__ int claim(FwSlot *tab, uint32_t mask, const FwSlot &row, unsigned long long *cnt) { return fw_claim(tab, mask, row.key, row.key_b, cnt); }
#endif
};

struct FwEval;                                // the exact sweeps' scratch and last response rows (scopa_full_chance_eval.hip)
void chance_eval_free(FwEval *e);             // scopa_full_chance_eval.hip; the stream must be idle
struct FwCfr;                                 // the exact CFR iteration's scratch (scopa_full_chance_cfr.hip)
void chance_cfr_free(FwCfr *c);               // scopa_full_chance_cfr.hip; the stream must be idle
struct FwXplay;                               // the cross-play scratch (scopa_full_chance_xplay.hip)
void chance_xplay_free(FwXplay *x);           // scopa_full_chance_xplay.hip; the stream must be idle
struct FwSdcfr;                               // Deep CFR's forest, policy tables and visit count (scopa_full_chance_sdcfr.hip)
void chance_sdcfr_free(FwSdcfr *c);           // scopa_full_chance_sdcfr.hip; the stream must be idle

}  // namespace scopa_full

struct scopa_full_chance : scopa_full::StoreHandle<scopa_full::FwSlot> {
    uint8_t *d_decks = nullptr;               // [n_decks][40]
    uint8_t *decks = nullptr;                 // the host copy
    int32_t n_decks = 0;
    scopa_full::FwEval *eval = nullptr;       // allocated by the first scopa_full_chance_exploitability, freed by destroy
    scopa_full::FwCfr *cfr = nullptr;         // allocated by the first scopa_full_chance_cfr_iterate, freed by destroy
    scopa_full::FwXplay *xplay = nullptr;     // allocated by the first scopa_full_chance_cross_play with this handle first, freed by destroy
    scopa_full::FwSdcfr *sd = nullptr;        // allocated by the first scopa_full_chance_sdcfr_traverse / _average_policy, freed by destroy
};
