// scopa_full_store.h -- the keyed store of FullScopa infoset rows and the handle behind scopa_full_mccfr_*, shared by the translation units that read
// it: scopa_full_mccfr.hip (the sampling solver, which also claims slots) and scopa_full_eval.hip (the exact sweeps, which only read).  Also here:
// StoreHandle<Slot>, the part of a handle that this store and the two-word store of scopa_full_wide.h have in common, and SlotKey<Slot>, the one place
// where the two differ for the kernels and host plumbing of scopa_full_store_host.h.
//
//   slot      128 bytes, one line: key | regret[3] | strategy[3] | d_regret[3] | d_strategy[3] | count.  Key word 0 = empty.
//   probe     home = fm_hash(key) & (2^capacity_log2 - 1), then the next slot and the next, wrapping at the end of the table, kMaxProbe = 64 slots in
//             all.  fm_find here is THE read-only probe: nothing is deleted between resets, so an empty slot on the way means the key is absent.
//             fm_claim below walks the same sequence and claims the first empty slot with ONE compare-and-swap; the two loops must agree: with
//             cut > 0 the prefix lanes find what lane 0 claims.  tests/full_mccfr_ref.py restates the sequence.
#pragma once
#include "scopa_ctx.h"
#include "scopa_full_key.h"

namespace scopa_full {

constexpr int kMaxProbe = 64;          // slots a probe may look at
constexpr int kMaxCut = 3;             // a handle's cut: 6^3 = 216 sub-trees, one workgroup of 256 (scopa_full_mccfr_walk.h)

struct alignas(128) FmSlot {
    unsigned long long key;
    double regret[3], strategy[3], d_regret[3], d_strategy[3];
    uint32_t count, pad32;             // (the action count of a row is not stored: it is the number of hand bits of its key)
    uint64_t pad[2];
};
static_assert(sizeof(FmSlot) == 128, "one slot per 128-byte line");

enum { kCntChoice = 0, kCntTerminal, kCntRows, kCntDropped, kCntCursor, kCntWords = 8 };

__host__ __device__ __forceinline__ uint32_t fm_hash(uint64_t k) {   // splitmix64's finaliser
    k ^= k >> 30; k *= 0xBF58476D1CE4E5B9ull;
    k ^= k >> 27; k *= 0x94D049BB133111EBull;
    k ^= k >> 31;
    return (uint32_t)k ^ (uint32_t)(k >> 32);
}

#if defined(__HIPCC__)
// the slot of `key`, or -1 where the store does not hold it; never writes
__device__ __forceinline__ int fm_find(const FmSlot *tab, uint32_t mask, uint64_t key) {
    uint32_t i = fm_hash(key) & mask;
    for (int p = 0; p < kMaxProbe; p++, i = (i + 1u) & mask) {
        const unsigned long long k = __hip_atomic_load(&tab[i].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == key) return (int)i;
        if (k == 0ull) return -1;
    }
    return -1;
}

// the slot of `key`, claimed if the store does not hold it yet; -1 (and dropped += 1) where kMaxProbe slots hold other keys
__device__ __forceinline__ int fm_claim(FmSlot *tab, uint32_t mask, uint64_t key, unsigned long long *cnt) {
    uint32_t i = fm_hash(key) & mask;
    for (int p = 0; p < kMaxProbe; p++, i = (i + 1u) & mask) {
        unsigned long long k = __hip_atomic_load(&tab[i].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == 0ull) {
            k = atomicCAS(&tab[i].key, 0ull, (unsigned long long)key);   // one attempt: a lost race leaves the winner's key in k
            if (k == 0ull) { atomicAdd(cnt + kCntRows, 1ull); return (int)i; }
        }
        if (k == key) return (int)i;
    }
    atomicAdd(cnt + kCntDropped, 1ull);
    return -1;
}
#endif

// what the shared kernels and host plumbing (scopa_full_store_host.h) ask of a slot type: its key words in the caller's uint64 array, the claim, the
// action count, and what tables_set checks of a key and says where it refuses one
template <class Slot> struct SlotKey;
template <> struct SlotKey<FmSlot> {
    static constexpr int kWords = 1;
    static constexpr const char *kWho = "scopa_full_mccfr";
    static constexpr const char *kExport = "k_full_mccfr_export", *kImport = "k_full_mccfr_import";   // a failed launch's name in the error text
    static constexpr const char *kBadKey = "a key without the marker bit, or an action count that is not the key's (2 or 3)";
    static constexpr const char *kTwice = "a key twice";
    static void set(FmSlot &row, const uint64_t *k) { row.key = k[0]; }
    static void get(const FmSlot &row, uint64_t *k) { k[0] = row.key; }
    static int actions(const FmSlot &row) { return key_actions(row.key); }
    static bool key_ok(const FmSlot &row) { return (row.key >> 63) == 1ull; }
#if defined(__HIPCC__)
    static __device__ __forceinline__ int claim(FmSlot *tab, uint32_t mask, const FmSlot &row, unsigned long long *cnt) { return fm_claim(tab, mask, row.key, cnt); }
#endif
};

// what create asks of a root, and the exact sweeps of theirs: 0 = a non-terminal round boundary holding the deck's deal of its round,
// 1 = not a round boundary of a game in play, 2 = the hands are not this deck's deal of the round
inline int root_check(const scopa_full_state &root, const uint8_t *deck40) {
    if (!(!root.terminal && root.step % 6 == 0 && root.round <= 5 && root.step == 6 * root.round && root.deck_pos == 10 + 6 * root.round &&
          root.nh[0] == 3 && root.nh[1] == 3 && root.nt <= kMaxTable && !(root.flags & 1u)))
        return 1;
    for (int p = 0; p < 2; p++)
        for (int i = 0; i < 3; i++)
            if (hand_get(root, p, i) != deck40[4 + 6 * root.round + 3 * p + i]) return 2;
    return 0;
}

struct FmEval;                                // the exact sweeps' scratch and last response rows (scopa_full_eval.hip)
void eval_free(FmEval *e);                    // scopa_full_eval.hip; the stream must be idle

// what the handles of the two stores have in common
template <class S>
struct StoreHandle {
    using Slot = S;
    scopa_ctx *ctx = nullptr;
    S *d_tab = nullptr;
    unsigned long long *d_cnt = nullptr;      // kCntWords counters, then 8 words of match sums
    scopa_full_state root;
    int capacity_log2 = 0, cut = -1;
    uint32_t iteration = 0;                   // applies since create
    uint64_t dropped_seen = 0;                // the dropped counter as the last call left it
};

inline long long *match_sums(unsigned long long *d_cnt) { return (long long *)(d_cnt + kCntWords); }   // the match sums behind the counters

}  // namespace scopa_full

struct scopa_full_mccfr : scopa_full::StoreHandle<scopa_full::FmSlot> {
    uint8_t *d_deck = nullptr;
    uint8_t deck[40] = {0};
    scopa_full::FmEval *eval = nullptr;       // allocated by the first scopa_full_mccfr_exploitability, freed by destroy
};
