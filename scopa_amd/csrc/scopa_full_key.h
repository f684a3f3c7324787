// scopa_full_key.h -- the 64-bit infoset key of FullScopa: what scopa_full_state_infoset_string says about a decision node of `player`, packed so that
// the solvers can keep rows by key (scopa_full_mccfr.hip) without enumerating the tree.
//
//   bit 63      always 1: a key is never 0, the empty-slot word of the store
//   bit 62      player
//   bits 59-61  round (0..5)
//   bits 56-58  hand: which of the player's three cards of the round (deck[4 + 6 * round + 3 * player + i], bit i) are still held
//   bits 16-55  table, a 40-bit card mask (the string sorts the table: order is not information)
//   bits 10-15  cards captured by `player`
//   bits 5-9    scopas of player 0;  bits 0-4  scopas of player 1
//
// The opponent's capture count is not packed: at a decision node of `player` the 4 + 6 * (round + 1) cards dealt so far are the two capture piles, the
// table and the two hands, and the opponent holds as many cards as the mover (player 0 moving) or one fewer (player 1 moving).  So over the decision
// nodes of ONE deck, two (state, mover) pairs have equal keys exactly when their strings are equal.  The hand is a subsequence of the deal order (step()
// closes the gap a played card leaves), so action slot a of a key is the a-th set hand bit wherever the key occurs on the deck.
#pragma once
#include "scopa_full_rules.h"

namespace scopa_full {

constexpr int kKeyHandShift = 56, kKeyTableShift = 16;

SCF_HD uint64_t infoset_key(const scopa_full_state &s, const uint8_t *deck, int player) {
    const int base = 4 + 6 * (int)s.round + 3 * player, n = nh_of(s, player);
    uint64_t sub = 0ull;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int c = deck[base + i];
        bool held = false;
#pragma unroll
        for (int j = 0; j < 3; j++) held = held || (j < n && hand_get(s, player, j) == c);
        sub |= (uint64_t)held << i;
    }
    uint64_t table = 0ull;
SCF_UNROLL
    for (int i = 0; i < kMaxTable; i++) {
        if (!any_lane(i < s.nt)) break;
        if (i < s.nt) table |= 1ull << tab_get(s, i);
    }
    const uint64_t own = (uint64_t)popc64(player ? s.cap[1] : s.cap[0]);
    return (1ull << 63) | ((uint64_t)player << 62) | ((uint64_t)(s.round & 7) << 59) | (sub << kKeyHandShift) | (table << kKeyTableShift) |
           (own << 10) | ((uint64_t)(s.scopas[0] & 31) << 5) | (uint64_t)(s.scopas[1] & 31);
}

// the number of cards the mover of a key holds = its action count
SCF_HD int key_actions(uint64_t key) {
    const uint32_t h = (uint32_t)(key >> kKeyHandShift) & 7u;
    return (int)((h & 1u) + ((h >> 1) & 1u) + (h >> 2));
}

}  // namespace scopa_full
