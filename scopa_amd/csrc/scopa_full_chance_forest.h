// scopa_full_chance_forest.h -- the kernels that lay out the deck-major FOREST of FullScopa over a set of decks, ONE definition for the two translation
// units that sweep it: scopa_full_chance_eval.hip (the exact value and response across the decks) and scopa_full_chance_cfr.hip (the exact weighted CFR
// iteration).  The forest is stated in scopa_full_chance_eval.hip's head and under `exploitability` of scopa_full_chance in include/scopa.h.
//
//   roots     k_full_chance_eval_roots, a lane per deck: root_on(root, deck d), and w = 1.0.
//   expand    k_full_chance_eval_expand, a lane per child: the deck from the child's index, the mover's a-th card in ASCENDING CARD ID (sorted_hand),
//             one step, three at a round's last choice level (full_chance_forest_child, which scopa_full_chance_xplay.hip's expand calls too).
//   gather    k_full_chance_eval_gather: a key word carried through a sort pass's permutation.
//   mean      k_full_chance_eval_mean, one lane: (0.0 + V[root 0] + V[root 1] + ...) / n in deck order.
#pragma once
#include "scopa_full_eval_passes.h"
#include "scopa_full_wide.h"

namespace scopa_full {
namespace {

constexpr uint64_t kMaxLeaves = 1ull << 22;   // n x 36^R: 3 236 decks at R = 2, 89 at R = 3, 2 at R = 4
constexpr unsigned kHandSortBits = 40;        // word B is a 40-bit card mask

__global__ void __launch_bounds__(256)
k_full_chance_eval_roots(const scopa_full_state root, const uint8_t *__restrict__ decks, uint32_t n, scopa_full_state *__restrict__ state,
                         double *__restrict__ w) {
    const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= n) return;
    state[d] = root_on(root, decks + 40u * d);
    w[d] = 1.0;
}

// child c of a level whose mover p holds n cards: the state after the mover's a-th card in ascending card id, a = c % n, and at a round's last
// choice level after the two one-card plies too.  tree_child: the nodes ONE tree has in the children's level (c < decks x tree_child)
__device__ __forceinline__ scopa_full_state full_chance_forest_child(const scopa_full_state *__restrict__ parent, uint32_t c, uint32_t tree_child, int p, int n,
                                                                     int round_end, const uint8_t *__restrict__ decks) {
    const uint32_t g = c / (uint32_t)n;
    const int a = (int)(c - g * (uint32_t)n);
    const uint8_t *deck = decks + 40u * (c / tree_child);
    scopa_full_state s = parent[g];
    int cards[3];
    sorted_hand(s, p, cards);
    step(s, deck, card_at(cards, a));
    if (round_end) {                                              // the one-card plies: player 0's last card, then player 1's
        step(s, deck, hand_get(s, 0, 0));
        step(s, deck, hand_get(s, 1, 0));
    }
    return s;
}

__global__ void __launch_bounds__(256)
k_full_chance_eval_expand(const scopa_full_state *__restrict__ parent, uint32_t n_child, uint32_t tree_child, int p, int n, int round_end,
                          const uint8_t *__restrict__ decks, scopa_full_state *__restrict__ child, double *__restrict__ leaf) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_child) return;
    const scopa_full_state s = full_chance_forest_child(parent, c, tree_child, p, n, round_end, decks);
    if (leaf) leaf[c] = (double)s.r2_p0 / 2.0;
    else child[c] = s;
}

// dst[k] = src[idx[k]]: a key word carried through a pass's permutation (idx[k] < N: a permutation of the level's nodes)
__global__ void __launch_bounds__(256)
k_full_chance_eval_gather(const unsigned long long *__restrict__ src, const uint32_t *__restrict__ idx, uint32_t N, unsigned long long *__restrict__ dst) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= N) return;
    dst[k] = src[idx[k]];
}

// one lane: the mean of the n roots' values, added in deck order
__global__ void k_full_chance_eval_mean(const double *__restrict__ V, uint32_t n, double *__restrict__ out) {
    if (blockIdx.x != 0u || threadIdx.x != 0u) return;
    double v = 0.0;
    for (uint32_t d = 0; d < n; d++) v += V[d];
    *out = v / (double)n;
}

}  // namespace
}  // namespace scopa_full
