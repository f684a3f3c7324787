// scopa_full_chance_match.h -- one episode of the seat-swapped match of FullScopa over a set of decks, ONE definition for the two kernels that play it:
// k_full_chance_match (scopa_full_chance.hip: the agent's store against uniform play) and k_full_chance_pair_match (scopa_full_chance_xplay.hip: the
// agent's store against the average policy of a second store).  The opponent's table is the parameter that tells them apart.
//
//   episode   i is played on deck j % k, j = i in the first half (the agent in seat 0) and i - ceil(n / 2) in the second, so both seats meet the same
//             decks.  A mover with a choice plays prob: uniform 1.0 / n, or strategy[a] / total of its own store's row where the pair is held and
//             total > 1e-12.  kOpp = false: the opponent has no store and plays uniformly.  Draws at Philox counter
//             (i, i >> 32, stream_id << 8 | state.step, 208), slots in ascending card id, fm_pick.
//   sums      r2 of the agent by seat (0, 1), its squares by seat (2, 3), the agent's scopas (4), the opponent's (5): integer atomics, exact in any order.
#pragma once
#include "scopa_full_mccfr_walk.h"
#include "scopa_full_wide.h"

namespace scopa_full {

constexpr uint32_t kMatchTag = 208u;   // Philox counter word 3 of the match draws
constexpr uint32_t kRespondTag = 144u; // ... of the response walks' (a fixed store's, scopa_full_chance.hip; the nets', scopa_full_chance_sdcfr.hip):
                                       // deck_index << 8 | 144 + responder

#if defined(__HIPCC__)
// THE rule by which an average policy is played at a node of nl > 1 legal slots, in its two halves: without a row 1.0 / nl (fw_uniform_probs), and a
// row S over it (fw_row_probs): S[a] / total where total > 1e-12 over the nl legal slots, else what prob held.  A store's row (fw_average_probs) and
// the nets' row of average_at (k_fsm_step and k_frn_step, scopa_full_chance_sdcfr.hip) go through these two and nothing else
__device__ __forceinline__ void fw_uniform_probs(int nl, double prob[3]) {
#pragma unroll
    for (int k = 0; k < 3; k++) prob[k] = 1.0 / (double)nl;
}

__device__ __forceinline__ void fw_row_probs(const double S[3], int nl, double prob[3]) {
    double total = 0.0;
#pragma unroll
    for (int k = 0; k < 3; k++) if (k < nl) total += S[k];
    if (total > 1e-12) {
#pragma unroll
        for (int k = 0; k < 3; k++) prob[k] = S[k] / total;
    }
}

// the rule on a store's average policy, `slot` the node's row in t or -1.  The episode below and the sampled response's opponent (scopa_full_chance.hip) share it
__device__ __forceinline__ void fw_average_probs(const FwSlot *__restrict__ t, int slot, int nl, double prob[3]) {
    fw_uniform_probs(nl, prob);
    if (slot >= 0) {
        double S[3];
#pragma unroll
        for (int k = 0; k < 3; k++) S[k] = t[slot].strategy[k];
        fw_row_probs(S, nl, prob);
    }
}

template <bool kOpp>
__device__ __forceinline__ void full_chance_episode(const FwSlot *__restrict__ tab, uint32_t mask, const FwSlot *__restrict__ opp_tab, uint32_t opp_mask,
                                                    const uint8_t *__restrict__ decks, long long k_decks, const scopa_full_state &root0, long long n,
                                                    uint32_t stream_id, uint32_t seed_lo, uint32_t seed_hi, long long *__restrict__ sums,
                                                    int8_t *__restrict__ r2_agent) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int seat = 2 * i < n ? 0 : 1;
    const long long j = seat ? i - (n + 1) / 2 : i;
    const uint8_t *deck = decks + 40 * (j % k_decks);
    scopa_full_state s = root_on(root0, deck);
    while (!s.terminal) {
        const int p = s.step & 1, nl = nh_of(s, p);
        int cards[3];
        sorted_hand(s, p, cards);
        int a = 0;
        if (nl > 1) {
            double prob[3];
#pragma unroll
            for (int k = 0; k < 3; k++) prob[k] = 1.0 / (double)nl;
            if (kOpp || p == seat) {
                const FwSlot *__restrict__ t = (!kOpp || p == seat) ? tab : opp_tab;
                const uint32_t m = (!kOpp || p == seat) ? mask : opp_mask;
                const WideKey key = wide_key(s, p);
                fw_average_probs(t, fw_find(t, m, key.a, key.b), nl, prob);
            }
            const scopa::philox_out x = scopa::philox4x32_10((uint32_t)i, (uint32_t)((unsigned long long)i >> 32), (stream_id << 8) | (uint32_t)s.step, kMatchTag, seed_lo, seed_hi);
            a = fm_pick(prob, nl, scopa::u53(x.x0, x.x1));
        }
        step(s, deck, card_at(cards, a));
    }
    const long long r2 = seat ? -(long long)s.r2_p0 : (long long)s.r2_p0;
    if (r2_agent) r2_agent[i] = (int8_t)r2;
    atomicAdd((unsigned long long *)sums + seat, (unsigned long long)r2);                      // (two's complement: the sums are signed)
    atomicAdd((unsigned long long *)sums + 2 + seat, (unsigned long long)(r2 * r2));
    atomicAdd((unsigned long long *)sums + 4, (unsigned long long)(seat ? s.scopas[1] : s.scopas[0]));
    atomicAdd((unsigned long long *)sums + 5, (unsigned long long)(seat ? s.scopas[0] : s.scopas[1]));
}
#endif

}  // namespace scopa_full
