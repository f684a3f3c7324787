// scopa_full_mccfr_walk.h -- THE external-sampling traversal of FullScopa, one definition for its two solvers: scopa_full_mccfr.hip (one deck, one-word
// keys in hand order) and scopa_full_chance.hip (a set of decks, deck-free two-word keys in ascending card id).  What differs between them is a policy P:
//
//   P::Args                      the launch's arguments; the walk reads tab (slots with regret / d_regret / d_strategy / count), cnt, mask-free fields
//                                iteration, seed_lo, seed_hi, traverser, cut
//   P::Lane(A, g)                lane or workgroup g of the launch: exists, deck (the 40 cards the walk deals from), trav_id, tag (Philox counter word 3)
//   P::root(A, deck)             the state the traversal starts from
//   P::card(s, p, a)             the card of action slot a of mover p
//   P::find(A, s, deck, p)       the slot of the mover's row or -1, read-only;  P::claim(...): claimed where absent, -1 (and dropped += 1) on a full probe
//   P::kRespond                  false: the non-traverser plays the store's own frozen sigma and its row takes d_strategy and a visit (training).
//                                true: the non-traverser is a FIXED policy outside the store -- P::opp_probs(A, s, p, n, prob) gives its probabilities,
//                                no row of it is claimed, written or counted, and the traverser's rows are all the launch touches (a sampled response)
//
//   traverse  regrets are FROZEN for the launch: a traversal reads `regret` and adds only into d_regret / d_strategy / count (float64 and uint32
//             atomics), so sigma at a key is the same wherever and whenever the launch meets it, a draw named by its node (ply, the traverser's
//             choices so far, traversal id, iteration, tag) is the same however the work is cut, and a sub-tree may be walked by another lane that
//             recomputes the prefix leading to it.
//   cut       cut = K > 0: a workgroup per g; lane c < 6^K replays the first K rounds with the traverser's choices fixed to the digits of c
//             (no writes), walks the sub-tree below with updates and leaves its value in LDS; after one workgroup barrier lane 0 walks the first
//             K rounds with updates, reading the value of sub-tree q where it reaches the cut.  cut = 0: a lane per g walks everything.
#pragma once
#include "scopa_full_store.h"
#include "scopa_mccfr_sigma.h"
#include "scopa_philox.h"

namespace scopa_full {

constexpr int kMaxFrames = 12;         // traverser nodes with a choice on one path: two per round
constexpr int kNoStop = 0x7FFFFFFF;

__device__ __forceinline__ void fm_row(const double *src, int slot, double R[4]) {
#pragma unroll
    for (int a = 0; a < 3; a++) R[a] = slot >= 0 ? src[a] : 0.0;
    R[3] = 0.0;
}

// first slot whose running sum of the probabilities exceeds u; the last legal slot as fallback
__device__ __forceinline__ int fm_pick(const double *prob, int n, double u) {
    double acc = 0.0;
    int a = n - 1;
    bool found = false;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        if (i < n) {
            acc += prob[i];
            if (!found && acc > u) { a = i; found = true; }
        }
    }
    return a;
}

struct FmFrame {
    scopa_full_state s;
    double sigma[3], cfv[3];
    int slot, a, n;
    uint32_t q;
};

template <class Args>
__device__ __forceinline__ double fm_draw(const Args &A, uint32_t tag, uint32_t trav_id, const scopa_full_state &s, uint32_t q) {
    const scopa::philox_out x = scopa::philox4x32_10(((uint32_t)s.step << 16) | q, trav_id, A.iteration, tag, A.seed_lo, A.seed_hi);
    return scopa::u53(x.x0, x.x1);
}

// the body of a traversal kernel; s_vals: 216 doubles of LDS.  Every lane of the workgroup calls it (it holds the workgroup barrier of cut > 0)
template <class P>
__device__ __forceinline__ void full_mccfr_walk(const typename P::Args &A, double *s_vals) {
    const int tid = threadIdx.x, K = A.cut, trav = A.traverser;
    int T = 1;
    for (int k = 0; k < K; k++) T *= 6;
    const typename P::Lane L(A, K ? blockIdx.x : blockIdx.x * blockDim.x + (uint32_t)tid);
    const bool exists = L.exists;
    const uint32_t trav_id = L.trav_id;
    const uint8_t *deck = L.deck;
    const scopa_full_state root = P::root(A, deck);
    unsigned long long n_choice = 0ull, n_term = 0ull;
    FmFrame st[kMaxFrames];

    for (int pass = 0; pass < (K ? 2 : 1); pass++) {
        if (pass) __syncthreads();                          // (K and pass are the same in every lane of the workgroup)
        scopa_full_state s = root;
        uint32_t q = 0u;
        int stop = kNoStop;
        bool active = exists;
        if (K && pass == 0) {
            active = exists && tid < T;
            if (active) {                                   // the prefix of sub-tree `tid`: the traverser's digits, the opponent's node-keyed draws, no writes
                int rest = T, c = tid;
                const int cut_step = (int)root.step + 6 * K;
                while (!s.terminal && (int)s.step < cut_step) {
                    const int p = s.step & 1, n = nh_of(s, p);
                    int a = 0;
                    if (n > 1) {
                        if (p == trav) { rest /= n; a = c / rest; c -= a * rest; q = q * (uint32_t)n + (uint32_t)a; }
                        else {
                            double sigma[4];
                            if constexpr (P::kRespond) P::opp_probs(A, s, p, n, sigma);
                            else {
                                double R[4];
                                const int slot = P::find(A, s, deck, p);
                                fm_row(A.tab[slot >= 0 ? slot : 0].regret, slot, R);
                                scopa::mc_sigma(R, n, sigma);
                            }
                            a = fm_pick(sigma, n, fm_draw(A, L.tag, trav_id, s, q));
                        }
                    }
                    step(s, deck, P::card(s, p, a));
                }
            }
        } else if (K) {
            active = exists && tid == 0;
            stop = (int)root.step + 6 * K;
        }
        if (!active) continue;

        int d = 0;
        double ret = 0.0;
        bool down = true;
        for (;;) {
            if (down) {
                if ((int)s.step == stop) { ret = s_vals[q]; down = false; continue; }
                if (s.terminal) {
                    ret = 0.5 * (double)s.r2_p0;
                    if (trav) ret = -ret;
                    n_term++;
                    down = false;
                    continue;
                }
                const int p = s.step & 1, n = nh_of(s, p);
                if (n <= 1) { step(s, deck, P::card(s, p, 0)); continue; }       // one card: no row, no draw, no count
                n_choice++;
                if constexpr (P::kRespond) {
                    if (p != trav) {                                             // the fixed opponent: no claim, no write, no count
                        double prob[4];
                        P::opp_probs(A, s, p, n, prob);
                        const int a = fm_pick(prob, n, fm_draw(A, L.tag, trav_id, s, q));
                        step(s, deck, P::card(s, p, a));
                        continue;
                    }
                }
                const int slot = P::claim(A, s, deck, p);
                double R[4], sigma[4];
                fm_row(A.tab[slot >= 0 ? slot : 0].regret, slot, R);
                scopa::mc_sigma(R, n, sigma);
                if (p != trav) {
                    if (slot >= 0) {
#pragma unroll
                        for (int a = 0; a < 3; a++) if (a < n) atomicAdd(&A.tab[slot].d_strategy[a], sigma[a]);
                        atomicAdd(&A.tab[slot].count, 1u);
                    }
                    const int a = fm_pick(sigma, n, fm_draw(A, L.tag, trav_id, s, q));
                    step(s, deck, P::card(s, p, a));
                    continue;
                }
                if (d >= kMaxFrames) { ret = 0.0; down = false; continue; }      // (not reachable from a checked root: two such nodes per round)
                FmFrame &f = st[d++];
                f.s = s; f.slot = slot; f.a = 0; f.n = n; f.q = q;
#pragma unroll
                for (int a = 0; a < 3; a++) { f.sigma[a] = sigma[a]; f.cfv[a] = 0.0; }
                q = q * (uint32_t)n;
                step(s, deck, P::card(s, p, 0));
            } else {
                if (d == 0) break;
                FmFrame &f = st[d - 1];
                f.cfv[f.a] = ret;
                f.a++;
                if (f.a < f.n) {
                    s = f.s;
                    q = f.q * (uint32_t)f.n + (uint32_t)f.a;
                    step(s, deck, P::card(f.s, trav, f.a));
                    down = true;
                } else {
                    double v = 0.0;
#pragma unroll
                    for (int a = 0; a < 3; a++) if (a < f.n) v += f.sigma[a] * f.cfv[a];
                    if (f.slot >= 0) {
#pragma unroll
                        for (int a = 0; a < 3; a++) if (a < f.n) atomicAdd(&A.tab[f.slot].d_regret[a], f.cfv[a] - v);
                        atomicAdd(&A.tab[f.slot].count, 1u);
                    }
                    ret = v;
                    d--;
                }
            }
        }
        if (K && pass == 0) s_vals[tid] = ret;
    }
    if (n_choice) atomicAdd(A.cnt + kCntChoice, n_choice);
    if (n_term) atomicAdd(A.cnt + kCntTerminal, n_term);
}

}  // namespace scopa_full
