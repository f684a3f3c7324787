// scopa_tree_passes.h -- the exact passes over a deal's flat tree, each defined once for the kernels that run it: regret matching, the
// synchronous sweep's pieces (k_cfr_sync, k_cfr_sync_weighted: scopa_eval.hip; k_chance_sweep: scopa_chance.hip), the best-response pass
// (k_exploitability: scopa_eval.hip; k_best_response: scopa_xplay.hip), the cross-play levels (k_cross_play: scopa_xplay.hip; k_chance_cross_play:
// scopa_chance_xplay.hip) and a policy row's sampling thresholds (k_eval_thresholds, k_pair_thresholds, k_chance_pair_thresholds).
//
// Every result of these kernels is pinned bit for bit: a float64 sum here keeps its order and its start value (0.0 or the first element), a
// comparison its form (!(R <= 0.0), strict >), and nothing is contracted (-ffp-contract=off).  The functions are called by every lane of the
// workgroup (they contain barriers where their comments say so); tid / nt are threadIdx.x / blockDim.x.
//
// scopa_mccfr.hip, scopa_sdcfr.hip and scopa_multi.hip do not include this header: the committed counter profiles are keyed by a fingerprint of
// those sources, so scopa_multi.hip keeps a regret_match of its own, and k_cfr_sync, k_cfr_sync_weighted and k_exploitability keep the exact
// signatures of scopa_kernels.h that it launches.
#pragma once
#include "scopa_ctx.h"

namespace scopa {

constexpr int kXWidth = 576;             // the widest ply (level_width(6..8)): one lane per node of a level
constexpr size_t kInfBytes = 1656 * 2;   // a deal's node -> infoset map staged in LDS, rounded up to 8 bytes

// dynamic LDS of the synchronous sweep: regret and sigma tables, reach x2 and values, the infoset map
inline size_t cfr_sync_lds(int n_infosets) { return (size_t)n_infosets * 32 * 2 + sizeof(double) * kNodes * 3 + kInfBytes; }
// ... of the best-response pass: policy and q tables, reach and values, the choices, the infoset map
inline size_t best_response_lds(int n_infosets) {
    return (size_t)n_infosets * 32 * 2 + sizeof(double) * kNodes * 2 + sizeof(int) * (size_t)n_infosets + kInfBytes;
}
// ... of the cross-play levels: the combined table, two adjacent levels of four quantities, the infoset map (include/scopa.h quotes this)
inline size_t cross_play_lds(int n_infosets) { return (size_t)n_infosets * 32 + sizeof(double) * 2 * 4 * kXWidth + kInfBytes; }

// ---- regret matching: InfoNode.get_strategy, vanilla_cfr.py:23-30 ------------------------------------------------------------------------
// writes N entries: a caller that wants a zero-padded row of 4 starts from a zeroed one
template <int N>
__device__ __forceinline__ void regret_match(const double *R, double *out) {
    double pos[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < N; i++) pos[i] = !(R[i] <= 0.0) ? R[i] : 0.0;  // np.maximum(R, 0): a NaN regret stays NaN (the sum is then NaN, not > 0: uniform)
    double s = pos[0];
    for (int i = 1; i < N; i++) s += pos[i];  // np.sum, n < 8: left-to-right
    for (int i = 0; i < N; i++) out[i] = s > 0.0 ? pos[i] / s : 1.0 / (double)N;
}

// the same for a legal count known at run time (1..4; anything else writes nothing)
__device__ __forceinline__ void regret_match_n(int n, const double *R, double *out) {
    if (n == 4) regret_match<4>(R, out); else if (n == 3) regret_match<3>(R, out); else if (n == 2) regret_match<2>(R, out); else if (n == 1) regret_match<1>(R, out);
}

// ---- the synchronous sweep ---------------------------------------------------------------------------------------------------------------
// reach probabilities of both players, top down, from s_r0[0] = s_r1[0] = 1.0 (set by the caller before its last barrier); a barrier per ply
__device__ __forceinline__ void sync_reach_pass(const double *s_sig, const uint16_t *s_inf, double *s_r0, double *s_r1, int tid, int nt) {
    for (int d = 0; d < kPlies; d++) {
        const int n = nlegal_at(d), w1 = level_width(d + 1), p = d & 1;
        for (int j = tid; j < w1; j += nt) {
            const int par = j / n, a = j - par * n;
            const double sg = s_sig[s_inf[level_offset(d) + par] * 4 + a];
            const double a0 = s_r0[level_offset(d) + par], a1 = s_r1[level_offset(d) + par];
            s_r0[level_offset(d + 1) + j] = p == 0 ? a0 * sg : a0;
            s_r1[level_offset(d + 1) + j] = p == 1 ? a1 * sg : a1;
        }
        __syncthreads();
    }
}

// player 0's values at the terminals (no barrier)
__device__ __forceinline__ void sync_terminal_values(const int8_t *__restrict__ g_payoff, double *s_val, int tid, int nt) {
    for (int j = tid; j < kTerminal; j += nt) s_val[level_offset(8) + j] = 0.5 * (double)g_payoff[j];
}

// ply d's node values from ply d + 1's, weighted by the rows of s_sig: children left to right from 0.0 (no barrier)
__device__ __forceinline__ void ply_node_values(int d, const double *s_sig, const uint16_t *s_inf, double *s_val, int tid, int nt) {
    const int n = nlegal_at(d), w = level_width(d), off = level_offset(d);
    for (int j = tid; j < w; j += nt) {
        const int r = s_inf[off + j];
        double v = 0.0;
        for (int a = 0; a < n; a++) v += s_sig[r * 4 + a] * s_val[level_offset(d + 1) + j * n + a];
        s_val[off + j] = v;
    }
}

// the increments of cell (r, a) of a row of ply d: one lane scans the ply's nodes in ascending order, both sums from 0.0
__device__ __forceinline__ void sync_cell_scan(int d, int r, int a, const double *s_sig, const uint16_t *s_inf, const double *s_r0, const double *s_r1,
                                               const double *s_val, double &dR, double &dS) {
    const int n = nlegal_at(d), w = level_width(d), off = level_offset(d), p = d & 1;
    const double sgn = p == 0 ? 1.0 : -1.0;
    dR = 0.0; dS = 0.0;
    const double sg = s_sig[r * 4 + a];
    for (int j = 0; j < w; j++) {
        if (s_inf[off + j] != r) continue;
        const double reach = p == 0 ? s_r0[off + j] : s_r1[off + j], opp = p == 0 ? s_r1[off + j] : s_r0[off + j];
        dR += opp * (sgn * (s_val[level_offset(d + 1) + j * n + a] - s_val[off + j]));
        dS += reach * sg;
    }
}

// ---- the best-response pass --------------------------------------------------------------------------------------------------------------
// Pass `br` on the policy in s_pol: 0 / 1 the best response of that player, 2 nobody responds (the plain value for player 0).  Reach of everyone
// but the responder top down; terminals; bottom up, on a responder ply q[I][a] = sum over the infoset's nodes, in node order from 0.0, of
// reach * value(child a) -- one lane per (infoset, action) scans the ply (<= 576 nodes) so the order is fixed -- then the argmax by a strict `>`
// (ties to the lowest action) and the selected values; any other ply takes policy-weighted values.  Leaves the root in s_val[0] and the
// responder's choices in s_choice; ends on a barrier.
__device__ __forceinline__ void best_response_pass(int br, const int8_t *__restrict__ g_payoff, const uint64_t *__restrict__ g_key, int I, const double *s_pol,
                                                   double *s_q, double *s_reach, double *s_val, int *s_choice, const uint16_t *s_inf, int tid, int nt) {
    // top-down: reach of everyone but the best responder
    if (tid == 0) s_reach[0] = 1.0;
    __syncthreads();
    for (int d = 0; d < kPlies; d++) {
        const int n = nlegal_at(d), w1 = level_width(d + 1), p = d & 1;
        for (int j = tid; j < w1; j += nt) {
            const int par = j / n, a = j - par * n;
            const double r = s_reach[level_offset(d) + par];
            s_reach[level_offset(d + 1) + j] = p == br ? r : r * s_pol[s_inf[level_offset(d) + par] * 4 + a];
        }
        __syncthreads();
    }
    // terminals
    for (int j = tid; j < kTerminal; j += nt) {
        const int p0 = g_payoff[j];
        s_val[level_offset(8) + j] = 0.5 * (double)(br == 1 ? -p0 : p0);
    }
    __syncthreads();
    // bottom-up; unrolled, so that a ply's width, offsets and legal count are constants of its copy
#pragma unroll
    for (int d = kPlies - 1; d >= 0; d--) {
        const int n = nlegal_at(d), w = level_width(d), off = level_offset(d), p = d & 1;
        if (p == br) {
            for (int cell = tid; cell < I * 4; cell += nt) {
                const int r = cell >> 2, a = cell & 3;
                if ((int)(g_key[r] & 1) != p || (int)((g_key[r] >> 1) & 7) != n || a >= n) continue;
                double q = 0.0;
                for (int j = 0; j < w; j++)
                    if (s_inf[off + j] == r) q += s_reach[off + j] * s_val[level_offset(d + 1) + j * n + a];
                s_q[cell] = q;
            }
            __syncthreads();
            for (int r = tid; r < I; r += nt) {
                if ((int)(g_key[r] & 1) != p || (int)((g_key[r] >> 1) & 7) != n) continue;
                int best = 0;
                for (int a = 1; a < n; a++) if (s_q[r * 4 + a] > s_q[r * 4 + best]) best = a;
                s_choice[r] = best;
            }
            __syncthreads();
            for (int j = tid; j < w; j += nt) s_val[off + j] = s_val[level_offset(d + 1) + j * n + s_choice[s_inf[off + j]]];
        } else {
            ply_node_values(d, s_pol, s_inf, s_val, tid, nt);
        }
        __syncthreads();
    }
}

// ---- the cross-play levels ---------------------------------------------------------------------------------------------------------------
// Four quantities -- seat 0's reward, its square, the scopas of either seat -- set at the 576 terminals of the deal (payoff, states: the deal's own)
// and carried up the eight plies by the combined table in s_pol, v = 0.0; v += row[c] * child[c], children left to right.  Only two adjacent
// levels are alive at a time, s_lvl[2][4][kXWidth]; the three LDS areas are disjoint (__restrict__).  The first barrier also covers what the caller staged into s_pol and s_inf.  Returns the
// buffer that holds the root: quantity q is s_lvl[(cur * 4 + q) * kXWidth].
__device__ __forceinline__ int cross_play_levels(const double *__restrict__ s_pol, double *__restrict__ s_lvl, const uint16_t *__restrict__ s_inf, const int8_t *__restrict__ payoff,
                                                 const scopa_state *__restrict__ states, int tid, int nt) {
    for (int j = tid; j < kTerminal; j += nt) {
        const int p0 = payoff[j];
        const uint32_t w = reinterpret_cast<const uint4 *>(states)[kDecision + j].w;   // ncap[2] | scopas[2]
        s_lvl[0 * kXWidth + j] = 0.5 * (double)p0;
        s_lvl[1 * kXWidth + j] = 0.25 * (double)p0 * (double)p0;
        s_lvl[2 * kXWidth + j] = (double)((w >> 16) & 255u);
        s_lvl[3 * kXWidth + j] = (double)(w >> 24);
    }
    __syncthreads();
    int cur = 0;   // the buffer that holds ply d + 1
    for (int d = kPlies - 1; d >= 0; d--) {
        const int n = nlegal_at(d), w = level_width(d), off = level_offset(d);
        const double *child = s_lvl + cur * 4 * kXWidth;
        double *mine = s_lvl + (cur ^ 1) * 4 * kXWidth;
        for (int j = tid; j < w; j += nt) {
            const double *row = s_pol + (size_t)s_inf[off + j] * 4;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                double v = 0.0;
                for (int c = 0; c < n; c++) v += row[c] * child[q * kXWidth + j * n + c];
                mine[q * kXWidth + j] = v;
            }
        }
        cur ^= 1;
        __syncthreads();
    }
    return cur;
}

// ---- sampling thresholds of a policy row ---------------------------------------------------------------------------------------------------
// np.random.choice(actions, p = probs) is index = #{q : cdf_q / cdf_last <= u}, and every u an episode draws is N * 2^-53 with an integer N; x * 2^53
// is exact in float64, so x <= u  <=>  ceil(x * 2^53) <= N.  thr[k] = ceil(cdf_k / cdf_last * 2^53) for k < n - 1, 0 where the quotient is <= 0,
// 2^53 (never counted) beyond, where it is >= 1 or NaN (a row that sums to 0 or NaN), and for a legal count outside 1..4.
__device__ __forceinline__ void policy_thresholds(int n, const double *__restrict__ row, unsigned long long *__restrict__ thr /*[3]*/) {
    double c = 0.0, cdf[4] = {0.0, 0.0, 0.0, 0.0};
    for (int q = 0; q < n && q < 4; q++) { c = q ? c + row[q] : row[0]; cdf[q] = c; }
    const double last = n > 0 && n <= 4 ? cdf[n - 1] : 0.0;
    for (int k = 0; k < 3; k++) {
        unsigned long long t = 1ull << 53;
        if (k < n - 1) {
            const double x = cdf[k] / last;
            if (x <= 0.0) t = 0ull;                                  // x <= u for every u >= 0
            else if (x < 1.0) t = (unsigned long long)ceil(x * 9007199254740992.0);
            // x >= 1 or NaN: never <= u (u < 1)
        }
        thr[k] = t;
    }
}

}  // namespace scopa
