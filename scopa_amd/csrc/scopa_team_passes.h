// scopa_team_passes.h -- the Team MiniScopa tree passes, one definition each, for the one-deal solver (scopa_team_cfr.hip) and the solver over a
// set of deals (scopa_team_chance.hip): the first-round cut and its LDS layout, the arithmetic of a CFR node (value, increments, weighted update),
// the reach passes, the node of a value pass, the walk from a deal's root along a row's path, the average-policy row.  The two solvers differ in
// where a row lives (the node's own row / the shared row of its key, through the deal's map) and in who applies an increment (the node's lane /
// the reduce over the key's occurrences); what is computed per node is this file's.
#pragma once
#include <string.h>

#include "scopa_team_rules.h"
#include "scopa_team_solver.h"
#include "scopa_tree_passes.h"

namespace {

constexpr int kCutDepth = 4, kSubtrees = 256, kTopRows = 85;                // depths 0..3 hold 1 + 4 + 16 + 64 nodes
constexpr int kSubRows = 1255, kSubLeaves = 1296;                           // one depth-4 subtree: 1 + 3 + 9 + 27 + 81 + 162 + 324 + 648 rows
constexpr int kSubThreads = 256;   // the widest level has 648 rows / 1 296 leaves: three to five rounds of four wavefronts, one per SIMD

// a depth-4 subtree's level d (4..12): its width and its offset among the subtree's rows (level 12 = the leaves, right after the 1 255 rows)
__host__ __device__ constexpr int s_width(int d) { return t_width(d) / kSubtrees; }
__host__ __device__ constexpr int s_offset(int d) { int o = 0; for (int k = kCutDepth; k < d; k++) o += s_width(k); return o; }
static_assert(t_offset(4) == kTopRows && s_offset(12) == kSubRows && s_width(12) == kSubLeaves, "tree shape");

// LDS of a subtree sweep (dynamic, 80 648 bytes): the subtree's 1 255 sigma rows staged whole (they are read on the way down and again on the way
// up), both reaches of its rows, the values of rows and leaves.
constexpr size_t kSubLds = sizeof(double) * ((size_t)kSubRows * 4 + kSubRows * 2 + kSubRows + kSubLeaves);

// ---- one node of the CFR sweep (vanilla_cfr.py:87-97) with B legal actions -------------------------------------------------------------------
// value = np.sum(local_strategy * action_utils), the products added left to right
template <int B>
__device__ __forceinline__ double cfr_value(const double *u, const double *ls) {
    double v = ls[0] * u[0];
#pragma unroll
    for (int c = 1; c < B; c++) v += ls[c] * u[c];
    return v;
}

// what a traverser's node adds to its row: regret_sum += opponent_reach * (action_utils - value), strategy_sum += reach * local_strategy
template <int B>
__device__ __forceinline__ void cfr_increments(const double *u, const double *ls, double v, double reach, double opp, double *dR, double *dS) {
#pragma unroll
    for (int c = 0; c < B; c++) {
        dR[c] = opp * (u[c] - v);
        dS[c] = reach * ls[c];
    }
}

// the row's update with the iteration's weights: R <- R + dR; R <- !(R <= 0) ? R * pos : R * neg; S <- (S + dS) * strat
template <int B>
__device__ __forceinline__ void cfr_apply(Row4 &R, Row4 &S, const double *dR, const double *dS, double wpos, double wneg, double wstrat) {
#pragma unroll
    for (int c = 0; c < B; c++) {
        const double r = R.x[c] + dR[c];
        R.x[c] = !(r <= 0.0) ? r * wpos : r * wneg;
        S.x[c] = (S.x[c] + dS[c]) * wstrat;
    }
}

// the terminal's reward for team `persp` at a depth-12 node: 0.5 * r2 of that team, exact
__device__ __forceinline__ double leaf_value(int r2_team0, int persp) { return 0.5 * (double)(persp == 0 ? r2_team0 : -r2_team0); }

// ---- reaches ---------------------------------------------------------------------------------------------------------------------------
// the running products from the root down (vanilla_cfr.py:83-85) along the four ancestors of subtree g's root; row_of(level-major row) is the sigma
// table's row of that node
template <class RowOf>
__device__ __forceinline__ void sub_root_reaches(int g, const double *g_sig, RowOf row_of, double &r0, double &r1) {
    r0 = 1.0; r1 = 1.0;
#pragma unroll
    for (int d = 0; d < kCutDepth; d++) {
        const int idx = g >> (2 * (kCutDepth - d)), a = (g >> (2 * (kCutDepth - 1 - d))) & 3;
        const double sg = g_sig[(size_t)row_of(t_offset(d) + idx) * 4 + a];
        if (t_team(d) == 0) r0 = r0 * sg; else r1 = r1 * sg;
    }
}

// reaches of a subtree's level D + 1 from level D, in LDS; a barrier behind it
template <int D>
__device__ __forceinline__ void sub_reach_level(const double *s_sig, double *s_r0, double *s_r1, int tid) {
    constexpr int b = t_branch(D), w1 = s_width(D + 1), lo = s_offset(D), lo1 = s_offset(D + 1);
    for (int j = tid; j < w1; j += kSubThreads) {
        const int par = j / b, a = j - par * b;
        const double sg = s_sig[(lo + par) * 4 + a], a0 = s_r0[lo + par], a1 = s_r1[lo + par];
        s_r0[lo1 + j] = t_team(D) == 0 ? a0 * sg : a0;
        s_r1[lo1 + j] = t_team(D) == 1 ? a1 * sg : a1;
    }
    __syncthreads();
}

__device__ __forceinline__ void sub_reach_pass(const double *s_sig, double *s_r0, double *s_r1, int tid) {   // levels 5..11 from the root's s_r0[0], s_r1[0]
    sub_reach_level<4>(s_sig, s_r0, s_r1, tid); sub_reach_level<5>(s_sig, s_r0, s_r1, tid); sub_reach_level<6>(s_sig, s_r0, s_r1, tid); sub_reach_level<7>(s_sig, s_r0, s_r1, tid);
    sub_reach_level<8>(s_sig, s_r0, s_r1, tid); sub_reach_level<9>(s_sig, s_r0, s_r1, tid); sub_reach_level<10>(s_sig, s_r0, s_r1, tid);
}

// reaches of depths 1..3 from s_r0[0] = s_r1[0] = 1.0 (set before the caller's last barrier), the 85 top rows' sigma in LDS
__device__ __forceinline__ void top_reach_pass(const double *s_sig, double *s_r0, double *s_r1, int tid) {
#pragma unroll
    for (int d = 0; d < kCutDepth - 1; d++) {
        for (int j = tid; j < t_width(d + 1); j += kSubThreads) {
            const int par = j >> 2, a = j & 3;
            const double sg = s_sig[(t_offset(d) + par) * 4 + a], a0 = s_r0[t_offset(d) + par], a1 = s_r1[t_offset(d) + par];
            s_r0[t_offset(d + 1) + j] = t_team(d) == 0 ? a0 * sg : a0;
            s_r1[t_offset(d + 1) + j] = t_team(d) == 1 ? a1 * sg : a1;
        }
        __syncthreads();
    }
}

// ---- the value pass: one upward sweep with a mode per team ------------------------------------------------------------------------------
// kFollow: the team plays its table's rows as given, v = 0.0; v += row[c] * child[c], children left to right; kUniform: the same with 1 / b in
// every legal slot; kMaximise: the team takes the child that is best for ITSELF, a strict `>` from action 0 on (ties to the lowest action).
// Values are those of team `persp`: the terminals' 0.5 * r2, negated for team 1.  With one node per infoset a best response needs no reach
// weighting: the per-node maximum is the best response at every node, reachable or not.  g_out (or NULL) receives the table that was played:
// one-hot rows where a team maximised, the followed rows elsewhere.  `row` is the row of the tables that the node reads and writes.
enum { kFollow = 0, kUniform = 1, kMaximise = 2 };
struct TeamPlay { const double *tab[2]; int mode[2]; int persp; };

template <int B>
__device__ __forceinline__ double value_node(const double *u, int team, const TeamPlay &pl, size_t row, double *g_out) {
    const int mode = team == 0 ? pl.mode[0] : pl.mode[1];
    Row4 r = {{0.0, 0.0, 0.0, 0.0}};
    double v;
    if (mode == kMaximise) {
        const bool own = team == pl.persp;
        int best = 0;
        double vb = u[0];
#pragma unroll
        for (int c = 1; c < B; c++) {
            const bool better = own ? u[c] > vb : -u[c] > -vb;
            best = better ? c : best;
            vb = better ? u[c] : vb;
        }
#pragma unroll
        for (int c = 0; c < B; c++) r.x[c] = c == best ? 1.0 : 0.0;
        v = vb;
    } else {
        if (mode == kFollow) {
            r = load_row((team == 0 ? pl.tab[0] : pl.tab[1]) + row * 4);
#pragma unroll
            for (int c = B; c < 4; c++) r.x[c] = 0.0;   // the padding is not part of the row
        } else {
#pragma unroll
            for (int c = 0; c < B; c++) r.x[c] = 1.0 / (double)B;
        }
        v = 0.0;
#pragma unroll
        for (int c = 0; c < B; c++) v += r.x[c] * u[c];
    }
    if (g_out) store_row(g_out + row * 4, r);
    return v;
}

// ---- the walk from a deal's root ------------------------------------------------------------------------------------------------------------
// `plies` steps from the root on the state's ten words: the first `depth` (<= 12) follow the digits of idx, the index of a node within level
// `depth` (mixed radix, first ply most significant); later plies play the first card of the hand (the forced plies 12..15 have one).
__device__ __forceinline__ void team_walk(uint32_t (&w)[10], int depth, int idx, int plies) {
    int rem = idx, span = 1;
    for (int k = 0; k < depth; k++) span *= t_branch(k);
#pragma unroll 1
    for (int ply = 0; ply < plies; ply++) {
        int k = 0;
        if (ply < depth) {
            span /= t_branch(ply);               // nodes of level `depth` below one child of this ply's node
            k = rem / span;
            rem -= k * span;
        }
        const uint32_t seat = (uint32_t)ply & 3u;
        const uint32_t hand = (((seat & 2u) ? w[4] : w[3]) >> (16u * (seat & 1u))) & 0xFFFFu;
        scopa_team::step_words(w, scopa::nib(hand, k));
    }
}

// the payoff of depth-12 node i of the deal: its four forced plies played out, reward x2 of team 0
__device__ __forceinline__ int team_leaf_r2(const scopa_team_state &root, int i) {
    uint32_t w[10];
    memcpy(w, &root, 40);
    team_walk(w, 12, i, scopa_team::kPlies);
    scopa_team_state s;
    memcpy(&s, w, 40);
    return scopa_team::r2_team0_of(s);
}

// InfoNode.policy (vanilla_cfr.py:32-39) of a row with b legal slots: the strategy sums normalised, np.sum left to right; uniform where the sum is not > 0
__device__ __forceinline__ Row4 average_row(const Row4 &S, int b) {
    double s = S.x[0];
#pragma unroll
    for (int c = 1; c < 4; c++) if (c < b) s += S.x[c];
    Row4 r;
#pragma unroll
    for (int c = 0; c < 4; c++) r.x[c] = c < b ? (s > 0.0 ? S.x[c] / s : 1.0 / (double)b) : 0.0;
    return r;
}

}  // namespace
