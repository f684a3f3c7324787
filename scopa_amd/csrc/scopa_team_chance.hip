// scopa_team_chance.hip -- Team MiniScopa TPI over a SET of deals with the deal as a chance move.
//
// On one deal (scopa_team_cfr.hip) the information-state string ends in the whole action history, every node is its own infoset and the game is
// one of perfect information.  What makes the team game a game is that a seat sees neither its partner's hand nor its opponents': chance picks
// one of n deals uniformly, and a team's rows are shared between all deals the acting seat cannot tell apart.
//
//   key (64 bits) of a choice node (depths 0..11): bits 60-63 the depth; bits 44-59 the acting seat's INITIAL hand as scopa_team_state.hand holds
//       it (nibble i = hand position i); bits 0-43 the card ids played so far, nibble i = ply i.  The table is empty at the deal, so the table and
//       everyone's remaining cards follow from that history: this is the partition of the reference's information_state_string
//       (openspiel_team_mini_scopa.py:138-168) with ONE refinement, the one MiniScopa's ordered key makes -- the hand is kept in hand order, not
//       sorted.  Two occurrences of a key therefore have the same legal slots in the same order and a row's slot c means the same card everywhere;
//       a deal set whose seats' hands are stored ascending makes equal hand sets share rows.  The depth fixes the team ((d & 3) >> 1) and the
//       legal count (4 - (d >> 2)).  Forced plies (depths 12..15) have one action and no row; there is no leaf_reach_sum.
//   index (create): keys on the device, one lane per (deal, row) walking the row's path digits from the deal's root (team_walk); sorted on the
//       host; global id = rank among the distinct keys, so the ids of one depth are contiguous.  map[n][321365] local row -> global id, a CSR list
//       of occurrences deal * 321365 + row per global id in ascending (deal, row) order, the depth-12 payoffs r2[n][331776].
//   k_team_chance_sub (grid 256 x n)  k_team_cfr_sub's cut, one workgroup per (deal, depth-4 subtree): the subtree's 1 255 sigma rows gathered into
//       LDS through the deal's map row (the same 80 648-byte layout), reaches from the four ancestor rows, values up with cfr_node's arithmetic.  It
//       updates nothing: a traverser's row writes the 64-byte increment row {opp * (u[c] - v), reach * ls[c]} into the deal's slot of the image
//       [n][321365][8].  The other team's rows are neither written nor read later.
//   k_team_chance_top (grid n)  depths 3..0 of each deal from its 256 subtree values, the same increments, the deal's root value.
//   k_team_chance_reduce  one lane per global row of the traverser's team: the row's cells added over its occurrences in CSR order STARTING FROM
//       THE FIRST occurrence's value, then R <- R + dR; R <- !(R <= 0) ? R * pos : R * neg; S <- (S + dS) * strat and the row's sigma by regret
//       matching.  Lane 0 also leaves (v_deal0 + v_deal1 + ...) / n where the call asked for root values.  The common factor 1/n is left out of the
//       tables (it cancels in regret matching and in the average policy).
//   deal-sampled iterations (scopa_team_chance_cfr_iterate_sampled): the caller lists m of the n deals per iteration.  k_team_chance_sub (grid
//       256 x m) and k_team_chance_top (grid m) take the deal from the list and write its own slot of the image; k_team_chance_mark (one workgroup)
//       fills a table [n] from the list ahead of them; k_team_chance_reduce_sampled asks the table for every occurrence's deal, loads the rows of
//       listed occurrences only and sums them in the same CSR order from the first listed one, +0.0 where a row has none.  Every row of the updated
//       team(s) is then updated and discounted as above.  Simultaneous updates: both traversers' sweeps against the same sigma rows (their image
//       rows are disjoint), one reduce over the rows of both teams.
//   No float64 atomics, one writer per row, every sum in a fixed order: runs are bit-identical, and one deal gives scopa_team_cfr_iterate's bits.
//
// Traffic of a traversal: the traverser's increment rows written once and read once (4.0 / 16.5 MB per deal for traverser 0 / 1), the sigma rows gathered once per deal.  Rows move
// as 32-byte vectors (two per increment row).
//
// Best response across deals.  The per-node maximum is no best response here: a responder's row is shared by nodes in several deals.  Level by
// level from depth 11 up, per responder p: a lane per (deal, node) writes q[c] = opp_reach(node) * val(child c) into the image, a lane per global
// row of that depth adds q over the occurrences in CSR order from the first and takes the first slot that is best by a strict `>`, and the
// level's values are val(child[choice]); the other team's levels follow the policy with value_node's arithmetic.  A sequence of launches, lane per
// node, no host round trip: an evaluation pass, not the throughput path.
#include <algorithm>
#include <new>
#include <vector>

#include "scopa_team_chance.h"
#include "scopa_team_passes.h"

using scopa::fail;

namespace {

// ---- the index -----------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_team_chance_keys(const scopa_team_state *__restrict__ g_roots, uint64_t *__restrict__ g_keys, long long total) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int deal = (int)(i / kTChoice), row = (int)(i - (long long)deal * kTChoice);
    const int d = depth_of_row(row);
    const scopa_team_state root = g_roots[deal];
    uint32_t w[10];
    memcpy(w, &root, 40);
    team_walk(w, d, row - t_offset(d), d);
    const uint32_t seat = (uint32_t)d & 3u;
    const uint32_t hand = (uint32_t)((seat & 2u) ? (seat & 1u ? root.hand[3] : root.hand[2]) : (seat & 1u ? root.hand[1] : root.hand[0]));
    g_keys[i] = ((uint64_t)d << 60) | ((uint64_t)hand << 44) | (((uint64_t)w[1] << 32) | (uint64_t)w[0]);
}

__global__ void __launch_bounds__(256)
k_team_chance_leaves(const scopa_team_state *__restrict__ g_roots, int8_t *__restrict__ g_r2, long long total) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int deal = (int)(i / kTLeaves);
    g_r2[i] = (int8_t)team_leaf_r2(g_roots[deal], (int)(i - (long long)deal * kTLeaves));
}

// sigma of every global row from its regrets (after create, a reset or a tables_set; the reduce keeps it current afterwards)
__global__ void __launch_bounds__(256)
k_team_chance_sigma(const uint64_t *__restrict__ g_key, const double *__restrict__ g_R, double *__restrict__ g_sig, long long G) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    const Row4 R = load_row(g_R + g * 4);
    Row4 L = {{0.0, 0.0, 0.0, 0.0}};
    scopa::regret_match_n(t_branch(key_depth(g_key[g])), R.x, L.x);
    store_row(g_sig + g * 4, L);
}

// ---- the sweep -------------------------------------------------------------------------------------------------------------------------------
// a traverser's node leaves its increments in the deal's slot of the image, two 32-byte stores; the padding cells are written as 0
template <int B>
__device__ __forceinline__ void write_increments(const double *u, const double *ls, double v, double r0, double r1, int trav, double *g_row) {
    double dR[B], dS[B];
    cfr_increments<B>(u, ls, v, trav == 0 ? r0 : r1, trav == 0 ? r1 : r0, dR, dS);
    Row4 a = {{0.0, 0.0, 0.0, 0.0}}, b = {{0.0, 0.0, 0.0, 0.0}};
#pragma unroll
    for (int c = 0; c < B; c++) { a.x[c] = dR[c]; b.x[c] = dS[c]; }
    store_row(g_row, a);
    store_row(g_row + 4, b);
}

template <int D>
__device__ __forceinline__ void sub_increment_level(int g, int trav, const double *s_sig, const double *s_r0, const double *s_r1, double *s_val, double *g_img /* the deal's */,
                                                    int tid) {
    constexpr int b = t_branch(D), w = s_width(D), lo = s_offset(D), lo1 = s_offset(D + 1);
    for (int j = tid; j < w; j += kSubThreads) {
        double u[b], ls[b];
#pragma unroll
        for (int c = 0; c < b; c++) { u[c] = s_val[lo1 + j * b + c]; ls[c] = s_sig[(lo + j) * 4 + c]; }
        const double v = cfr_value<b>(u, ls);
        if (t_team(D) == trav) write_increments<b>(u, ls, v, s_r0[lo + j], s_r1[lo + j], trav, g_img + ((size_t)t_offset(D) + (size_t)g * w + j) * 8);
        s_val[lo + j] = v;
    }
    __syncthreads();
}

__global__ void __launch_bounds__(kSubThreads)
k_team_chance_sub(const double *__restrict__ g_sig, const int32_t *__restrict__ g_map, const int8_t *__restrict__ g_r2, double *__restrict__ g_img,
                  double *__restrict__ g_sub /*[n][256]*/, int trav, const int32_t *__restrict__ g_list /* the iteration's deals, or NULL = every deal */) {
    extern __shared__ double s_team_chance[];
    double *s_sig = s_team_chance, *s_r0 = s_sig + kSubRows * 4, *s_r1 = s_r0 + kSubRows, *s_val = s_r1 + kSubRows;
    const int g = blockIdx.x, deal = g_list ? g_list[blockIdx.y] : (int)blockIdx.y, tid = threadIdx.x;
    const int32_t *map = g_map + (size_t)deal * kTChoice;
    // the subtree's rows of level d are consecutive in the level-major order; each comes from the shared row of its key, one 32-byte load
#pragma unroll
    for (int d = kCutDepth; d < 12; d++)
        for (int k = tid; k < s_width(d); k += kSubThreads) {
            const Row4 r = load_row(g_sig + (size_t)map[t_offset(d) + g * s_width(d) + k] * 4);
#pragma unroll
            for (int c = 0; c < 4; c++) s_sig[(s_offset(d) + k) * 4 + c] = r.x[c];
        }
    if (tid == 0) sub_root_reaches(g, g_sig, [map](int row) { return map[row]; }, s_r0[0], s_r1[0]);
    __syncthreads();
    sub_reach_pass(s_sig, s_r0, s_r1, tid);
    for (int j = tid; j < kSubLeaves; j += kSubThreads) s_val[kSubRows + j] = leaf_value(g_r2[(size_t)deal * kTLeaves + (size_t)g * kSubLeaves + j], trav);
    __syncthreads();
    double *img = g_img + (size_t)deal * kTChoice * 8;
#define SC_TEAM_UP(D) sub_increment_level<D>(g, trav, s_sig, s_r0, s_r1, s_val, img, tid)
    SC_TEAM_UP(11); SC_TEAM_UP(10); SC_TEAM_UP(9); SC_TEAM_UP(8); SC_TEAM_UP(7); SC_TEAM_UP(6); SC_TEAM_UP(5); SC_TEAM_UP(4);
#undef SC_TEAM_UP
    if (tid == 0) g_sub[(size_t)deal * kSubtrees + g] = s_val[0];
}

__global__ void __launch_bounds__(kSubThreads)
k_team_chance_top(const double *__restrict__ g_sig, const int32_t *__restrict__ g_map, double *__restrict__ g_img, const double *__restrict__ g_sub,
                  double *__restrict__ g_rootdeal /*[n]*/, int trav, const int32_t *__restrict__ g_list /* as k_team_chance_sub's */) {
    __shared__ double s_sig[kTopRows * 4], s_r0[kTopRows], s_r1[kTopRows], s_val[kTopRows + kSubtrees];
    const int deal = g_list ? g_list[blockIdx.x] : (int)blockIdx.x, tid = threadIdx.x;
    const int32_t *map = g_map + (size_t)deal * kTChoice;
    for (int k = tid; k < kTopRows; k += kSubThreads) {
        const Row4 r = load_row(g_sig + (size_t)map[k] * 4);
#pragma unroll
        for (int c = 0; c < 4; c++) s_sig[k * 4 + c] = r.x[c];
    }
    for (int k = tid; k < kSubtrees; k += kSubThreads) s_val[kTopRows + k] = g_sub[(size_t)deal * kSubtrees + k];
    if (tid == 0) { s_r0[0] = 1.0; s_r1[0] = 1.0; }
    __syncthreads();
    top_reach_pass(s_sig, s_r0, s_r1, tid);
    double *img = g_img + (size_t)deal * kTChoice * 8;
#pragma unroll
    for (int d = kCutDepth - 1; d >= 0; d--) {
        for (int j = tid; j < t_width(d); j += kSubThreads) {
            const int row = t_offset(d) + j;
            double u[4], ls[4];
#pragma unroll
            for (int c = 0; c < 4; c++) { u[c] = s_val[t_offset(d + 1) + j * 4 + c]; ls[c] = s_sig[row * 4 + c]; }
            const double v = cfr_value<4>(u, ls);
            if (t_team(d) == trav) write_increments<4>(u, ls, v, s_r0[row], s_r1[row], trav, img + (size_t)row * 8);
            s_val[row] = v;
        }
        __syncthreads();
    }
    if (tid == 0) g_rootdeal[deal] = s_val[0];
}

template <int B>
__device__ __forceinline__ void reduce_apply(long long g, const Row4 &dR, const Row4 &dS, double *g_R, double *g_S, double *g_sig, double wpos, double wneg, double wstrat) {
    Row4 R = load_row(g_R + g * 4), S = load_row(g_S + g * 4);
    cfr_apply<B>(R, S, dR.x, dS.x, wpos, wneg, wstrat);
    store_row(g_R + g * 4, R);
    store_row(g_S + g * 4, S);
    Row4 L = {{0.0, 0.0, 0.0, 0.0}};
    scopa::regret_match<B>(R.x, L.x);
    store_row(g_sig + g * 4, L);
}

__global__ void __launch_bounds__(256)
k_team_chance_reduce(const uint64_t *__restrict__ g_key, const int32_t *__restrict__ g_occ_off, const int32_t *__restrict__ g_occ, const double *__restrict__ g_img,
                     double *__restrict__ g_R, double *__restrict__ g_S, double *__restrict__ g_sig, long long G, int trav, double wpos, double wneg, double wstrat,
                     const double *__restrict__ g_rootdeal, int n, double *__restrict__ g_root /* one value, or NULL */) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g == 0 && g_root) {
        double s = g_rootdeal[0];
        for (int i = 1; i < n; i++) s += g_rootdeal[i];
        g_root[0] = s / (double)n;
    }
    if (g >= G) return;
    const int d = key_depth(g_key[g]);
    if (t_team(d) != trav) return;
    const int o = g_occ_off[g], e = g_occ_off[g + 1];
    Row4 dR = load_row(g_img + (size_t)g_occ[o] * 8), dS = load_row(g_img + (size_t)g_occ[o] * 8 + 4);
    for (int i = o + 1; i < e; i++) {
        const Row4 a = load_row(g_img + (size_t)g_occ[i] * 8), b = load_row(g_img + (size_t)g_occ[i] * 8 + 4);
#pragma unroll
        for (int c = 0; c < 4; c++) { dR.x[c] += a.x[c]; dS.x[c] += b.x[c]; }
    }
    const int b = t_branch(d);
    if (b == 4) reduce_apply<4>(g, dR, dS, g_R, g_S, g_sig, wpos, wneg, wstrat);
    else if (b == 3) reduce_apply<3>(g, dR, dS, g_R, g_S, g_sig, wpos, wneg, wstrat);
    else reduce_apply<2>(g, dR, dS, g_R, g_S, g_sig, wpos, wneg, wstrat);
}

// ---- deal-sampled iterations ------------------------------------------------------------------------------------------------------------------
// the iteration's table [n]: 1 where the deal is in its list.  One workgroup, ahead of the iteration's sweeps on the same stream (n <= 1 670)
__global__ void __launch_bounds__(256)
k_team_chance_mark(const int32_t *__restrict__ g_list, int m, int32_t *__restrict__ g_mark, int n) {
    for (int i = threadIdx.x; i < n; i += 256) g_mark[i] = 0;
    __syncthreads();
    for (int k = threadIdx.x; k < m; k += 256) g_mark[g_list[k]] = 1;   // distinct ids in [0, n): checked on the host
}

// (v_a + v_b + ...) / m over the listed deals in ascending deal id, from the first listed one's value
__device__ __forceinline__ double sampled_root(const double *g_rootdeal, const int32_t *g_mark, int n, int m) {
    double s = 0.0;
    bool any = false;
    for (int i = 0; i < n; i++) {
        if (g_mark && !g_mark[i]) continue;
        const double v = g_rootdeal[i];
        s = any ? s + v : v;
        any = true;
    }
    return s / (double)m;
}

// k_team_chance_reduce over the LISTED occurrences only: an occurrence counts when its deal is marked (g_mark NULL: every deal is), and only then
// is its image row loaded.  Same CSR order, from the first listed occurrence's value; a row with none takes +0.0 for both sums and is updated like
// every other row.  trav -1: the rows of both teams (a simultaneous iteration: the two sweeps wrote disjoint rows), root values from both arrays.
__global__ void __launch_bounds__(256)
k_team_chance_reduce_sampled(const uint64_t *__restrict__ g_key, const int32_t *__restrict__ g_occ_off, const int32_t *__restrict__ g_occ, const double *__restrict__ g_img,
                             const int32_t *__restrict__ g_mark /*[n] or NULL*/, double *__restrict__ g_R, double *__restrict__ g_S, double *__restrict__ g_sig, long long G,
                             int trav, double wpos, double wneg, double wstrat, const double *__restrict__ g_rootdeal0, const double *__restrict__ g_rootdeal1, int n, int m,
                             double *__restrict__ g_root /* the iteration's two values, or NULL */) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g == 0 && g_root) {
        if (trav != 1) g_root[0] = sampled_root(g_rootdeal0, g_mark, n, m);
        if (trav != 0) g_root[1] = sampled_root(g_rootdeal1, g_mark, n, m);
    }
    if (g >= G) return;
    const int d = key_depth(g_key[g]);
    if (trav >= 0 && t_team(d) != trav) return;
    const int o = g_occ_off[g], e = g_occ_off[g + 1];
    Row4 dR = {{0.0, 0.0, 0.0, 0.0}}, dS = {{0.0, 0.0, 0.0, 0.0}};
    bool any = false;
    for (int i = o; i < e; i++) {
        const int oc = g_occ[i];
        if (g_mark && !g_mark[oc / kTChoice]) continue;
        const Row4 a = load_row(g_img + (size_t)oc * 8), b = load_row(g_img + (size_t)oc * 8 + 4);
#pragma unroll
        for (int c = 0; c < 4; c++) { dR.x[c] = any ? dR.x[c] + a.x[c] : a.x[c]; dS.x[c] = any ? dS.x[c] + b.x[c] : b.x[c]; }
        any = true;
    }
    const int b = t_branch(d);
    if (b == 4) reduce_apply<4>(g, dR, dS, g_R, g_S, g_sig, wpos, wneg, wstrat);
    else if (b == 3) reduce_apply<3>(g, dR, dS, g_R, g_S, g_sig, wpos, wneg, wstrat);
    else reduce_apply<2>(g, dR, dS, g_R, g_S, g_sig, wpos, wneg, wstrat);
}

// ---- exploitability across deals --------------------------------------------------------------------------------------------------------------
// the evaluated policy: a caller's table as given, or the average of the strategy table by k_team_average_policy's rule
__global__ void __launch_bounds__(256)
k_team_chance_policy(const uint64_t *__restrict__ g_key, const double *__restrict__ g_S, const double *__restrict__ g_pin, double *__restrict__ g_pol, long long G) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    store_row(g_pol + g * 4, g_pin ? load_row(g_pin + g * 4) : average_row(load_row(g_S + g * 4), t_branch(key_depth(g_key[g]))));
}

// the product of the policy's probabilities of the team that is NOT the responder along every node's path, as a running product from the root
__global__ void __launch_bounds__(256)
k_team_chance_opp_reach(const int32_t *__restrict__ g_map, const double *__restrict__ g_pol, double *__restrict__ g_reach, long long total, int responder) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int deal = (int)(i / kTChoice), row = (int)(i - (long long)deal * kTChoice);
    const int32_t *map = g_map + (size_t)deal * kTChoice;
    const int d = depth_of_row(row);
    int rem = row - t_offset(d), span = 1, anc = 0;
    for (int k = 0; k < d; k++) span *= t_branch(k);
    double r = 1.0;
    for (int k = 0; k < d; k++) {
        span /= t_branch(k);
        const int a = rem / span;
        rem -= a * span;
        if (t_team(k) != responder) r = r * g_pol[(size_t)map[t_offset(k) + anc] * 4 + a];
        anc = anc * t_branch(k) + a;
    }
    g_reach[(size_t)deal * kTNodes + row] = r;
}

__global__ void __launch_bounds__(256)
k_team_chance_leaf_values(const int8_t *__restrict__ g_r2, double *__restrict__ g_val, long long total, int persp) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int deal = (int)(i / kTLeaves);
    g_val[(size_t)deal * kTNodes + kTChoice + (size_t)(i - (long long)deal * kTLeaves)] = leaf_value(g_r2[i], persp);
}

// one level of a pass, a lane per (deal, node).  kLevelQ: the responder's level, q rows into the image; kLevelSelect: its values from the choices;
// kLevelFollow: the level follows the policy (value_node, kFollow).  The depth-12 values lie behind the rows: child ids need no case.
enum { kLevelQ = 0, kLevelSelect = 1, kLevelFollow = 2 };

template <int B>
__device__ __forceinline__ void level_node(int what, int d, int gid, size_t node, const double *u, const double *g_pol, const double *g_reach, double *g_val,
                                           double *g_q, const int32_t *g_choice) {
    if (what == kLevelQ) {
        const double opp = g_reach[node];
        Row4 q = {{0.0, 0.0, 0.0, 0.0}};
#pragma unroll
        for (int c = 0; c < B; c++) q.x[c] = opp * u[c];
        store_row(g_q, q);
    } else if (what == kLevelSelect) {
        const int ch = g_choice[gid];
        double v = u[0];
#pragma unroll
        for (int c = 1; c < B; c++) v = ch == c ? u[c] : v;
        g_val[node] = v;
    } else {
        TeamPlay pl;
        pl.tab[0] = pl.tab[1] = g_pol;
        pl.mode[0] = pl.mode[1] = kFollow;
        pl.persp = 0;
        g_val[node] = value_node<B>(u, t_team(d), pl, (size_t)gid, nullptr);
    }
}

__global__ void __launch_bounds__(256)
k_team_chance_level(int what, int d, const int32_t *__restrict__ g_map, const double *__restrict__ g_pol, const double *__restrict__ g_reach, double *g_val,
                    double *__restrict__ g_img, const int32_t *__restrict__ g_choice, int n) {
    const int w = t_width(d), b = t_branch(d);
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)n * w) return;
    const int deal = (int)(i / w), j = (int)(i - (long long)deal * w), row = t_offset(d) + j;
    const size_t base = (size_t)deal * kTNodes;
    const double *child = g_val + base + t_offset(d + 1) + (size_t)j * b;
    double u[4] = {0.0, 0.0, 0.0, 0.0};
    for (int c = 0; c < b; c++) u[c] = child[c];
    const int gid = g_map[(size_t)deal * kTChoice + row];
    double *q = g_img + ((size_t)deal * kTChoice + row) * 8;
    if (b == 4) level_node<4>(what, d, gid, base + row, u, g_pol, g_reach, g_val, q, g_choice);
    else if (b == 3) level_node<3>(what, d, gid, base + row, u, g_pol, g_reach, g_val, q, g_choice);
    else level_node<2>(what, d, gid, base + row, u, g_pol, g_reach, g_val, q, g_choice);
}

// the responder's slot at every global row of one depth: q added over the occurrences in CSR order from the first, the first slot that is best by
// a strict `>` (ties to the lowest slot; an all-zero row takes slot 0)
__global__ void __launch_bounds__(256)
k_team_chance_choose(long long lo, long long hi, int b, const int32_t *__restrict__ g_occ_off, const int32_t *__restrict__ g_occ, const double *__restrict__ g_img,
                     int32_t *__restrict__ g_choice) {
    const long long g = lo + (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= hi) return;
    const int o = g_occ_off[g], e = g_occ_off[g + 1];
    Row4 q = load_row(g_img + (size_t)g_occ[o] * 8);
    for (int i = o + 1; i < e; i++) {
        const Row4 a = load_row(g_img + (size_t)g_occ[i] * 8);
#pragma unroll
        for (int c = 0; c < 4; c++) q.x[c] += a.x[c];
    }
    int best = 0;
    double vb = q.x[0];
#pragma unroll
    for (int c = 1; c < 4; c++) {
        const bool better = c < b && q.x[c] > vb;
        best = better ? c : best;
        vb = better ? q.x[c] : vb;
    }
    g_choice[g] = best;
}

// a complete table of the responder: its rows one-hot at the choice, the other team's rows the policy's
__global__ void __launch_bounds__(256)
k_team_chance_br_table(const uint64_t *__restrict__ g_key, const double *__restrict__ g_pol, const int32_t *__restrict__ g_choice, double *__restrict__ g_br, long long G,
                       int responder) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    Row4 r = load_row(g_pol + g * 4);
    if (t_team(key_depth(g_key[g])) == responder) {
        const int ch = g_choice[g];
#pragma unroll
        for (int c = 0; c < 4; c++) r.x[c] = c == ch ? 1.0 : 0.0;
    }
    store_row(g_br + g * 4, r);
}

__global__ void __launch_bounds__(256)
k_team_chance_roots(const double *__restrict__ g_val, double *__restrict__ g_out, int n) {
    const int deal = blockIdx.x * blockDim.x + threadIdx.x;
    if (deal < n) g_out[deal] = g_val[(size_t)deal * kTNodes];
}

__global__ void __launch_bounds__(256)
k_team_chance_scatter(const int32_t *__restrict__ g_map /* the deal's */, const double *__restrict__ g_pol, double *__restrict__ g_local) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row < kTChoice) store_row(g_local + (size_t)row * 4, load_row(g_pol + (size_t)g_map[row] * 4));
}

unsigned blocks_of(long long lanes) { return (unsigned)((lanes + 255) / 256); }

int32_t tc_sigma(scopa_team_chance *g) {
    hipLaunchKernelGGL(k_team_chance_sigma, dim3(blocks_of(g->G)), dim3(256), 0, g->ctx->stream, (const uint64_t *)g->d_gkey, (const double *)g->d_R, g->d_sig, g->G);
    SC_HIP(g->ctx, hipGetLastError());
    return SCOPA_OK;
}

// every list of a sampled call holds m distinct ids in [0, n)
bool cs_lists_ok(int n, int32_t n_lists, int32_t m, const int32_t *h_deals) {
    std::vector<int32_t> seen((size_t)n, -1);
    for (int32_t it = 0; it < n_lists; it++)
        for (int32_t k = 0; k < m; k++) {
            const int32_t d = h_deals[(size_t)it * m + k];
            if (d < 0 || d >= n || seen[(size_t)d] == it) return false;
            seen[(size_t)d] = it;
        }
    return true;
}

// the mark table and traverser 1's per-deal root values at the first sampled call; the call's deal lists, once, into g->d_cs_list (grown as needed:
// n_iters * m ids).  Synchronises the stream after the upload: the caller's rows are only borrowed
int32_t cs_upload_lists(scopa_team_chance *g, size_t n_ids, const int32_t *h_deals) {
    scopa_ctx *ctx = g->ctx;
    if (!g->d_cs_mark) {
        const bool ok = hipMalloc(&g->d_cs_mark, (size_t)g->n * 4) == hipSuccess && hipMalloc(&g->d_cs_root, (size_t)g->n * 8) == hipSuccess;
        if (!ok) {
            if (g->d_cs_mark) (void)hipFree(g->d_cs_mark);
            g->d_cs_mark = nullptr; g->d_cs_root = nullptr;
            return fail(ctx, SCOPA_ENOMEM, "scopa_team_chance_cfr_iterate_sampled: no device memory for the mark table");
        }
    }
    if (!h_deals) return SCOPA_OK;
    if (n_ids > g->cs_list_cap) {
        SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (g->d_cs_list) { (void)hipFree(g->d_cs_list); g->d_cs_list = nullptr; g->cs_list_cap = 0; }
        if (hipMalloc(&g->d_cs_list, n_ids * 4) != hipSuccess) { g->d_cs_list = nullptr; return fail(ctx, SCOPA_ENOMEM, "scopa_team_chance_cfr_iterate_sampled: no device memory for the lists"); }
        g->cs_list_cap = n_ids;
    }
    SC_HIP(ctx, hipMemcpyAsync(g->d_cs_list, h_deals, n_ids * 4, hipMemcpyHostToDevice, ctx->stream));
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SCOPA_OK;
}

}  // namespace

extern "C" {

int32_t scopa_team_chance_destroy(scopa_team_chance *g) {
    if (!g) return SCOPA_EINVAL;
    (void)hipSetDevice(g->ctx->device);
    (void)hipStreamSynchronize(g->ctx->stream);
    void *bufs[] = {g->d_gkey, g->d_map, g->d_occ_off, g->d_occ, g->d_r2, g->d_R, g->d_S, g->d_sig, g->d_img, g->d_sub, g->d_rootdeal, g->d_root,
                    g->d_reach, g->d_val, g->d_pol, g->d_choice, g->d_vals, g->d_mc_delta, g->d_mc_list, g->d_cs_list, g->d_cs_mark, g->d_cs_root};
    for (void *b : bufs) if (b) (void)hipFree(b);
    scopa::team_xplay_release(&g->xp);
    scopa::team_chance_sdcfr_release(g);
    delete g;
    return SCOPA_OK;
}

int32_t scopa_team_chance_debug_image_budget(scopa_ctx *ctx, int64_t bytes) {
    if (!ctx || bytes < 0) return SCOPA_EINVAL;
    ctx->team_chance_budget = bytes;
    return SCOPA_OK;
}

int32_t scopa_team_chance_create(scopa_ctx *ctx, int32_t n, const uint8_t *h_perms, scopa_team_chance **out) {
    if (!ctx || !out) return SCOPA_EINVAL;
    *out = nullptr;
    SC_REQUIRE(ctx, n >= 1 && h_perms, SCOPA_EINVAL, "scopa_team_chance_create: at least one deal is required");
    SC_REQUIRE(ctx, (long long)n * kTChoice < (1ll << 31), SCOPA_ELIMIT, "scopa_team_chance_create: n * 321365 must stay below 2^31");
    const long long budget = ctx->team_chance_budget > 0 ? ctx->team_chance_budget : kTeamChanceImageBudget;
    SC_REQUIRE(ctx, (long long)n * kTChoice * 64 <= budget, SCOPA_ELIMIT, "scopa_team_chance_create: the increment image exceeds its byte budget");
    std::vector<scopa_team_state> roots((size_t)n);
    for (int d = 0; d < n; d++)
        SC_REQUIRE(ctx, scopa_team_state_init(h_perms + (size_t)d * 16, &roots[(size_t)d]) == SCOPA_OK, SCOPA_EINVAL,
                   "scopa_team_chance_create: a perm16 is not a permutation of 0..15");
    SC_HIP(ctx, hipSetDevice(ctx->device));
    scopa_team_chance *g = new (std::nothrow) scopa_team_chance();
    if (!g) return fail(ctx, SCOPA_ENOMEM, "scopa_team_chance_create: out of host memory");
    g->ctx = ctx; g->n = n;
    g->h_roots = roots;
    const size_t rows = (size_t)n * kTChoice, leaves = (size_t)n * kTLeaves;
    g->n_occ = (long long)rows;

    // keys and payoffs on the device; the keys borrow the image, which is allocated first and zeroed afterwards
    scopa_team_state *d_roots = nullptr;
    bool ok = hipMalloc(&g->d_img, rows * 64) == hipSuccess && hipMalloc(&g->d_r2, leaves) == hipSuccess && hipMalloc(&d_roots, (size_t)n * sizeof(scopa_team_state)) == hipSuccess;
    if (!ok) { if (d_roots) (void)hipFree(d_roots); scopa_team_chance_destroy(g); return fail(ctx, SCOPA_ENOMEM, "scopa_team_chance_create: device allocation failed"); }
    std::vector<uint64_t> keys(rows);
    uint64_t *d_keys = reinterpret_cast<uint64_t *>(g->d_img);
    ok = hipMemcpyAsync(d_roots, roots.data(), (size_t)n * sizeof(scopa_team_state), hipMemcpyHostToDevice, ctx->stream) == hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(k_team_chance_keys, dim3(blocks_of((long long)rows)), dim3(256), 0, ctx->stream, (const scopa_team_state *)d_roots, d_keys, (long long)rows);
        hipLaunchKernelGGL(k_team_chance_leaves, dim3(blocks_of((long long)leaves)), dim3(256), 0, ctx->stream, (const scopa_team_state *)d_roots, g->d_r2, (long long)leaves);
        ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(keys.data(), d_keys, rows * 8, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess &&
             hipStreamSynchronize(ctx->stream) == hipSuccess;
    }
    (void)hipFree(d_roots);
    if (!ok) { scopa_team_chance_destroy(g); return fail(ctx, SCOPA_EHIP, "scopa_team_chance_create: building the keys failed"); }

    std::vector<uint64_t> &gk = g->h_gkey;
    gk = keys;
    std::sort(gk.begin(), gk.end());
    gk.erase(std::unique(gk.begin(), gk.end()), gk.end());
    g->G = (long long)gk.size();
    for (int d = 0; d <= 12; d++) g->depth_off[d] = (long long)(std::lower_bound(gk.begin(), gk.end(), (uint64_t)d << 60) - gk.begin());
    g->depth_off[12] = g->G;
    g->h_map.resize(rows);
    std::vector<int32_t> occ_off((size_t)g->G + 1, 0), occ(rows);
    for (size_t i = 0; i < rows; i++) {
        const int32_t gid = (int32_t)(std::lower_bound(gk.begin(), gk.end(), keys[i]) - gk.begin());
        g->h_map[i] = gid;
        occ_off[(size_t)gid + 1]++;
    }
    for (long long i = 0; i < g->G; i++) occ_off[(size_t)i + 1] += occ_off[(size_t)i];
    {
        std::vector<int32_t> at(occ_off.begin(), occ_off.end() - 1);
        for (size_t i = 0; i < rows; i++) occ[(size_t)at[(size_t)g->h_map[i]]++] = (int32_t)i;   // i = deal * 321365 + row, ascending
    }

    const size_t Gs = (size_t)g->G;
    ok = hipMalloc(&g->d_gkey, Gs * 8) == hipSuccess && hipMalloc(&g->d_map, rows * 4) == hipSuccess && hipMalloc(&g->d_occ_off, (Gs + 1) * 4) == hipSuccess &&
         hipMalloc(&g->d_occ, rows * 4) == hipSuccess && hipMalloc(&g->d_R, Gs * 32) == hipSuccess && hipMalloc(&g->d_S, Gs * 32) == hipSuccess &&
         hipMalloc(&g->d_sig, Gs * 32) == hipSuccess && hipMalloc(&g->d_sub, (size_t)n * kSubtrees * 8) == hipSuccess && hipMalloc(&g->d_rootdeal, (size_t)n * 8) == hipSuccess;
    if (!ok) { scopa_team_chance_destroy(g); return fail(ctx, SCOPA_ENOMEM, "scopa_team_chance_create: device allocation failed"); }
    ok = hipMemcpyAsync(g->d_gkey, gk.data(), Gs * 8, hipMemcpyHostToDevice, ctx->stream) == hipSuccess &&
         hipMemcpyAsync(g->d_map, g->h_map.data(), rows * 4, hipMemcpyHostToDevice, ctx->stream) == hipSuccess &&
         hipMemcpyAsync(g->d_occ_off, occ_off.data(), occ_off.size() * 4, hipMemcpyHostToDevice, ctx->stream) == hipSuccess &&
         hipMemcpyAsync(g->d_occ, occ.data(), rows * 4, hipMemcpyHostToDevice, ctx->stream) == hipSuccess &&
         hipMemsetAsync(g->d_img, 0, rows * 64, ctx->stream) == hipSuccess && hipMemsetAsync(g->d_R, 0, Gs * 32, ctx->stream) == hipSuccess &&
         hipMemsetAsync(g->d_S, 0, Gs * 32, ctx->stream) == hipSuccess && hipStreamSynchronize(ctx->stream) == hipSuccess;   // the host vectors go out of scope below
    if (!ok) { scopa_team_chance_destroy(g); return fail(ctx, SCOPA_EHIP, "scopa_team_chance_create: upload of the index failed"); }
    { const int32_t rc = tc_sigma(g); if (rc != SCOPA_OK) { scopa_team_chance_destroy(g); return rc; } }
    *out = g;
    return SCOPA_OK;
}

int32_t scopa_team_chance_counts(scopa_team_chance *g, int32_t *n_deals, int64_t *n_global, int64_t *n_occurrences) {
    if (!g) return SCOPA_EINVAL;
    if (n_deals) *n_deals = g->n;
    if (n_global) *n_global = g->G;
    if (n_occurrences) *n_occurrences = g->n_occ;
    return SCOPA_OK;
}

int32_t scopa_team_chance_index_get(scopa_team_chance *g, uint64_t *h_keys, int32_t *h_map) {
    if (!g) return SCOPA_EINVAL;
    if (h_keys) std::copy(g->h_gkey.begin(), g->h_gkey.end(), h_keys);
    if (h_map) std::copy(g->h_map.begin(), g->h_map.end(), h_map);
    return SCOPA_OK;
}

int32_t scopa_team_chance_tables_reset(scopa_team_chance *g) {
    if (!g) return SCOPA_EINVAL;
    scopa_ctx *ctx = g->ctx;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    SC_HIP(ctx, hipMemsetAsync(g->d_R, 0, (size_t)g->G * 32, ctx->stream));
    SC_HIP(ctx, hipMemsetAsync(g->d_S, 0, (size_t)g->G * 32, ctx->stream));
    if (g->d_mc_delta) SC_HIP(ctx, hipMemsetAsync(g->d_mc_delta, 0, (size_t)g->G * 40, ctx->stream));   // walks not yet applied go with the tables; the counters stay
    if (int32_t rc = tc_sigma(g)) return rc;
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SCOPA_OK;
}

int32_t scopa_team_chance_tables_get(scopa_team_chance *g, double *h_regret, double *h_strategy) {
    if (!g) return SCOPA_EINVAL;
    scopa_ctx *ctx = g->ctx;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    if (h_regret) SC_HIP(ctx, hipMemcpyAsync(h_regret, g->d_R, (size_t)g->G * 32, hipMemcpyDeviceToHost, ctx->stream));
    if (h_strategy) SC_HIP(ctx, hipMemcpyAsync(h_strategy, g->d_S, (size_t)g->G * 32, hipMemcpyDeviceToHost, ctx->stream));
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SCOPA_OK;
}

int32_t scopa_team_chance_sigma_get(scopa_team_chance *g, double *h_sigma) {
    if (!g || !h_sigma) return SCOPA_EINVAL;
    scopa_ctx *ctx = g->ctx;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    SC_HIP(ctx, hipMemcpyAsync(h_sigma, g->d_sig, (size_t)g->G * 32, hipMemcpyDeviceToHost, ctx->stream));
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SCOPA_OK;
}

int32_t scopa_team_chance_tables_set(scopa_team_chance *g, const double *h_regret, const double *h_strategy) {
    if (!g) return SCOPA_EINVAL;
    scopa_ctx *ctx = g->ctx;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    if (h_regret) SC_HIP(ctx, hipMemcpyAsync(g->d_R, h_regret, (size_t)g->G * 32, hipMemcpyHostToDevice, ctx->stream));
    if (h_strategy) SC_HIP(ctx, hipMemcpyAsync(g->d_S, h_strategy, (size_t)g->G * 32, hipMemcpyHostToDevice, ctx->stream));
    if (h_regret) { if (int32_t rc = tc_sigma(g)) return rc; }
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the host buffers are only borrowed for the call
    return SCOPA_OK;
}

int32_t scopa_team_chance_cfr_iterate(scopa_team_chance *g, int32_t n_iters, const double *h_w, double *h_root_values) {
    if (!g || n_iters < 0 || n_iters > (1 << 20)) return SCOPA_EINVAL;
    scopa_ctx *ctx = g->ctx;
    if (n_iters == 0) return SCOPA_OK;
    SC_REQUIRE(ctx, !h_w || scopa::cfr_weights_ok(h_w, n_iters), SCOPA_EINVAL, "scopa_team_chance_cfr_iterate: every weight must be finite and in [0, 1]");
    SC_HIP(ctx, hipSetDevice(ctx->device));
    if (h_root_values && g->root_cap < (size_t)n_iters * 2) {
        if (g->d_root) SC_HIP(ctx, hipFree(g->d_root));
        g->d_root = nullptr; g->root_cap = 0;
        SC_HIP(ctx, hipMalloc(&g->d_root, sizeof(double) * 2 * (size_t)n_iters));
        g->root_cap = (size_t)n_iters * 2;
    }
    SC_LDS_ATTR(ctx, scopa::kLdsTeamChance, k_team_chance_sub, (int)kSubLds);
    for (int32_t it = 0; it < n_iters; it++) {
        // the weights are launch arguments: (1, 1, 1) multiplies every cell by 1.0, which changes no bit
        const double wpos = h_w ? h_w[it * 3 + 0] : 1.0, wneg = h_w ? h_w[it * 3 + 1] : 1.0, wstrat = h_w ? h_w[it * 3 + 2] : 1.0;
        for (int p = 0; p < 2; p++) {   // for i in range(num_players): _cfr_recursive(root, i, 1.0, 1.0)  (vanilla_cfr.py:108-110)
            hipLaunchKernelGGL(k_team_chance_sub, dim3(kSubtrees, g->n), dim3(kSubThreads), kSubLds, ctx->stream, (const double *)g->d_sig, (const int32_t *)g->d_map,
                               (const int8_t *)g->d_r2, g->d_img, g->d_sub, p, (const int32_t *)nullptr);
            hipLaunchKernelGGL(k_team_chance_top, dim3(g->n), dim3(kSubThreads), 0, ctx->stream, (const double *)g->d_sig, (const int32_t *)g->d_map, g->d_img,
                               (const double *)g->d_sub, g->d_rootdeal, p, (const int32_t *)nullptr);
            hipLaunchKernelGGL(k_team_chance_reduce, dim3(blocks_of(g->G)), dim3(256), 0, ctx->stream, (const uint64_t *)g->d_gkey, (const int32_t *)g->d_occ_off,
                               (const int32_t *)g->d_occ, (const double *)g->d_img, g->d_R, g->d_S, g->d_sig, g->G, p, wpos, wneg, wstrat, (const double *)g->d_rootdeal, g->n,
                               h_root_values ? g->d_root + (size_t)it * 2 + p : (double *)nullptr);
            SC_HIP(ctx, hipGetLastError());
        }
    }
    if (h_root_values) {
        SC_HIP(ctx, hipMemcpyAsync(h_root_values, g->d_root, sizeof(double) * 2 * (size_t)n_iters, hipMemcpyDeviceToHost, ctx->stream));
        SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return SCOPA_OK;
}

int32_t scopa_team_chance_cfr_iterate_sampled(scopa_team_chance *g, int32_t n_iters, int32_t m, const int32_t *h_deals, const double *h_w, int32_t alternating,
                                              double *h_root_values) {
    if (!g || n_iters < 0 || n_iters > (1 << 20) || (alternating != 0 && alternating != 1)) return SCOPA_EINVAL;
    scopa_ctx *ctx = g->ctx;
    if (n_iters == 0) return SCOPA_OK;
    SC_REQUIRE(ctx, !h_w || scopa::cfr_weights_ok(h_w, n_iters), SCOPA_EINVAL, "scopa_team_chance_cfr_iterate_sampled: every weight must be finite and in [0, 1]");
    SC_REQUIRE(ctx, !h_deals || (m >= 1 && m <= g->n && cs_lists_ok(g->n, n_iters, m, h_deals)), SCOPA_EINVAL,
               "scopa_team_chance_cfr_iterate_sampled: every list must hold 1 <= m <= n distinct deal ids in [0, n)");
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const int slots = h_deals ? m : g->n;
    if (int32_t rc = cs_upload_lists(g, (size_t)n_iters * (size_t)slots, h_deals)) return rc;   // once per call
    if (h_root_values && g->root_cap < (size_t)n_iters * 2) {
        if (g->d_root) SC_HIP(ctx, hipFree(g->d_root));
        g->d_root = nullptr; g->root_cap = 0;
        SC_HIP(ctx, hipMalloc(&g->d_root, sizeof(double) * 2 * (size_t)n_iters));
        g->root_cap = (size_t)n_iters * 2;
    }
    SC_LDS_ATTR(ctx, scopa::kLdsTeamChance, k_team_chance_sub, (int)kSubLds);
    const int32_t *mark = h_deals ? g->d_cs_mark : nullptr;
    for (int32_t it = 0; it < n_iters; it++) {   // the weights are launch arguments, as in cfr_iterate; no host synchronisation in between
        const double wpos = h_w ? h_w[it * 3 + 0] : 1.0, wneg = h_w ? h_w[it * 3 + 1] : 1.0, wstrat = h_w ? h_w[it * 3 + 2] : 1.0;
        const int32_t *list = h_deals ? g->d_cs_list + (size_t)it * m : nullptr;
        double *root = h_root_values ? g->d_root + (size_t)it * 2 : nullptr;
        if (list) hipLaunchKernelGGL(k_team_chance_mark, dim3(1), dim3(256), 0, ctx->stream, list, m, g->d_cs_mark, g->n);
        for (int p = 0; p < 2; p++) {
            // simultaneous: both sweeps against the sigma rows of the iteration's start (their image rows are disjoint), then one reduce of both teams
            double *rootdeal = alternating || p == 0 ? g->d_rootdeal : g->d_cs_root;
            hipLaunchKernelGGL(k_team_chance_sub, dim3(kSubtrees, slots), dim3(kSubThreads), kSubLds, ctx->stream, (const double *)g->d_sig, (const int32_t *)g->d_map,
                               (const int8_t *)g->d_r2, g->d_img, g->d_sub, p, list);
            hipLaunchKernelGGL(k_team_chance_top, dim3(slots), dim3(kSubThreads), 0, ctx->stream, (const double *)g->d_sig, (const int32_t *)g->d_map, g->d_img,
                               (const double *)g->d_sub, rootdeal, p, list);
            if (alternating || p == 1)
                hipLaunchKernelGGL(k_team_chance_reduce_sampled, dim3(blocks_of(g->G)), dim3(256), 0, ctx->stream, (const uint64_t *)g->d_gkey, (const int32_t *)g->d_occ_off,
                                   (const int32_t *)g->d_occ, (const double *)g->d_img, mark, g->d_R, g->d_S, g->d_sig, g->G, alternating ? p : -1, wpos, wneg, wstrat,
                                   (const double *)g->d_rootdeal, (const double *)rootdeal, g->n, slots, root);
            SC_HIP(ctx, hipGetLastError());
        }
    }
    if (h_root_values) {
        SC_HIP(ctx, hipMemcpyAsync(h_root_values, g->d_root, sizeof(double) * 2 * (size_t)n_iters, hipMemcpyDeviceToHost, ctx->stream));
        SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return SCOPA_OK;
}

int32_t scopa_team_chance_cfr_launch(scopa_team_chance *g, int32_t traverser, int32_t part) {
    if (!g || traverser < 0 || traverser > 1 || part < 0 || part > 2) return SCOPA_EINVAL;
    scopa_ctx *ctx = g->ctx;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    if (part == 0) {
        SC_LDS_ATTR(ctx, scopa::kLdsTeamChance, k_team_chance_sub, (int)kSubLds);
        hipLaunchKernelGGL(k_team_chance_sub, dim3(kSubtrees, g->n), dim3(kSubThreads), kSubLds, ctx->stream, (const double *)g->d_sig, (const int32_t *)g->d_map,
                           (const int8_t *)g->d_r2, g->d_img, g->d_sub, traverser, (const int32_t *)nullptr);
    } else if (part == 1) {
        hipLaunchKernelGGL(k_team_chance_top, dim3(g->n), dim3(kSubThreads), 0, ctx->stream, (const double *)g->d_sig, (const int32_t *)g->d_map, g->d_img,
                           (const double *)g->d_sub, g->d_rootdeal, traverser, (const int32_t *)nullptr);
    } else {
        hipLaunchKernelGGL(k_team_chance_reduce, dim3(blocks_of(g->G)), dim3(256), 0, ctx->stream, (const uint64_t *)g->d_gkey, (const int32_t *)g->d_occ_off,
                           (const int32_t *)g->d_occ, (const double *)g->d_img, g->d_R, g->d_S, g->d_sig, g->G, traverser, 1.0, 1.0, 1.0, (const double *)g->d_rootdeal, g->n,
                           (double *)nullptr);
    }
    SC_HIP(ctx, hipGetLastError());
    return SCOPA_OK;
}

int32_t scopa_team_chance_exploitability(scopa_team_chance *g, const double *d_policy, double *h_out4, double *d_policy_out, double *d_br) {
    if (!g || !h_out4) return SCOPA_EINVAL;
    scopa_ctx *ctx = g->ctx;
    SC_REQUIRE(ctx, (((uintptr_t)d_policy | (uintptr_t)d_policy_out | (uintptr_t)d_br) & 31) == 0, SCOPA_EINVAL, "scopa_team_chance_exploitability: tables must be 32-byte aligned");
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const int n = g->n;
    const size_t Gs = (size_t)g->G;
    if (!g->d_reach) {
        const bool ok = hipMalloc(&g->d_reach, (size_t)n * kTNodes * 8) == hipSuccess && hipMalloc(&g->d_val, (size_t)n * kTNodes * 8) == hipSuccess &&
                        hipMalloc(&g->d_pol, Gs * 32) == hipSuccess && hipMalloc(&g->d_choice, Gs * 4) == hipSuccess && hipMalloc(&g->d_vals, (size_t)n * 3 * 8) == hipSuccess;
        if (!ok) {
            void *bufs[] = {g->d_reach, g->d_val, g->d_pol, g->d_choice, g->d_vals};
            for (void *b : bufs) if (b) (void)hipFree(b);
            g->d_reach = g->d_val = g->d_pol = g->d_vals = nullptr; g->d_choice = nullptr;
            return fail(ctx, SCOPA_ENOMEM, "scopa_team_chance_exploitability: no device memory for the scratch");
        }
    }
    const int32_t *map = g->d_map;
    const double *pol = g->d_pol;
    hipLaunchKernelGGL(k_team_chance_policy, dim3(blocks_of(g->G)), dim3(256), 0, ctx->stream, (const uint64_t *)g->d_gkey, (const double *)g->d_S, d_policy, g->d_pol, g->G);
    if (d_policy_out) SC_HIP(ctx, hipMemcpyAsync(d_policy_out, g->d_pol, Gs * 32, hipMemcpyDeviceToDevice, ctx->stream));
    for (int pass = 0; pass < 3; pass++) {   // 0 / 1: that team responds, valued for itself; 2: nobody does, valued for team 0
        const int persp = pass == 1 ? 1 : 0;
        if (pass < 2)
            hipLaunchKernelGGL(k_team_chance_opp_reach, dim3(blocks_of((long long)n * kTChoice)), dim3(256), 0, ctx->stream, map, pol, g->d_reach, (long long)n * kTChoice, pass);
        hipLaunchKernelGGL(k_team_chance_leaf_values, dim3(blocks_of((long long)n * kTLeaves)), dim3(256), 0, ctx->stream, (const int8_t *)g->d_r2, g->d_val,
                           (long long)n * kTLeaves, persp);
        for (int d = 11; d >= 0; d--) {
            const unsigned blocks = blocks_of((long long)n * t_width(d));
#define SC_TC_LEVEL(what) hipLaunchKernelGGL(k_team_chance_level, dim3(blocks), dim3(256), 0, ctx->stream, (what), d, map, pol, (const double *)g->d_reach, g->d_val, g->d_img, \
                                             (const int32_t *)g->d_choice, n)
            if (pass < 2 && t_team(d) == pass) {
                const long long lo = g->depth_off[d], hi = g->depth_off[d + 1];
                SC_TC_LEVEL((int)kLevelQ);
                hipLaunchKernelGGL(k_team_chance_choose, dim3(blocks_of(hi - lo)), dim3(256), 0, ctx->stream, lo, hi, t_branch(d), (const int32_t *)g->d_occ_off,
                                   (const int32_t *)g->d_occ, (const double *)g->d_img, g->d_choice);
                SC_TC_LEVEL((int)kLevelSelect);
            } else {
                SC_TC_LEVEL((int)kLevelFollow);
            }
#undef SC_TC_LEVEL
        }
        hipLaunchKernelGGL(k_team_chance_roots, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, (const double *)g->d_val, g->d_vals + (size_t)pass * n, n);
        if (pass < 2 && d_br)
            hipLaunchKernelGGL(k_team_chance_br_table, dim3(blocks_of(g->G)), dim3(256), 0, ctx->stream, (const uint64_t *)g->d_gkey, pol, (const int32_t *)g->d_choice,
                               d_br + (size_t)pass * Gs * 4, g->G, pass);
        SC_HIP(ctx, hipGetLastError());
    }
    std::vector<double> v((size_t)n * 3);
    SC_HIP(ctx, hipMemcpyAsync(v.data(), g->d_vals, v.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    double mean[3];
    for (int pass = 0; pass < 3; pass++) {   // (v_deal0 + v_deal1 + ...) / n in deal order
        double s = v[(size_t)pass * n];
        for (int d = 1; d < n; d++) s += v[(size_t)pass * n + d];
        mean[pass] = s / (double)n;
    }
    h_out4[0] = (mean[0] + mean[1]) / 2.0; h_out4[1] = mean[0]; h_out4[2] = mean[1]; h_out4[3] = mean[2];
    return SCOPA_OK;
}

int32_t scopa_team_chance_policy_for_deal(scopa_team_chance *g, const double *d_policy_G, int32_t deal, double *d_policy_local) {
    if (!g || !d_policy_G || !d_policy_local || deal < 0 || deal >= g->n) return SCOPA_EINVAL;
    scopa_ctx *ctx = g->ctx;
    SC_REQUIRE(ctx, (((uintptr_t)d_policy_G | (uintptr_t)d_policy_local) & 31) == 0, SCOPA_EINVAL, "scopa_team_chance_policy_for_deal: tables must be 32-byte aligned");
    SC_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_team_chance_scatter, dim3(blocks_of(kTChoice)), dim3(256), 0, ctx->stream, (const int32_t *)(g->d_map + (size_t)deal * kTChoice), d_policy_G, d_policy_local);
    SC_HIP(ctx, hipGetLastError());
    return SCOPA_OK;
}

}  // extern "C"
