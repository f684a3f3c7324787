// scopa_team_mccfr_walk.h -- the ONE definition of the level-by-level walk of Team MiniScopa's external-sampling MCCFR: a workgroup expands one
// traversal of one traverser through LDS against frozen regrets (the shape of the recursion, the records and the update are described at the top of
// scopa_team_mccfr.hip).  Two kernels run it: k_team_mccfr_walk on the one-deal tables (scopa_team_mccfr.hip) and k_team_chance_mccfr_walk on the
// rows a set of deals shares by key (scopa_team_chance_mccfr.hip).  They differ in where a local row's regret row and delta row live and in whether
// the walk leaves marks, and that is the ADDRESSING POLICY, a template parameter of every function that touches a table:
//
//   kMarks        the walk writes seen[row] at every decision visit and counts the arrivals at depth-12 nodes in leaf_visits
//   at(row)       the row of the regret table and of the delta buffer that belongs to the deal's local row `row`
//
// The LDS accumulator of the rows of depths 0..4 is indexed by LOCAL row under either policy; the kernel that owns it flushes it through at().
#pragma once
#include "scopa_mccfr_sigma.h"
#include "scopa_philox.h"
#include "scopa_team_solver.h"

namespace {

// ---- the instance tree ---------------------------------------------------------------------------------------------------------------------
template <int TRAV> __host__ __device__ constexpr int i_mult(int d) { return t_team(d) == TRAV ? t_branch(d) + 1 : 1; }
template <int TRAV> __host__ __device__ constexpr int i_width(int d) { int w = 1; for (int k = 0; k < d; k++) w *= i_mult<TRAV>(k); return w; }
template <int TRAV> __host__ __device__ constexpr int i_offset(int d) { int o = 0; for (int k = 0; k < d; k++) o += i_width<TRAV>(k); return o; }
// the traverser's K-th ply (0..5), the cards it plays from, and its instances: 1, 5, 25, 100, 400, 1 200 for either traverser
template <int TRAV> __host__ __device__ constexpr int s_depth(int k) { return 4 * (k >> 1) + (k & 1) + 2 * TRAV; }
__host__ __device__ constexpr int s_cards(int k) { return 4 - (k >> 1); }
__host__ __device__ constexpr int s_count(int k) { int w = 1; for (int j = 0; j < k; j++) w *= s_cards(j) + 1; return w; }
__host__ __device__ constexpr int s_first(int k) { int o = 0; for (int j = 0; j < k; j++) o += s_count(j); return o; }
constexpr int kStages = 6, kStageRecs = s_first(kStages), kArrivals = s_count(kStages);
constexpr int kShallowRows = t_offset(5);   // rows of depths 0..4, accumulated in LDS
constexpr unsigned long long kDraws0 = 49381, kDraws1 = 20583, kTerminals = 4ull * kArrivals;   // per traversal, forced tails included
static_assert(kStageRecs == 1731 && kArrivals == 3600 && kShallowRows == 341, "instance tree");
static_assert(i_offset<0>(12) == 9781 && i_offset<1>(12) == 2583 && i_width<0>(12) == kArrivals && i_width<1>(12) == kArrivals, "instance tree");
static_assert(i_offset<0>(12) + 11 * kArrivals == kDraws0 && i_offset<1>(12) + 5 * kArrivals == kDraws1, "draws per traversal");
static_assert(s_depth<0>(5) == 9 && s_depth<1>(5) == 11 && s_depth<1>(0) == 2, "traverser plies");
constexpr uint32_t kPhiloxTag = 64u;   // counter word 3 = 64 + traverser (0, 1: k_mccfr_traverse; 4, 5: SDCFR; 32: full-game playouts; 48: team playouts)

// np.random.choice(legal, p=sigma) (mc_cfr.py:55): cdf = cumsum(p); cdf /= cdf[-1]; searchsorted(cdf, u, side="right") -- the rule of k_mccfr_replay
template <int N>
__device__ __forceinline__ int choice(const double *sigma, double u) {
    double cdf[N];
    double c = sigma[0];
    cdf[0] = c;
#pragma unroll
    for (int i = 1; i < N; i++) { c += sigma[i]; cdf[i] = c; }
    const double last = cdf[N - 1];
    int a = 0;
#pragma unroll
    for (int i = 0; i < N; i++) a += cdf[i] / last <= u ? 1 : 0;
    return a < N - 1 ? a : N - 1;
}
// x[a] by compares: the values are passed one by one, so that no run-time index ever addresses the array (that would put it in scratch memory)
__device__ __forceinline__ double pick4(double x0, double x1, double x2, double x3, int a) {
    double r = x0;
    r = a == 1 ? x1 : r;
    r = a == 2 ? x2 : r;
    r = a == 3 ? x3 : r;
    return r;
}
template <int N>
__device__ __forceinline__ double pick(const double *x, int a) { return pick4(x[0], N > 1 ? x[1] : 0.0, N > 2 ? x[2] : 0.0, N > 3 ? x[3] : 0.0, a); }
// np.dot(sigma, cfv_all) (:79) as k_mccfr_replay writes it
template <int N>
__device__ __forceinline__ double dot(const double *sigma, const double *cfv) {
    double v = 0.0;
#pragma unroll
    for (int i = 0; i < N; i++) v = fma(sigma[i], cfv[i], v);
    return v;
}

// ---- the addressing policies -------------------------------------------------------------------------------------------------------------------
// the one-deal solver: a local row is its own table row; seen and leaf_visits are kept
struct OwnRows {
    static constexpr bool kMarks = true;
    __device__ __forceinline__ size_t at(size_t row) const { return row; }
};
// the chance game: the tables are over the global rows, a deal's local row goes through the deal's map row; no marks
struct MappedRows {
    static constexpr bool kMarks = false;
    const int32_t *map;   // [321365] of the deal at hand
    __device__ __forceinline__ size_t at(size_t row) const { return (size_t)map[row]; }
};

// ---- the walk --------------------------------------------------------------------------------------------------------------------------------
constexpr int kWalkThreads = 256;
struct WalkLds {
    double reach[kStageRecs], samp[kStageRecs];   // opponent reach and traverser sampling probability of a traverser instance, as running products
    double delta[kShallowRows * 5];               // the workgroup's increments into rows of depths 0..4
    uint32_t node[kStageRecs];                    // its node within its level | sampled action << 30
    int8_t val[kStageRecs + 5], leaf[kArrivals];  // return values, reward x2
};
static_assert(sizeof(WalkLds) == 53600, "LDS per workgroup");   // three would fit a compute unit; the kernel's 180 VGPRs allow two (a wavefront of each per SIMD)

template <class Addr>
struct Walk {
    const double *R;
    uint8_t *seen;               // kMarks only
    unsigned long long *lv;      // kMarks only
    const int8_t *r2;            // the deal's
    double *delta;
    uint32_t trav_id, iteration, seed_lo, seed_hi;
    Addr addr;
};

// one decision visit: the row's frozen sigma and the action its draw picks.  Philox counter (instance index in the traversal's recursion, global
// traversal id, iteration, 64 + traverser) under the context's seed; u = u53(x0, x1)
template <int D, int TRAV, class Addr>
__device__ __forceinline__ int visit(const Walk<Addr> &w, int node, int inst, double *sigma) {
    constexpr int n = t_branch(D);
    const size_t row = (size_t)t_offset(D) + node;
    if constexpr (Addr::kMarks) w.seen[row] = 1;
    const Row4 R = load_row(w.R + w.addr.at(row) * 4);
    scopa::mc_sigma(R.x, n, sigma);
    const scopa::philox_out x = scopa::philox4x32_10((uint32_t)(i_offset<TRAV>(D) + inst), w.trav_id, w.iteration, kPhiloxTag + TRAV, w.seed_lo, w.seed_hi);
    return choice<n>(sigma, scopa::u53(x.x0, x.x1));
}

// the other team's plies from depth D down to the traverser's next ply or depth 12: single children, the instance index carries over
template <int D, int TRAV, class Addr>
__device__ __forceinline__ void descend(const Walk<Addr> &w, int &node, int inst, double &reach) {
    if constexpr (D < 12 && t_team(D) != TRAV) {
        double sigma[4];
        const int a = visit<D, TRAV>(w, node, inst, sigma);
        reach = reach * pick<t_branch(D)>(sigma, a);
        node = node * t_branch(D) + a;
        descend<D + 1, TRAV>(w, node, inst, reach);
    }
}

template <int K, int TRAV, class Addr>
__device__ __forceinline__ void make_record(const Walk<Addr> &w, WalkLds &s, int node, int inst, double reach, double samp) {
    double sigma[4];
    const int a = visit<s_depth<TRAV>(K), TRAV>(w, node, inst, sigma);
    s.node[s_first(K) + inst] = (uint32_t)node | ((uint32_t)a << 30);
    s.reach[s_first(K) + inst] = reach;
    s.samp[s_first(K) + inst] = samp;
}

// the b + 1 child instances of every traverser instance of ply K: down to the next traverser ply's record, or to the depth-12 node
template <int K, int TRAV, class Addr>
__device__ __forceinline__ void expand(const Walk<Addr> &w, WalkLds &s, int tid) {
    constexpr int D = s_depth<TRAV>(K), b = s_cards(K);
    for (int j = tid; j < s_count(K + 1); j += kWalkThreads) {
        const int i = j / (b + 1), slot = j - i * (b + 1);
        const uint32_t rec = s.node[s_first(K) + i];
        const int pnode = (int)(rec & 0x3FFFFFFFu), c = slot == 0 ? (int)(rec >> 30) : slot - 1;
        const Row4 R = load_row(w.R + w.addr.at((size_t)t_offset(D) + pnode) * 4);
        double sigma[4];
        scopa::mc_sigma(R.x, b, sigma);
        double reach = s.reach[s_first(K) + i];
        const double samp = s.samp[s_first(K) + i] * pick<b>(sigma, c);   // :62, :77
        int node = pnode * b + c;
        descend<D + 1, TRAV>(w, node, j, reach);
        if constexpr (K + 1 < kStages) {
            make_record<K + 1, TRAV>(w, s, node, j, reach, samp);
        } else {
            if constexpr (Addr::kMarks) atomicAdd(w.lv + (size_t)TRAV * kTLeaves + node, 1ull);
            const int p0 = w.r2[node];
            s.leaf[j] = (int8_t)(TRAV == 0 ? p0 : -p0);
        }
    }
    __syncthreads();
}

// values up and the regret increments of ply K's instances (:79-83)
template <int K, int TRAV, class Addr>
__device__ __forceinline__ void update(const Walk<Addr> &w, WalkLds &s, int tid) {
    constexpr int D = s_depth<TRAV>(K), b = s_cards(K);
    const int8_t *below = K + 1 < kStages ? s.val + s_first(K + 1) : s.leaf;
    for (int i = tid; i < s_count(K); i += kWalkThreads) {
        const int node = (int)(s.node[s_first(K) + i] & 0x3FFFFFFFu);
        const int row = t_offset(D) + node;
        const size_t at = w.addr.at((size_t)row);
        const Row4 R = load_row(w.R + at * 4);
        double sigma[4], cfv[b];
        scopa::mc_sigma(R.x, b, sigma);
        s.val[s_first(K) + i] = below[i * (b + 1)];
#pragma unroll
        for (int c = 0; c < b; c++) cfv[c] = 0.5 * (double)below[i * (b + 1) + 1 + c];
        const double v = dot<b>(sigma, cfv);
        const double reach = s.reach[s_first(K) + i], samp = s.samp[s_first(K) + i];
        const double wt = samp > 0.0 ? reach / samp : 0.0;
#pragma unroll
        for (int c = 0; c < b; c++) {
            const double inc = wt * (cfv[c] - v);
            if (inc == 0.0) continue;   // adding 0.0 changes nothing: a loop child of probability 0 has weight 0 throughout its subtree
            if constexpr (D < 5) atomicAdd(s.delta + row * 5 + c, inc); else atomicAdd(w.delta + at * 5 + c, inc);
        }
        if constexpr (D < 5) atomicAdd(s.delta + row * 5 + 4, 1.0); else atomicAdd(w.delta + at * 5 + 4, 1.0);
    }
    __syncthreads();
}

template <int TRAV, class Addr>
__device__ __forceinline__ void walk_one(const Walk<Addr> &w, WalkLds &s, int tid) {
    if (tid == 0) {
        int node = 0;
        double reach = 1.0;
        descend<0, TRAV>(w, node, 0, reach);
        make_record<0, TRAV>(w, s, node, 0, reach, 1.0);
    }
    __syncthreads();
    expand<0, TRAV>(w, s, tid); expand<1, TRAV>(w, s, tid); expand<2, TRAV>(w, s, tid); expand<3, TRAV>(w, s, tid); expand<4, TRAV>(w, s, tid); expand<5, TRAV>(w, s, tid);
    update<5, TRAV>(w, s, tid); update<4, TRAV>(w, s, tid); update<3, TRAV>(w, s, tid); update<2, TRAV>(w, s, tid); update<1, TRAV>(w, s, tid); update<0, TRAV>(w, s, tid);
}

}  // namespace
