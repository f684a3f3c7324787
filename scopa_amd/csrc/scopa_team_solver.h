// scopa_team_solver.h -- what the two Team MiniScopa solvers share: the tree's shape as constant expressions, the 32-byte table row, and the team
// state of a context (scopa_team_cfr.hip owns the tables and the deal, scopa_team_mccfr.hip the sampling solver's state beside them).
#pragma once
#include "scopa_ctx.h"

namespace {

constexpr int kTChoice = SCOPA_TEAM_N_CHOICE, kTLeaves = SCOPA_TEAM_N_LEAVES, kTInfosets = SCOPA_TEAM_N_INFOSETS;   // infosets = choice nodes + 4 forced plies x 331 776

__host__ __device__ constexpr int t_branch(int d) { return 4 - (d >> 2); }
__host__ __device__ constexpr int t_team(int d) { return (d & 3) >> 1; }
__host__ __device__ constexpr int t_width(int d) { int w = 1; for (int k = 0; k < d; k++) w *= t_branch(k); return w; }
__host__ __device__ constexpr int t_offset(int d) { int o = 0; for (int k = 0; k < d; k++) o += t_width(k); return o; }
static_assert(t_offset(12) == kTChoice && t_width(12) == kTLeaves, "tree shape");

__device__ __forceinline__ int depth_of_row(int row) {
    int d = 0;
#pragma unroll
    for (int k = 1; k < 12; k++) d += row >= t_offset(k) ? 1 : 0;
    return d;
}

struct Row4 { double x[4]; };
__device__ __forceinline__ Row4 load_row(const double *p) {
    const double4 v = *reinterpret_cast<const double4 *>(p);
    return Row4{{v.x, v.y, v.z, v.w}};
}
__device__ __forceinline__ void store_row(double *p, const Row4 &r) { *reinterpret_cast<double4 *>(p) = make_double4(r.x[0], r.x[1], r.x[2], r.x[3]); }

}  // namespace

// Scratch of the cross-play and match calls (scopa_team_xplay.hip), owned by a context's team state or by a handle over a set of deals; everything is
// allocated at the first call that needs it and freed with its owner.
struct scopa_team_xplay_scratch {
    uint8_t *d_leaf_sc = nullptr;                                 // [deals][331776] scopas at every depth-12 node: team 0 in the low nibble, team 1 in the high nibble
    bool leaf_sc_valid = false;                                   // false until built for the deal(s) in force
    double *d_sub = nullptr, *d_img = nullptr;                    // [deals][K * K][256][4] subtree values between the launches; [deals][K][K][4] where the caller gives no image
    size_t sub_bytes = 0, img_bytes = 0;
    unsigned long long *d_stats = nullptr;                        // [10] the sums of a match
};

// Team state of a context: next to the MiniScopa deal, never touched by scopa_set_deal, freed by scopa_ctx_destroy.
struct scopa_team_solver {
    bool has_deal = false;
    scopa_team_state root = {};                                   // the deal's root, for what is built from it after set_deal (the leaf scopas)
    scopa_team_xplay_scratch xp;
    int8_t *d_r2 = nullptr;                                       // [331776] r2 of team 0 at every depth-12 node
    double *d_R = nullptr, *d_S = nullptr, *d_L = nullptr;        // [321365][4]
    double *d_lrs = nullptr;                                      // [2][331776] leaf_reach_sum
    double *d_sub = nullptr;                                      // [256] subtree values between the two launches, then [8] values of the value passes
    double *d_avg = nullptr;                                      // [321365][4] the average policy scopa_team_exploitability evaluates (allocated at first use)
    double *d_root = nullptr;                                     // [n_iters][2] root values of a scopa_team_cfr_iterate call that asked for them
    size_t root_cap = 0;
    // the sampling solver (scopa_team_mccfr.hip), allocated at its first call; all-zero in the reset state
    uint8_t *d_seen = nullptr;                                    // [321365] a decision visit reached the row (the reference's dict holds its key)
    unsigned long long *d_leaf_visits = nullptr;                  // [2][331776] arrivals at each depth-12 node, per traverser
    double *d_delta = nullptr;                                    // [321365][5] 4 regret increments + traverser-visit count of the traversals since the last apply
    double *d_uniforms = nullptr;                                 // the replay's uniform stream
    size_t uniforms_cap = 0;
    long long *d_consumed = nullptr;                              // [1] uniforms the last replay launch read
    uint32_t mccfr_iteration = 0;                                 // applies since the reset: the Philox iteration word of scopa_team_mccfr_iterate
    unsigned long long mccfr_decision = 0, mccfr_terminal = 0;    // visits of the sampling solver's walks, from the recursion's fixed shape
};

namespace scopa {
int32_t team_mccfr_reset(scopa_ctx *ctx, scopa_team_solver *t);   // scopa_team_mccfr.hip: the sampling solver's state back to all-zero (set_deal, tables_reset)
void team_mccfr_release(scopa_team_solver *t);
void team_xplay_release(scopa_team_xplay_scratch *xp);            // scopa_team_xplay.hip
}  // namespace scopa

// the team state of a C ABI call, or SCOPA_ESTATE
#define SC_TEAM_READY(ctx, name)                                                                             \
    scopa_team_solver *t = (ctx)->team;                                                                      \
    SC_REQUIRE((ctx), t && t->has_deal, SCOPA_ESTATE, name ": no team deal set (scopa_team_set_deal)");      \
    SC_HIP((ctx), hipSetDevice((ctx)->device))
