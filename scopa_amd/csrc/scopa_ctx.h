// scopa_ctx.h -- context object behind the C ABI (include/scopa.h): one HIP device, one stream, one deal.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../include/scopa.h"
#include "scopa_rules.h"

// Device-resident data of one context.
//
//  tree (built on device by k_tree_build, BFS/level order; the tree's shape is deal-independent so children
//  are index arithmetic and only two small arrays are kept):
//    d_states   [2229]  scopa_state per node            (35.7 KB)
//    d_infoset  [1653]  uint16 dense infoset id per decision node; ids in reference DFS first-visit order
//    d_payoff   [576]   int8 rewards_x2 of player 0 at each terminal (player 1 = negation)
//    d_key      [1653]  uint64 infoset key per infoset id
//  tables, row-padded [kDecision][4] float64 (only the first n_infosets rows are live):
//    d_regret, d_strat, d_local
//  batched MCCFR:
//    d_delta    [kDecision][5] float64: 4 regret deltas + traverser-visit count (the all-reduce payload)
//    d_groups   [8][5][kDecision] float64: group tables the traversal launches add their partial deltas into (memory-side atomics)
struct scopa_p2p;  // scopa_p2p.hip
struct scopa_team_solver;  // scopa_team_cfr.hip

struct scopa_ctx {
    int device = -1;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    char err[512] = {0};

    bool has_deal = false;
    uint8_t perm[16] = {0};
    int n_infosets = 0;

    scopa_state *d_states = nullptr;
    uint16_t *d_infoset = nullptr;
    int8_t *d_payoff = nullptr;
    uint64_t *d_key = nullptr;
    int32_t *d_meta = nullptr;  // [0] = n_infosets, [1] = first-visit sequence counter
    uint32_t *d_visit = nullptr;  // [kDecision] first-visit sequence number per infoset (0 = unvisited)

    double *d_regret = nullptr, *d_strat = nullptr, *d_local = nullptr;
    double *d_delta = nullptr;        // buffer in use (internal or caller-bound)
    double *d_delta_own = nullptr;    // the internal one
    double *d_scratch = nullptr;  // root values / uniforms staging
    double *d_sigcdf = nullptr;   // [kDecision][6] sigma | threshold rows of the frozen regret table (48 bytes: the layout the traversal keeps in LDS)
    bool sigcdf_valid = false;    // false whenever d_regret changed outside k_mccfr_apply
    bool mccfr_all_seen = false;  // every infoset of the deal has a first-visit mark in d_visit: traversal launches stop tracking first visits (scopa_mccfr.hip); false after scopa_tables_reset
    uint32_t mccfr_seen_wait = 0; // traversal launches since the marks were last counted
    double *d_groups = nullptr;   // [kDeltaGroups group tables][5][kGroupRows] float64: where traversal launches add their deltas (scopa_mccfr.hip); all-zero between launches' applies
    unsigned long long *d_clock = nullptr;   // [2048 sampled launches][512 workgroups][4] phase stamps on the 100 MHz device clock (allocated by scopa_prof_enable)
    uint16_t clock_grid[2048] = {0};         // workgroups of each sampled launch
    double prof_phase_us[3] = {0.0, 0.0, 0.0};   // mean (prologue, walks, epilogue) per workgroup of the samples last folded by scopa_prof_device
    double prof_spread_us[3] = {0.0, 0.0, 0.0};   // scopa_prof_spread: workgroup start offsets and the longest workgroup of the sampled launches
    size_t scratch_bytes = 0;

    unsigned long long *d_counters = nullptr;  // [0] decision visits, [1] terminal visits, [2] aux

    uint64_t seed = 0x5C09A;
    uint64_t sdcfr_visits = 0;  // decision-node visits of SDCFR traversals (one per frontier slot featurised)
    void *d_sdnode = nullptr;   // [kDecision] uint2: feature bits | mover's hand nibbles of every decision node (scopa_sdcfr.hip: k_sdcfr_nodeinfo), built at first use per deal
    bool sdnode_valid = false;  // false after scopa_set_deal
    void *d_eval_thr = nullptr;        // [kDecision][3] uint64: sampling thresholds of the tabular policy last given to scopa_eval_tabular_prepare
    bool eval_thr_valid = false;
    void *d_pair_thr = nullptr;        // [2][kDecision][3] uint64 thresholds of the two tables of scopa_eval_pair_match, then its ten sums (scopa_xplay.hip), allocated at first use
    void *d_train_partial = nullptr;   // [32][kStride = 13777] float: per-workgroup partial gradients (+ partial loss) of scopa_sdcfr_train_steps (scopa_train.hip; the shape: scopa_train_tile.h), allocated at first use
    void *d_full_train_partial = nullptr;   // [256][kStride = 23276] float partials of scopa_full_sdcfr_train_steps (23272 gradients, 3 loss sums, 1 pad), then their sum [23276] and 364 sums of squares (scopa_full_train.hip), allocated at first use
    void *d_sdpol = nullptr;    // [kDecision] float4: regret-matching policy of every decision node under the nets of the launch at hand (k_sdcfr_policy)
    bool sdpol_valid = false;   // d_sdpol holds a table computed on THIS deal; false after scopa_set_deal (scopa_sdcfr_policy_get then refuses)
    void *d_sdavg = nullptr;    // [n_snap][916] float4: weighted regret-matching policies per (snapshot, node) of scopa_sdcfr_average_policy's first pass
    size_t sdavg_bytes = 0;
    int sdcfr_mode = 0;         // 0 = policy table per launch + walks (one deal: every node evaluated once), 1 = a forward pass per visit (k_sdcfr_traverse)
    uint32_t iteration = 0;

    // profiling of the dominant kernel
    bool prof_on = false;
    int prof_stride = 1;
    long long prof_tick = 0;
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    int64_t prof_launches = 0;
    double prof_ms = 0.0;

    // exact vanilla CFR, scheduled form (scopa_cfr.hip): EXIT events of the deal's tree levelled under the per-infoset visit order
    uint32_t *d_lane_tab = nullptr;   // [15][64] uint4: what a lane's node slots are made of, for the traversal kernels (scopa_mccfr.hip: LaneSlots), built at first use
    uint16_t *d_sched = nullptr;   // events (uint32 each) | step offsets | [kDecision][8] path cells (layout: scopa_cfr.hip)
    int sched_steps = 0;
    bool sched_valid = false;      // false after scopa_set_deal
    int exact_last_route = -1;     // scopa_cfr_exact_last_route: 0 scheduled, 1 walk with LDS tables, 2 walk with HBM tables
    bool exact_sequential = false; // scopa_cfr_exact_mode(ctx, 1): force the one-lane walk (the form the schedule is checked against)

    scopa_p2p *p2p = nullptr;  // peer-memory exchange of the N > 1 path
    scopa_team_solver *team = nullptr;  // Team MiniScopa deal, tables and scratch (scopa_team_set_deal); independent of the MiniScopa deal above

    // graph mode of scopa_mccfr_iterate (scopa_mccfr.hip): captured (traverse, apply) x k chains by (batch, k); the iteration number
    // the captured launches use lives in d_meta[2]
    struct GraphEntry { uint32_t batch, k, track; void *exec; };
    std::vector<GraphEntry> mccfr_graphs;
    bool mccfr_graph_mode = false;

    int lds_limit = 160 * 1024;
    int n_cus = 256;
    uint32_t lds_attr_done = 0;  // kernels whose dynamic-LDS cap was raised on THIS context's device (scopa::ensure_lds_attr)
    long long team_xplay_group_limit = 0;  // scopa_team_debug_xplay_group_limit: workgroups a team cross-play launch may have; 0 = 2^31
    long long team_chance_budget = 0;  // scopa_team_chance_debug_image_budget: bytes an increment image may take at create; 0 = the default
    long long team_sdcfr_budget = 0;   // scopa_team_chance_debug_sdcfr: bytes the terms of scopa_team_chance_sdcfr_average_policy may take; 0 = 1 GiB
    int team_sdcfr_walk_groups = 0;    // ... and the workgroups a slot of scopa_team_chance_sdcfr_traverse's walk launch may have; 0 = the default
    int full_sdcfr_launches = 0;       // scopa_full_chance_debug_sdcfr: which launches a scopa_full_chance_sdcfr_traverse call makes: 0 both, 1 the policy launch alone, 2 the walk launch alone (benchmarks)
    int team_sdcfr_launches = 0;       // ... and which of its launches a call makes: 0 both, 1 the policy launch alone, 2 the walk launch alone (benchmarks)
    long long full_sdcfr_scratch = 0;  // scopa_full_chance_debug_sdcfr_scratch: bytes a chunk of scopa_full_chance_sdcfr_traverse_frontier's traversals may take; 0 = 1 GiB
    void *d_full_avg_slots = nullptr;  // [full_avg_slots_n] int32: the FIFO slot list of the scopa_full_chance_sdcfr_average_at call at hand, grown where a call lists more
    size_t full_avg_slots_n = 0;
    int full_avg_grid = 0;             // scopa_full_chance_debug_sdcfr_average_grid: workgroups of an average_at launch (at most one per tile); 0 = the rule of launch_average_at
};

namespace scopa {

// group tables of the batched-MCCFR delta (scopa_mccfr.hip): cell-major tables of [5][kGroupRows] float64 per context
#ifndef SCOPA_GROUPS
#define SCOPA_GROUPS 16
#endif
#ifndef SCOPA_GROUP_PERM
#define SCOPA_GROUP_PERM 0
#endif
constexpr int kDeltaGroups = SCOPA_GROUPS;
constexpr int kGroupRows = 1664;                                   // kDecision rounded up to 64 x 26
constexpr size_t kDeltaTable = (size_t)kGroupRows * 5;             // doubles per group table
// where cell k (0..3 regret deltas, 4 visit count) of infoset row r lies in a group table
__host__ __device__ inline size_t group_cell(int k, int r) {
#if SCOPA_GROUP_PERM == 1
    return (size_t)k * kGroupRows + (size_t)((r & 63) * 26 + (r >> 6));
#elif SCOPA_GROUP_PERM == 2
    return (size_t)k * kGroupRows + (size_t)((r & 7) * 208 + (r >> 3));
#else
    return (size_t)k * kGroupRows + (size_t)r;
#endif
}
constexpr int kClockSamples = 2048, kClockStride = 2048;           // sampled launches kept / uint64 per sample (512 workgroups x 4 phase stamps)

inline int32_t fail(scopa_ctx *ctx, int32_t code, const char *what, hipError_t e = hipSuccess) {
    if (ctx) {
        if (e != hipSuccess) snprintf(ctx->err, sizeof ctx->err, "%s: %s", what, hipGetErrorString(e));
        else snprintf(ctx->err, sizeof ctx->err, "%s", what);
    }
    return code;
}

#define SC_HIP(ctx, call)                                                         \
    do {                                                                          \
        hipError_t e__ = (call);                                                  \
        if (e__ != hipSuccess) return scopa::fail((ctx), SCOPA_EHIP, #call, e__); \
    } while (0)

#define SC_REQUIRE(ctx, cond, code, msg)                        \
    do {                                                        \
        if (!(cond)) return scopa::fail((ctx), (code), (msg)); \
    } while (0)

int32_t ensure_scratch(scopa_ctx *ctx, size_t bytes);

// roctx ranges around the solver's phases (traverse / exchange + apply / train), for rocprofv3 --marker-trace timelines: on only with SCOPA_ROCTX=1 in the
// environment (resolved once, from librocprofiler-sdk-roctx.so / libroctx64.so by dlopen: no link-time dependency, nothing in the loop otherwise)
void range_push(const char *name);
void range_pop();
struct Range { explicit Range(const char *n) { range_push(n); } ~Range() { range_pop(); } };

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-DEVICE property of a kernel, so the "already raised" flag lives in the
// context (one context = one device), not in a process-wide static: a second context on another device raises it again.
enum LdsAttrKernel : uint32_t { kLdsTraverse = 1u, kLdsReplay = 8u, kLdsCfrExact = 16u, kLdsCfrSched = 512u, kLdsExploit = 32u, kLdsCfrSync = 64u, kLdsSdcfr = 128u, kLdsMulti = 256u, kLdsSdcfrReplay = 1024u, kLdsSdPolicy = 2048u, kLdsSdWalk0 = 4096u, kLdsSdWalk1 = 8192u, kLdsCfrSyncW = 16384u, kLdsCrossPlay = 32768u, kLdsBestResponse = 65536u, kLdsMccfrChance = 131072u, kLdsChanceSdWalk0 = 262144u, kLdsChanceSdWalk1 = 524288u, kLdsChanceCrossPlay = 1048576u, kLdsTeamCfr = 2097152u, kLdsTeamChance = 4194304u, kLdsFullTrain = 8388608u };
// scopa_*_cfr_sync_iterate_weighted: every weight of h_w[n_iters][3] finite and in [0, 1] (a NaN fails both compares)
inline bool cfr_weights_ok(const double *h_w, int32_t n_iters) {
    for (size_t k = 0; k < (size_t)n_iters * 3; k++) if (!(h_w[k] >= 0.0 && h_w[k] <= 1.0)) return false;
    return true;
}
inline int32_t ensure_lds_attr(scopa_ctx *ctx, uint32_t kernel_bit, const void *fn, int bytes) {
    if (ctx->lds_attr_done & kernel_bit) return SCOPA_OK;
    SC_HIP(ctx, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    ctx->lds_attr_done |= kernel_bit;
    return SCOPA_OK;
}
#define SC_LDS_ATTR(ctx, bit, kernel, bytes)                                                                     \
    do {                                                                                                         \
        const int32_t rc__ = scopa::ensure_lds_attr((ctx), (bit), reinterpret_cast<const void *>(kernel), (bytes)); \
        if (rc__ != SCOPA_OK) return rc__;                                                                       \
    } while (0)
// (start, stop) events to attach to a sampled launch of the dominant kernel when profiling is on
bool prof_events(scopa_ctx *ctx, hipEvent_t *start, hipEvent_t *stop);
void p2p_release(scopa_ctx *ctx);
void team_release(scopa_ctx *ctx);   // scopa_team_cfr.hip: frees the team state on context destruction
void mccfr_graphs_clear(scopa_ctx *ctx);   // scopa_mccfr.hip: on a new deal, a new seed, context destruction

}  // namespace scopa
