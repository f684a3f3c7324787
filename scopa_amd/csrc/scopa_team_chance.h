// scopa_team_chance.h -- the object behind scopa_team_chance_* (scopa_team_chance.hip): Team MiniScopa over a set of deals, its index of shared
// infosets, the shared tables and the scratch of its passes; the sampling solver's state beside them (scopa_team_chance_mccfr.hip).
#pragma once
#include <vector>

#include "scopa_team_solver.h"

constexpr int kTNodes = kTChoice + kTLeaves;   // choice nodes, then the depth-12 nodes: the stride of a deal in the reach and value scratch
constexpr long long kTeamChanceImageBudget = 32ll << 30;   // default byte budget of the increment image: 1 670 deals

namespace {
__device__ __forceinline__ int key_depth(uint64_t key) { return (int)(key >> 60); }
}  // namespace

struct scopa_team_chance {
    scopa_ctx *ctx = nullptr;
    int n = 0;
    long long G = 0, n_occ = 0;
    long long depth_off[13] = {0};   // global ids of depth d: [depth_off[d], depth_off[d + 1]) -- the depth is the key's top nibble and keys ascend
    uint64_t *d_gkey = nullptr;      // [G] distinct keys, ascending
    int32_t *d_map = nullptr;        // [n][321365] local row -> global id
    int32_t *d_occ_off = nullptr;    // [G + 1]
    int32_t *d_occ = nullptr;        // [n_occ] deal * 321365 + row, ascending per global id
    int8_t *d_r2 = nullptr;          // [n][331776] r2 of team 0 at every depth-12 node
    double *d_R = nullptr, *d_S = nullptr, *d_sig = nullptr;   // [G][4]
    double *d_img = nullptr;         // [n][321365][8] increment rows of the traversal at hand; the q rows of a best-response level
    double *d_sub = nullptr;         // [n][256] subtree values between the two sweep launches
    double *d_rootdeal = nullptr;    // [n] the deals' root values of the traversal at hand
    double *d_root = nullptr;        // [root_cap] root values of a cfr_iterate call that asked for them
    size_t root_cap = 0;
    // deal-sampled iterations (scopa_team_chance_cfr_iterate_sampled), allocated at its first call
    int32_t *d_cs_list = nullptr;    // [cs_list_cap] the deal lists of the call at hand, [n_iters][m]
    size_t cs_list_cap = 0;
    int32_t *d_cs_mark = nullptr;    // [n] 1 where the deal is in the list of the iteration at hand
    double *d_cs_root = nullptr;     // [n] traverser 1's root values per deal in a simultaneous iteration
    // exploitability, allocated at first use
    double *d_reach = nullptr, *d_val = nullptr;   // [n][653141] reach of the responder's opponents; node values, the depth-12 nodes behind the rows
    double *d_pol = nullptr;         // [G][4] the evaluated policy
    int32_t *d_choice = nullptr;     // [G] the responder's slot
    double *d_vals = nullptr;        // [3][n] per-deal root values of the three passes
    // the sampling solver (scopa_team_chance_mccfr.hip), allocated at its first call
    double *d_mc_delta = nullptr;    // [G][5] 4 regret increments + traverser-visit count of the walks since the last apply; all-zero between iterations
    int32_t *d_mc_list = nullptr;    // [mc_list_cap] the deal lists of the mccfr_iterate call at hand
    size_t mc_list_cap = 0;
    std::vector<int32_t> h_mc_list;  // what d_mc_list holds: the same lists again are not uploaded again
    uint32_t mccfr_iteration = 0;    // applies since create: the Philox iteration word of scopa_team_chance_mccfr_iterate
    unsigned long long mccfr_decision = 0, mccfr_terminal = 0;   // visits of the walks, from the recursion's fixed shape
    // Deep CFR over the set (scopa_team_chance_sdcfr.hip), everything allocated at first use and freed by scopa::team_chance_sdcfr_release
    void *d_sd_ninfo = nullptr;      // [n][321365] uint2: feature bits | hand nibbles of every choice node of every deal, built once
    uint32_t *d_sd_finfo = nullptr;  // [n][4][331776] feature bits of the forced nodes of depths 12..15 below every depth-12 node, built once
    bool sd_info_built = false;
    void *d_sd_tab = nullptr;        // the policy tables of the traversal call at hand (layout: scopa_team_chance_sdcfr.hip), sd_tab_slots slots
    int sd_tab_slots = 0, sd_last_m = 0;   // sd_last_m: slots the last traversal call filled (0 = none yet)
    int32_t *d_sd_list = nullptr;    // [n] the deal list of the traversal call at hand
    int32_t *h_sd_list = nullptr;    // [4][n] pinned staging of the lists: a call copies from its turn's row without waiting for the stream
    hipEvent_t sd_ev[4] = {nullptr, nullptr, nullptr, nullptr};   // behind the copy out of each row
    unsigned sd_turn = 0;
    uint64_t sd_visits = 0;          // non-terminal visits of the traversal calls, counted on the host
    void *d_sd_rep[2] = {nullptr, nullptr};   // per team [sd_keys[t]] uint4 {feature bits, hand nibbles, global id, legal count} of its keys' representative nodes
    long long sd_keys[2] = {0, 0};
    bool sd_rep_built = false;
    void *d_sd_terms = nullptr;      // float4 terms [n_snap][chunk of keys] of the average-policy call at hand
    size_t sd_terms_bytes = 0;
    scopa_team_xplay_scratch xp;     // cross-play and match (scopa_team_xplay.hip): leaf scopas [n][331776] and the scratch images, allocated at first use
    std::vector<scopa_team_state> h_roots;   // the deals' roots, for the leaf scopas
    std::vector<uint64_t> h_gkey;
    std::vector<int32_t> h_map;
};

namespace scopa {
void team_chance_sdcfr_release(scopa_team_chance *g);   // scopa_team_chance_sdcfr.hip
}
