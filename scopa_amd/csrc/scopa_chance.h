// scopa_chance.h -- the object behind scopa_chance_* (scopa_chance.hip), shared with the translation unit that plays policies against each other
// on it (scopa_chance_xplay.hip).
#pragma once
#include <vector>

#include "scopa_ctx.h"
#include "scopa_multi.h"

constexpr int kChanceMaxDeals = 1 << 16;   // 65536 deals: delta rows 6.9 GB, occurrence ids (deal * 1653 + local) well inside int32
constexpr int kSdListRing = 4;             // pinned staging rows of scopa_chance_sdcfr_traverse's deal lists

struct scopa_chance {
    scopa_multi *m = nullptr;
    scopa_ctx *ctx = nullptr;
    int n = 0;
    long long G = 0, n_occ = 0;
    uint64_t *d_gkey = nullptr;      // [G] distinct keys, ascending
    int32_t *d_map = nullptr;        // [n][1653] local id -> global id, -1 past the deal's count
    int32_t *d_occ_off = nullptr;    // [G + 1]
    int32_t *d_occ = nullptr;        // [n_occ] deal * 1653 + local, ascending per global id
    uint16_t *d_order = nullptr;     // [n][1656] the deal's local ids ordered by (ply, local id)
    int32_t *d_plyoff = nullptr;     // [n][12]  [d] .. [d + 1]: ply d's span of d_order
    double *d_R = nullptr, *d_S = nullptr, *d_sig = nullptr;   // [G][4]
    double *d_delta = nullptr;       // [n][1653][8] increments of the sweep at hand; the q rows of an exploitability pass
    double *d_reach = nullptr, *d_val = nullptr;   // [n][2229] exploitability: reach of everyone but the responder, node values (allocated at first use)
    double *d_pol = nullptr, *d_pin = nullptr;     // [G][4] evaluated policy, a caller's policy
    int32_t *d_choice = nullptr;     // [G] the responder's action
    double *d_out = nullptr;         // [4]
    double *d_w = nullptr;           // [w_cap][3] weights of the call at hand
    size_t w_cap = 0;
    int32_t *d_list = nullptr;       // [list_cap] the sampled deals of the call at hand, [n_iters][m] (allocated at the first sampled call)
    size_t list_cap = 0;
    long long *d_stamp = nullptr;    // [n] (serial << 20) | slot of the last sampled sweep that took the deal; 0 = never (first sampled call)
    long long serial = 0;            // one per sampled (half-)sweep or MCCFR iteration over the handle's lifetime, from 1
    unsigned long long *d_mc_visits = nullptr;   // [n][2] decision | terminal visits of the MCCFR walks per deal (allocated at the first MCCFR call)
    uint32_t mccfr_iteration = 0;    // MCCFR iterations run on this handle: the Philox iteration word of the next one
    // Deep CFR over the set (scopa_chance_sdcfr_*), everything allocated at first use
    void *d_sdninfo = nullptr;       // [n][1653] uint2: feature bits | hand nibbles of every decision node of every deal (k_sdcfr_nodeinfo), built once
    bool sdninfo_built = false;
    void *d_sdtab = nullptr;         // [slots][1653] float4 policies, then [slots][1653][3] uint64 thresholds of the traversal call at hand
    int sdtab_slots = 0;
    int32_t *d_sdlist = nullptr;     // [n] the deal list of the traversal call at hand
    int32_t *h_sdlist = nullptr;     // [kSdListRing][n] pinned staging of the lists: a call copies from its turn's row without waiting for the stream
    hipEvent_t sd_ev[4] = {nullptr, nullptr, nullptr, nullptr};   // behind the copy out of each row
    unsigned sd_turn = 0;
    uint64_t sdcfr_visits = 0;       // decision visits of the traversal calls, counted on the host
    void *d_sdrep[2] = {nullptr, nullptr};   // per player [sd_keys[p]] uint4 {feature bits, hand nibbles, global id, legal count} of its keys' representative nodes
    int sd_keys[2] = {0, 0};
    bool sdrep_built = false;
    void *d_sdterms = nullptr;       // [n_snap][keys of the player] float4 terms of the average-policy call at hand
    size_t sdterms_bytes = 0;
    // policies against each other (scopa_chance_xplay.hip), everything allocated at first use
    double *d_xp_img = nullptr;      // [n][n_pol][n_pol][4] per-deal image of a cross-play call without a caller's d_per_deal (grown on demand)
    size_t xp_img_bytes = 0;
    void *d_xbr = nullptr;           // best-response scratch of a chunk of policies: reach, values [kc][n][2229], q rows [kc][n][1653][8], choices [kc][G]
    size_t xbr_bytes = 0;
    size_t xbr_budget = (size_t)1 << 30;   // what that scratch may take: policies go through in chunks that stay below it (one policy at least)
    void *d_xmatch = nullptr;        // [2][G][3] uint64 thresholds of the two tables of a match, then its ten sums
    std::vector<uint64_t> h_gkey;
    std::vector<int32_t> h_map;
};

namespace scopa {
// scopa_chance_exploitability's and scopa_chance_best_response's three passes over `chunk` policies (scopa_chance_xplay.hip)
void chance_br_passes(scopa_chance *g, int chunk, const double *policies, double *reach, double *val, double *q, int32_t *choice, double *out4, double *d_br);
}
