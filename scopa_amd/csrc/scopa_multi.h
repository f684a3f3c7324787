// scopa_multi.h -- the object behind scopa_multi_* (scopa_multi.hip), shared with the translation units that borrow its resident trees and keys
// (scopa_chance.hip).
#pragma once
#include "scopa_ctx.h"

struct scopa_multi {
    scopa_ctx *ctx = nullptr;
    int n = 0;
    bool built = false;
    int max_infosets = 0;
    uint8_t *d_perm = nullptr;       // [n][16]
    scopa_state *d_states = nullptr; // [n][2229]
    uint16_t *d_infoset = nullptr;   // [n][1653]
    int8_t *d_payoff = nullptr;      // [n][576]
    uint64_t *d_key = nullptr;       // [n][1653]
    int32_t *d_meta = nullptr;       // [n][8]
    double *d_regret = nullptr, *d_strat = nullptr, *d_local = nullptr;  // [n][1653][4]
    uint32_t *d_visit = nullptr;     // [n][1653]
    unsigned long long *d_counters = nullptr;  // [n][8]
    double *d_out = nullptr;         // [n][4] exploitability outputs
    int64_t *d_seeds = nullptr;      // [n]
    uint16_t *d_infoset_T = nullptr; // [1653][n]  node-major copies for the lane-per-deal kernel (coalesced across deals)
    int8_t *d_payoff_T = nullptr;    // [576][n]
    double *d_rows = nullptr;        // [n][1653][8]  lane-per-deal kernel's table image: one 64-byte row per infoset = regret[4] strategy[4]
    bool rows_current = false;       // the tables live in d_rows (true) or in d_regret/d_strat/d_local (false)
    uint32_t mccfr_iteration = 0;
};
