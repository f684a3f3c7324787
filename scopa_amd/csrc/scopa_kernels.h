// scopa_kernels.h -- prototypes of kernels that more than one translation unit launches (the multi-deal mode reuses
// the single-deal kernels with one workgroup per deal).
#pragma once
#include "scopa_ctx.h"

__global__ void k_tree_build(const uint8_t *__restrict__ perm16, scopa_state *__restrict__ states, uint16_t *__restrict__ infoset_of,
                             int8_t *__restrict__ payoff, uint64_t *__restrict__ key_of_infoset, int32_t *__restrict__ meta);
__global__ void k_tables_reset(double *regret, double *strat, double *local, const uint64_t *key_of_infoset, const int32_t *meta);
__global__ void k_cfr_exact(const uint16_t *__restrict__ g_infoset, const int8_t *__restrict__ g_payoff, double *__restrict__ g_regret,
                            double *__restrict__ g_strat, double *__restrict__ g_local, int n_infosets, int n_traversals,
                            int first_traverser, double *__restrict__ root_values, unsigned long long *__restrict__ g_counters,
                            int use_lds, uint32_t *__restrict__ g_visit, int32_t *__restrict__ g_meta, int start_depth, int start_idx,
                            double start_r0, double start_r1);
__global__ void k_cfr_sync(const uint16_t *__restrict__ g_infoset, const int8_t *__restrict__ g_payoff, const uint64_t *__restrict__ g_key,
                           double *__restrict__ g_regret, double *__restrict__ g_strat, int n_infosets, int n_iters,
                           unsigned long long *__restrict__ g_counters, uint32_t *__restrict__ g_visit, int32_t *__restrict__ g_meta);
__global__ void k_cfr_sync_weighted(const uint16_t *__restrict__ g_infoset, const int8_t *__restrict__ g_payoff, const uint64_t *__restrict__ g_key,
                                    double *__restrict__ g_regret, double *__restrict__ g_strat, int n_infosets, int n_iters, const double *__restrict__ g_w,
                                    int alternating, const uint8_t *__restrict__ g_active, unsigned long long *__restrict__ g_counters,
                                    uint32_t *__restrict__ g_visit, int32_t *__restrict__ g_meta);
__global__ void k_exploitability(const uint16_t *__restrict__ g_infoset, const int8_t *__restrict__ g_payoff,
                                 const uint64_t *__restrict__ g_key, const double *__restrict__ g_strat,
                                 const double *__restrict__ g_policy_in, int n_infosets, double *__restrict__ out4,
                                 double *__restrict__ g_policy_out, const int32_t *__restrict__ multi_meta);

namespace scopa {
int32_t launch_mccfr_multi(scopa_ctx *ctx, int n_deals, int max_infosets, const uint16_t *d_infoset, const int8_t *d_payoff,
                           const uint64_t *d_key, double *d_regret, double *d_strat, const int32_t *d_meta, uint32_t *d_visit,
                           unsigned long long *d_counters, uint64_t seed, uint32_t iter0, uint32_t n_iters, uint32_t batch);
// the walks of one MCCFR iteration of the chance game (scopa_chance.hip): slot b of d_delta[n_slots][1653][8] receives deal d_list[b]'s (NULL: deal b's)
// rows {dR[4], traverser visits, 0, 0, 0}; d_stamp[deal] = (serial << 20) | b; d_counters[n][2] per-deal decision and terminal visits
int32_t launch_mccfr_chance(scopa_ctx *ctx, int n_slots, int max_infosets, const uint16_t *d_infoset, const int8_t *d_payoff, const uint64_t *d_key,
                            const int32_t *d_map, const int32_t *d_meta, const double *d_R, double *d_delta, const int32_t *d_list, long long *d_stamp,
                            long long serial, unsigned long long *d_counters, uint64_t seed, uint32_t iteration, uint32_t batch);
// scopa_chance_sdcfr_traverse's launches (scopa_sdcfr.hip): the node-info image d_ninfo[n][1653] (uint2) over d_states[n][2229] at the first call
// (*ninfo_built), then k_chance_sdcfr_policy and k_chance_sdcfr_walk over the m listed deals (d_list NULL: deal = slot, m = n) with d_tables holding
// chance_sdcfr_table_bytes(m) bytes of policies and thresholds.  The caller has checked every argument; SCOPA_ELIMIT comes before any launch.
size_t chance_sdcfr_table_bytes(int slots);
size_t chance_sdcfr_walk_lds();   // dynamic + static LDS of k_chance_sdcfr_walk (k_sdcfr_walk's carving)
int32_t launch_chance_sdcfr(scopa_ctx *ctx, int n, const scopa_state *d_states, const int8_t *d_payoff, void *d_ninfo, bool *ninfo_built, int m,
                            const int32_t *d_list, void *d_tables, int traverser, int batch, const float *d_image, float *d_mem_feat, float *d_mem_regret,
                            float *d_mem_mask, uint32_t capacity, uint32_t write_base, float *d_root_values, uint32_t iteration, uint32_t b0);
// scopa_chance_sdcfr_average_policy's launches (scopa_sdcfr_avg.hip).  d_rep[n_keys] uint4 per key of `player`, ascending global id: {feature bits,
// hand nibbles, global id, legal count} of the key's representative node; d_terms holds n_snap * n_keys float4.
int32_t launch_chance_sdcfr_reps(scopa_ctx *ctx, long long G, const uint64_t *d_gkey, const int32_t *d_occ_off, const int32_t *d_occ, const uint16_t *d_infoset,
                                 const scopa_state *d_states, const int32_t *d_rank, void *d_rep0, void *d_rep1);
int32_t launch_chance_sdcfr_avg(scopa_ctx *ctx, int n_keys, const void *d_rep, int n_snap, const float *d_w1, const float *d_b1, const float *d_w2,
                                const float *d_b2, const float *d_w3, const float *d_b3, int max_size, const int32_t *d_slots, const float *d_coef, void *d_terms,
                                double *d_policy_G);
}
