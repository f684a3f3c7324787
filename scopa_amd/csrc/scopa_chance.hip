// scopa_chance.hip -- MiniScopa over a SET of deals with the deal as a chance move.
//
// Every other solver here works on one deal: its tree has no chance node, so a policy solved on it adapts to the one hand the opponent can
// hold (the reference's set-up).  The infoset key -- P{player}:H[own hand, ordered]_T[table, ordered] -- is exactly what a player
// who cannot see the other hand knows, so the same key occurs in many deals.  A scopa_chance borrows a built scopa_multi of n deals (its
// resident trees and keys; its per-deal tables are not touched), lets chance pick one deal uniformly, and identifies infosets ACROSS deals by
// key: one regret row, one strategy row and one sigma row per distinct key.  The common factor 1/n is left out of regrets and strategy sums
// (it cancels in regret matching and in the average policy) and applied to the reported values.
//
//   index (set-up, host): the keys are copied to the host once and sorted; global id = rank of the key among the distinct keys, ascending
//       unsigned.  map[n][1653] local id -> global id (-1 past the deal's count), a CSR list of occurrences deal * 1653 + local per global id in
//       ascending (deal, local) order, and per deal its local rows ordered by (ply, local id): a key fixes the player (bit 0) and the legal
//       count (bits 1-3), hence the ply, so a row's cells are summed in one ply's update and a ply only looks at its own rows.
//   k_chance_sweep   one workgroup per deal: k_cfr_sync_weighted's sweep (same LDS carving minus the regret table; the reach pass, the node values and
//       the per-cell scan are the same functions, scopa_tree_passes.h) with the deal's sigma rows gathered from the global sigma table through map.  It updates nothing: the deal's increments go to
//       delta[deal][local] as 64-byte rows {dR[4], dS[4]}.
//   k_chance_reduce  eight lanes per global row: lane k adds cell k of the occurrences' rows in CSR order, STARTING FROM THE FIRST occurrence's
//       value, then R <- R + dR; R <- !(R <= 0) ? R * pos : R * neg; S <- (S + dS) * strat and the row's sigma by regret matching.
//   No float64 atomics: every sum has a fixed order, so two runs give the same bits, and with one deal they are k_cfr_sync_weighted's bits.
//   deal-sampled iterations (scopa_chance_cfr_iterate_sampled): the caller lists m of the n deals per iteration.  k_chance_sweep with a list
//       sweeps deal list[b] into slot b of a compact [m][1653][8] image and stamps the deal with (serial << 20) | b; k_chance_reduce_sampled takes
//       an occurrence when its deal's stamp carries the sweep's serial (one per sampled (half-)sweep of the handle: no clear pass, no host round
//       trip), reads its row from the stamp's slot and sums in the same CSR order from the first sampled value, +0.0 where a row has none; the
//       update is the full iteration's for every row.  Increments are not scaled by n / m.  m = n gives k_chance_reduce's bits.
//   MCCFR iterations (scopa_chance_mccfr_iterate): external-sampling MCCFR with chance sampled too.  k_mccfr_chance (scopa_mccfr.hip: the batched
//       walk, one workgroup per listed deal) freezes the deal's rows from the shared regrets, walks `batch` traversal pairs with global traversal ids
//       deal * batch + i and leaves rows {dR[4], traverser visits, 0, 0, 0} in its slot of the same image, stamping the deal as the sampled sweep
//       does; k_chance_reduce_mccfr sums a row's stamped occurrences in CSR order from the first (lanes 0-3 the regret cells, lane 4 the visits, an
//       exact integer sum), R += dR, S += visits * mc_sigma(old R), refreshes the row's sigma, and leaves a row with no listed occurrence alone.
//       The only sums in arrival order are the LDS atomics of a workgroup's walks: reproducible to rounding, not bit for bit.
//
// Traffic of an iteration is the delta rows, written once and read once.  Both sides move whole rows: in the sweep a wavefront computes 16 rows
// (lane = row * 4 + action, holding dR and dS of its cell) and a shuffle turns them into two stores of 8 rows x 64 contiguous bytes; in the
// reduce the eight lanes of a row read the 64 bytes of an occurrence in one instruction.
//
// Exploitability across deals follows k_exploitability with q summed over all deals (the kernels and the pass loop are scopa_chance_xplay.hip's,
// run on one policy): reach and node values per deal persist in HBM between launches; on a responder ply the per-deal q (nodes ascending from 0.0) is reduced over the occurrences in CSR order from the first, the argmax
// taken (ties to the lowest action) and the values selected; any other ply takes sigma-weighted values.
#include <algorithm>
#include <new>
#include <vector>

#include "scopa_chance.h"
#include "scopa_kernels.h"
#include "scopa_mccfr_sigma.h"
#include "scopa_tree_passes.h"

using namespace scopa;

// sigma of every global row from its regrets (after a reset or a tables_set; the reduce keeps it current afterwards)
__global__ void __launch_bounds__(256) k_chance_sigma(const uint64_t *__restrict__ gkey, const double *__restrict__ R, double *__restrict__ sig, long long G) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    const int n = (int)((gkey[g] >> 1) & 7);
    double r[4], o[4] = {0.0, 0.0, 0.0, 0.0};
    for (int c = 0; c < 4; c++) r[c] = R[g * 4 + c];
    regret_match_n(n, r, o);
    for (int c = 0; c < 4; c++) sig[g * 4 + c] = o[c];
}

// only_player: -1 both players' plies, else the plies of that player alone (the alternating form's sweep).
// list == NULL: workgroup b sweeps deal b into delta[b].  Else (a sampled iteration) workgroup b sweeps deal list[b] into slot b of the compact
// image delta[m][1653][8] and stamps the deal with (serial << 20) | b for the reduce that follows.
__global__ void __launch_bounds__(1024)
k_chance_sweep(const uint16_t *__restrict__ g_infoset, const int8_t *__restrict__ g_payoff, const int32_t *__restrict__ g_map, const uint16_t *__restrict__ g_order,
               const int32_t *__restrict__ g_plyoff, const int32_t *__restrict__ g_meta, const double *__restrict__ g_sig /*[G][4]*/,
               double *__restrict__ g_delta /*[n][1653][8]*/, int only_player, const int32_t *__restrict__ list /*[gridDim.x] or NULL*/,
               long long *__restrict__ stamp /*[n]*/, long long serial) {
    extern __shared__ __align__(16) unsigned char smem[];
    const size_t slot = blockIdx.x, deal = list ? (size_t)list[slot] : slot;
    g_infoset += deal * kDecision; g_payoff += deal * kTerminal; g_map += deal * kDecision; g_order += deal * 1656; g_plyoff += deal * 12;
    g_delta += slot * kDecision * 8;
    if (list && threadIdx.x == 0) stamp[deal] = (serial << 20) | (long long)slot;
    const int I = g_meta[deal * 8], tid = threadIdx.x, nt = blockDim.x, lane = tid & 63;
    double *s_sig = reinterpret_cast<double *>(smem);   // [I][4]
    double *s_r0 = s_sig + (size_t)I * 4;               // [kNodes] reach of player 0 (BFS order)
    double *s_r1 = s_r0 + kNodes;                       // [kNodes]
    double *s_val = s_r1 + kNodes;                      // [kNodes] value for player 0
    uint16_t *s_inf = reinterpret_cast<uint16_t *>(s_val + kNodes);   // [1656]
    uint16_t *s_ord = s_inf + 1656;                     // [1656]
    for (int i = tid; i < I * 4; i += nt) s_sig[i] = g_sig[(size_t)g_map[i >> 2] * 4 + (i & 3)];   // four lanes per 32-byte row
    for (int i = tid; i < kDecision; i += nt) s_inf[i] = g_infoset[i];
    for (int i = tid; i < I; i += nt) s_ord[i] = g_order[i];
    if (tid == 0) { s_r0[0] = 1.0; s_r1[0] = 1.0; }
    __syncthreads();
    sync_reach_pass(s_sig, s_inf, s_r0, s_r1, tid, nt);
    sync_terminal_values(g_payoff, s_val, tid, nt);
    __syncthreads();
#pragma unroll   // as in cfr_sync_body (scopa_eval.hip): a ply's width, offsets and legal count are constants of its copy
    for (int d = kPlies - 1; d >= 0; d--) {  // values bottom up, then this ply's increments
        const int n = nlegal_at(d), p = d & 1;
        ply_node_values(d, s_sig, s_inf, s_val, tid, nt);
        __syncthreads();
        if (only_player >= 0 && p != only_player) continue;   // uniform
        const int row0 = g_plyoff[d], cells = (g_plyoff[d + 1] - row0) * 4;
        for (int base = 0; base < cells; base += nt) {        // uniform trip count: every lane of a wavefront takes part in the shuffles
            const int cell = base + tid, a = cell & 3;
            const bool live = cell < cells;
            const int r = live ? (int)s_ord[row0 + (cell >> 2)] : 0;
            double dR = 0.0, dS = 0.0;
            if (live && a < n) sync_cell_scan(d, r, a, s_sig, s_inf, s_r0, s_r1, s_val, dR, dS);
            // lane = row * 4 + action holds (dR, dS): two stores of 8 rows x {dR[4], dS[4]}, 64 contiguous bytes per row
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int src = h * 32 + (lane >> 3) * 4 + (lane & 3);
                const double vR = __shfl(dR, src, 64), vS = __shfl(dS, src, 64);
                const int rr = __shfl(r, src, 64), ok = __shfl((int)live, src, 64);
                if (ok) g_delta[(size_t)rr * 8 + (lane & 7)] = (lane & 4) ? vS : vR;
            }
        }
        __syncthreads();
    }
}

// eight lanes per global row: lanes 0-3 the regret cells, 4-7 the strategy cells.  w = (pos, neg, strat) of the iteration at hand.
// The update of cell k of row g by its summed increment `acc`, and the row's sigma; every lane of the wavefront calls it (shuffles).
__device__ __forceinline__ void chance_apply(long long g, int k, int n, bool act, double acc, double *__restrict__ R, double *__restrict__ S, double *__restrict__ sig,
                                             const double *__restrict__ w) {
    const int a = k & 3, lane = threadIdx.x & 63;
    double regret = 0.0;
    if (act && a < n) {
        if (k < 4) {
            const double r = R[g * 4 + a] + acc;
            regret = !(r <= 0.0) ? r * w[0] : r * w[1];
            R[g * 4 + a] = regret;
        } else {
            S[g * 4 + a] = (S[g * 4 + a] + acc) * w[2];
        }
    }
    const double pos = !(regret <= 0.0) ? regret : 0.0;   // lanes 0-3 of a row; cells past the legal count are not summed below
    const int l0 = lane & ~7;
    const double p0 = __shfl(pos, l0, 64), p1 = __shfl(pos, l0 + 1, 64), p2 = __shfl(pos, l0 + 2, 64), p3 = __shfl(pos, l0 + 3, 64);
    double s = p0;
    if (n > 1) s += p1;
    if (n > 2) s += p2;
    if (n > 3) s += p3;
    if (act && k < 4) sig[g * 4 + a] = a < n ? (s > 0.0 ? pos / s : 1.0 / (double)n) : 0.0;
}

__global__ void __launch_bounds__(256)
k_chance_reduce(const uint64_t *__restrict__ gkey, const int32_t *__restrict__ occ_off, const int32_t *__restrict__ occ, const double *__restrict__ delta,
                double *__restrict__ R, double *__restrict__ S, double *__restrict__ sig, long long G, const double *__restrict__ w, int only_player) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long g = t >> 3;
    const int k = (int)(t & 7);
    const uint64_t key = g < G ? gkey[g] : 0;
    const int n = (int)((key >> 1) & 7);
    const bool act = g < G && (only_player < 0 || (int)(key & 1) == only_player);
    double acc = 0.0;
    if (act) {
        const int b = occ_off[g], e = occ_off[g + 1];
        acc = delta[(size_t)occ[b] * 8 + k];
        for (int i = b + 1; i < e; i++) acc += delta[(size_t)occ[i] * 8 + k];
    }
    chance_apply(g, k, n, act, acc, R, S, sig, w);
}

// the reduce of a sampled iteration: an occurrence counts when its deal's stamp carries this sweep's serial, and its row is read from the slot
// the stamp names.  Same CSR order, from the first SAMPLED occurrence's value; a row with none takes +0.0 and is updated like every other row.
__global__ void __launch_bounds__(256)
k_chance_reduce_sampled(const uint64_t *__restrict__ gkey, const int32_t *__restrict__ occ_off, const int32_t *__restrict__ occ, const double *__restrict__ delta /*[m][1653][8]*/,
                        const long long *__restrict__ stamp /*[n]*/, long long serial, double *__restrict__ R, double *__restrict__ S, double *__restrict__ sig, long long G,
                        const double *__restrict__ w, int only_player) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long g = t >> 3;
    const int k = (int)(t & 7);
    const uint64_t key = g < G ? gkey[g] : 0;
    const int n = (int)((key >> 1) & 7);
    const bool act = g < G && (only_player < 0 || (int)(key & 1) == only_player);
    double acc = 0.0;
    if (act) {
        const int b = occ_off[g], e = occ_off[g + 1];
        bool any = false;
        for (int i = b; i < e; i++) {
            const int o = occ[i], deal = o / kDecision;
            const long long st = stamp[deal];
            if ((st >> 20) != serial) continue;
            const double v = delta[((size_t)(st & 0xFFFFF) * kDecision + (size_t)(o - deal * kDecision)) * 8 + k];
            acc = any ? acc + v : v;
            any = true;
        }
    }
    chance_apply(g, k, n, act, acc, R, S, sig, w);
}

// the reduce of an MCCFR iteration (k_mccfr_chance's rows {dR[4], traverser visits, 0, 0, 0}): eight lanes per global row, lanes 0-3 the regret
// cells, lane 4 the visits, over the occurrences whose deal's stamp carries the serial, in CSR order from the first.  R += dR;
// S += visits * mc_sigma(old R) -- the row's frozen strategy: every listed deal sampled from it -- for the legal cells; the row's sigma by
// regret_match, as the other reduces leave it.  A row with no listed occurrence keeps its bits.  Every lane reaches the shuffles.
__global__ void __launch_bounds__(256)
k_chance_reduce_mccfr(const uint64_t *__restrict__ gkey, const int32_t *__restrict__ occ_off, const int32_t *__restrict__ occ, const double *__restrict__ delta /*[m][1653][8]*/,
                      const long long *__restrict__ stamp /*[n]*/, long long serial, double *__restrict__ R, double *__restrict__ S, double *__restrict__ sig, long long G) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long g = t >> 3;
    const int k = (int)(t & 7), lane = threadIdx.x & 63, l0 = lane & ~7;
    const int n = g < G ? (int)((gkey[g] >> 1) & 7) : 0;
    double acc = 0.0;
    bool any = false;
    if (g < G) {
        const int b = occ_off[g], e = occ_off[g + 1];
        for (int i = b; i < e; i++) {
            const int o = occ[i], deal = o / kDecision;
            const long long st = stamp[deal];
            if ((st >> 20) != serial) continue;
            const double v = k < 5 ? delta[((size_t)(st & 0xFFFFF) * kDecision + (size_t)(o - deal * kDecision)) * 8 + k] : 0.0;
            acc = any ? acc + v : v;   // lane 4: integers far below 2^53, the sum is exact
            any = true;
        }
    }
    double old[4] = {0.0, 0.0, 0.0, 0.0}, sg[4];
    if (any) for (int c = 0; c < 4; c++) old[c] = R[g * 4 + c];
    mc_sigma(old, n, sg);
    const double visits = __shfl(acc, l0 + 4, 64);
    auto at = [k](const double (&v)[4]) { return k == 0 ? v[0] : k == 1 ? v[1] : k == 2 ? v[2] : v[3]; };   // selects: a run-time index would put the rows in scratch memory
    double regret = at(old);
    if (any && k < n) {   // n <= 4: lanes 0-3 of the row
        regret += acc;
        R[g * 4 + k] = regret;
        S[g * 4 + k] += visits * at(sg);
    }
    double now[4], out[4] = {0.0, 0.0, 0.0, 0.0};
    for (int c = 0; c < 4; c++) now[c] = __shfl(regret, l0 + c, 64);
    regret_match_n(n, now, out);
    if (any && k < 4) sig[g * 4 + k] = at(out);
}

// ---- exploitability across deals ---------------------------------------------------------------------------------------------------------
// the evaluated policy: given, or the average of the global strategy table, uniform where nothing was accumulated
__global__ void __launch_bounds__(256) k_chance_policy(const uint64_t *__restrict__ gkey, const double *__restrict__ S, const double *__restrict__ pin,
                                                       double *__restrict__ pol, long long G) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    const int n = (int)((gkey[g] >> 1) & 7);
    double p[4] = {0.0, 0.0, 0.0, 0.0};
    if (pin) {
        for (int c = 0; c < 4; c++) p[c] = pin[g * 4 + c];
    } else {
        double s = S[g * 4];
        for (int c = 1; c < n; c++) s += S[g * 4 + c];
        for (int c = 0; c < n; c++) p[c] = s > 0.0 ? S[g * 4 + c] / s : 1.0 / (double)n;
    }
    for (int c = 0; c < 4; c++) pol[g * 4 + c] = p[c];
}

__global__ void __launch_bounds__(256) k_chance_scatter(const int32_t *__restrict__ g_map, const double *__restrict__ pol_G, double *__restrict__ pol_local, int I) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;   // over I * 4
    if (i < I * 4) pol_local[i] = pol_G[(size_t)g_map[i >> 2] * 4 + (i & 3)];
}

namespace {
size_t sweep_lds(int max_infosets) { return (size_t)max_infosets * 4 * 8 + sizeof(double) * kNodes * 3 + 1656 * 2 * 2; }

int32_t chance_sigma(scopa_chance *g) {
    hipLaunchKernelGGL(k_chance_sigma, dim3((unsigned)((g->G + 255) / 256)), dim3(256), 0, g->ctx->stream, g->d_gkey, g->d_R, g->d_sig, g->G);
    SC_HIP(g->ctx, hipGetLastError());
    return SCOPA_OK;
}

// the weights of a call, once: h_w[n_iters][3] or NULL = all ones, into g->d_w (grown as needed); synchronises the stream
int32_t chance_upload_weights(scopa_chance *g, int32_t n_iters, const double *h_w, const char *no_memory) {
    scopa_ctx *ctx = g->ctx;
    if ((size_t)n_iters > g->w_cap) {
        SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (g->d_w) { (void)hipFree(g->d_w); g->d_w = nullptr; g->w_cap = 0; }
        if (hipMalloc(&g->d_w, (size_t)n_iters * 24) != hipSuccess) return fail(ctx, SCOPA_ENOMEM, no_memory);
        g->w_cap = (size_t)n_iters;
    }
    std::vector<double> ones;
    if (!h_w) { ones.assign((size_t)n_iters * 3, 1.0); h_w = ones.data(); }
    SC_HIP(ctx, hipMemcpyAsync(g->d_w, h_w, (size_t)n_iters * 24, hipMemcpyHostToDevice, ctx->stream));
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));   // `ones` (and a caller's pageable rows) may go away after this
    return SCOPA_OK;
}

// every list of a call: ids in [0, n), no id twice within an iteration
bool chance_lists_ok(int n, int32_t n_iters, int32_t m_deals, const int32_t *h_deals) {
    std::vector<int32_t> seen((size_t)n, -1);
    for (int it = 0; it < n_iters; it++)
        for (int s = 0; s < m_deals; s++) {
            const int32_t d = h_deals[(size_t)it * m_deals + s];
            if (d < 0 || d >= n || seen[(size_t)d] == it) return false;
            seen[(size_t)d] = it;
        }
    return true;
}

// the stamps of the listed deals, zeroed at first use (serial 0 is never used)
int32_t chance_ensure_stamps(scopa_chance *g, const char *no_memory) {
    scopa_ctx *ctx = g->ctx;
    if (g->d_stamp) return SCOPA_OK;
    if (hipMalloc(&g->d_stamp, (size_t)g->n * 8) != hipSuccess) { g->d_stamp = nullptr; return fail(ctx, SCOPA_ENOMEM, no_memory); }
    SC_HIP(ctx, hipMemsetAsync(g->d_stamp, 0, (size_t)g->n * 8, ctx->stream));
    return SCOPA_OK;
}

// the deal lists of a call, once, into g->d_list (grown as needed); synchronises the stream: a caller's pageable rows may go away after this
int32_t chance_upload_lists(scopa_chance *g, size_t n_ids, const int32_t *h_deals, const char *no_memory) {
    scopa_ctx *ctx = g->ctx;
    if (n_ids > g->list_cap) {
        SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (g->d_list) { (void)hipFree(g->d_list); g->d_list = nullptr; g->list_cap = 0; }
        if (hipMalloc(&g->d_list, n_ids * 4) != hipSuccess) { g->d_list = nullptr; return fail(ctx, SCOPA_ENOMEM, no_memory); }
        g->list_cap = n_ids;
    }
    SC_HIP(ctx, hipMemcpyAsync(g->d_list, h_deals, n_ids * 4, hipMemcpyHostToDevice, ctx->stream));
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SCOPA_OK;
}
}  // namespace

extern "C" {

int32_t scopa_chance_destroy(scopa_chance *g);

int32_t scopa_chance_create(scopa_multi *m, scopa_chance **out) {
    if (!m || !out) return SCOPA_EINVAL;
    *out = nullptr;
    scopa_ctx *ctx = m->ctx;
    SC_REQUIRE(ctx, m->built, SCOPA_ESTATE, "scopa_chance_create: call scopa_multi_build first");
    SC_REQUIRE(ctx, m->n <= kChanceMaxDeals, SCOPA_ELIMIT, "scopa_chance_create: more than 65536 deals");
    SC_REQUIRE(ctx, sweep_lds(m->max_infosets) <= (size_t)ctx->lds_limit, SCOPA_ELIMIT, "scopa_chance_create: a deal's sigma rows do not fit in LDS");
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const int n = m->n;
    std::vector<uint64_t> keys((size_t)n * kDecision);
    std::vector<int32_t> meta((size_t)n * 8);
    std::vector<uint16_t> inf((size_t)n * kDecision);
    SC_HIP(ctx, hipMemcpyAsync(keys.data(), m->d_key, keys.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    SC_HIP(ctx, hipMemcpyAsync(meta.data(), m->d_meta, meta.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    SC_HIP(ctx, hipMemcpyAsync(inf.data(), m->d_infoset, inf.size() * 2, hipMemcpyDeviceToHost, ctx->stream));
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));

    scopa_chance *g = new (std::nothrow) scopa_chance();
    if (!g) return SCOPA_ENOMEM;
    g->m = m; g->ctx = ctx; g->n = n;
    // a key fixes the player and the legal count, hence the ply: every node's infoset must carry the key of the node's own ply
    for (int deal = 0; deal < n; deal++) {
        const int I = meta[(size_t)deal * 8];
        for (int d = 0; d < kPlies; d++)
            for (int j = 0; j < level_width(d); j++) {
                const int r = inf[(size_t)deal * kDecision + level_offset(d) + j];
                const uint64_t key = r < I ? keys[(size_t)deal * kDecision + r] : ~0ull;
                if (r >= I || (int)(key & 1) != (d & 1) || (int)((key >> 1) & 7) != nlegal_at(d)) {
                    delete g;
                    return fail(ctx, SCOPA_ESTATE, "scopa_chance_create: an infoset key does not belong to its node's ply");
                }
            }
    }
    std::vector<uint64_t> &gk = g->h_gkey;
    for (int deal = 0; deal < n; deal++)
        gk.insert(gk.end(), keys.begin() + (size_t)deal * kDecision, keys.begin() + (size_t)deal * kDecision + meta[(size_t)deal * 8]);
    g->n_occ = (long long)gk.size();
    std::sort(gk.begin(), gk.end());
    gk.erase(std::unique(gk.begin(), gk.end()), gk.end());
    g->G = (long long)gk.size();
    g->h_map.assign((size_t)n * kDecision, -1);
    std::vector<int32_t> occ_off((size_t)g->G + 1, 0), occ((size_t)g->n_occ), plyoff((size_t)n * 12, 0);
    std::vector<uint16_t> order((size_t)n * 1656, 0);
    for (int deal = 0; deal < n; deal++)
        for (int r = 0; r < meta[(size_t)deal * 8]; r++) {
            const int32_t gid = (int32_t)(std::lower_bound(gk.begin(), gk.end(), keys[(size_t)deal * kDecision + r]) - gk.begin());
            g->h_map[(size_t)deal * kDecision + r] = gid;
            occ_off[(size_t)gid + 1]++;
        }
    for (long long i = 0; i < g->G; i++) occ_off[(size_t)i + 1] += occ_off[(size_t)i];
    {
        std::vector<int32_t> at(occ_off.begin(), occ_off.end() - 1);
        for (int deal = 0; deal < n; deal++)   // ascending (deal, local id)
            for (int r = 0; r < meta[(size_t)deal * 8]; r++) occ[(size_t)at[(size_t)g->h_map[(size_t)deal * kDecision + r]]++] = deal * kDecision + r;
    }
    for (int deal = 0; deal < n; deal++) {   // the deal's rows by (ply, local id): ply = 2 * (4 - legal count) + player
        const int I = meta[(size_t)deal * 8];
        int32_t *po = plyoff.data() + (size_t)deal * 12;
        auto ply_of = [&](int r) { const uint64_t key = keys[(size_t)deal * kDecision + r]; return 2 * (4 - (int)((key >> 1) & 7)) + (int)(key & 1); };
        for (int r = 0; r < I; r++) po[ply_of(r) + 1]++;
        for (int d = 0; d < kPlies; d++) po[d + 1] += po[d];
        int at[kPlies];
        for (int d = 0; d < kPlies; d++) at[d] = po[d];
        for (int r = 0; r < I; r++) order[(size_t)deal * 1656 + at[ply_of(r)]++] = (uint16_t)r;
    }

    const size_t Gs = (size_t)g->G;
    bool ok = hipMalloc(&g->d_gkey, Gs * 8) == hipSuccess && hipMalloc(&g->d_map, (size_t)n * kDecision * 4) == hipSuccess &&
              hipMalloc(&g->d_occ_off, (Gs + 1) * 4) == hipSuccess && hipMalloc(&g->d_occ, (size_t)g->n_occ * 4) == hipSuccess &&
              hipMalloc(&g->d_order, (size_t)n * 1656 * 2) == hipSuccess && hipMalloc(&g->d_plyoff, (size_t)n * 12 * 4) == hipSuccess &&
              hipMalloc(&g->d_R, Gs * 32) == hipSuccess && hipMalloc(&g->d_S, Gs * 32) == hipSuccess && hipMalloc(&g->d_sig, Gs * 32) == hipSuccess &&
              hipMalloc(&g->d_delta, (size_t)n * kDecision * 64) == hipSuccess && hipMalloc(&g->d_out, 64) == hipSuccess;
    if (!ok) { scopa_chance_destroy(g); return fail(ctx, SCOPA_ENOMEM, "scopa_chance_create: device allocation failed"); }
    ok = hipMemcpyAsync(g->d_gkey, gk.data(), Gs * 8, hipMemcpyHostToDevice, ctx->stream) == hipSuccess &&
         hipMemcpyAsync(g->d_map, g->h_map.data(), g->h_map.size() * 4, hipMemcpyHostToDevice, ctx->stream) == hipSuccess &&
         hipMemcpyAsync(g->d_occ_off, occ_off.data(), occ_off.size() * 4, hipMemcpyHostToDevice, ctx->stream) == hipSuccess &&
         hipMemcpyAsync(g->d_occ, occ.data(), occ.size() * 4, hipMemcpyHostToDevice, ctx->stream) == hipSuccess &&
         hipMemcpyAsync(g->d_order, order.data(), order.size() * 2, hipMemcpyHostToDevice, ctx->stream) == hipSuccess &&
         hipMemcpyAsync(g->d_plyoff, plyoff.data(), plyoff.size() * 4, hipMemcpyHostToDevice, ctx->stream) == hipSuccess &&
         hipMemsetAsync(g->d_delta, 0, (size_t)n * kDecision * 64, ctx->stream) == hipSuccess &&
         hipMemsetAsync(g->d_R, 0, Gs * 32, ctx->stream) == hipSuccess && hipMemsetAsync(g->d_S, 0, Gs * 32, ctx->stream) == hipSuccess &&
         hipStreamSynchronize(ctx->stream) == hipSuccess;   // the host vectors go out of scope below
    if (!ok) { scopa_chance_destroy(g); return fail(ctx, SCOPA_EHIP, "scopa_chance_create: upload of the index failed"); }
    { const int32_t rc = chance_sigma(g); if (rc != SCOPA_OK) { scopa_chance_destroy(g); return rc; } }
    *out = g;
    return SCOPA_OK;
}

int32_t scopa_chance_destroy(scopa_chance *g) {
    if (!g) return SCOPA_EINVAL;
    (void)hipSetDevice(g->ctx->device);
    (void)hipStreamSynchronize(g->ctx->stream);
    void *bufs[] = {g->d_gkey, g->d_map, g->d_occ_off, g->d_occ, g->d_order, g->d_plyoff, g->d_R, g->d_S, g->d_sig, g->d_delta, g->d_reach, g->d_val,
                    g->d_pol, g->d_pin, g->d_choice, g->d_out, g->d_w, g->d_list, g->d_stamp, g->d_mc_visits, g->d_xp_img, g->d_xbr, g->d_xmatch};
    for (void *b : bufs) if (b) (void)hipFree(b);
    void *sd_bufs[] = {g->d_sdninfo, g->d_sdtab, g->d_sdlist, g->d_sdrep[0], g->d_sdrep[1], g->d_sdterms};
    for (void *b : sd_bufs) if (b) (void)hipFree(b);
    if (g->h_sdlist) (void)hipHostFree(g->h_sdlist);
    for (hipEvent_t e : g->sd_ev) if (e) (void)hipEventDestroy(e);
    delete g;
    return SCOPA_OK;
}

int32_t scopa_chance_counts(scopa_chance *g, int32_t *n_deals, int64_t *n_global, int64_t *n_occurrences) {
    if (!g) return SCOPA_EINVAL;
    if (n_deals) *n_deals = g->n;
    if (n_global) *n_global = g->G;
    if (n_occurrences) *n_occurrences = g->n_occ;
    return SCOPA_OK;
}

int32_t scopa_chance_index_get(scopa_chance *g, uint64_t *h_keys, int32_t *h_map) {
    if (!g) return SCOPA_EINVAL;
    if (h_keys) std::copy(g->h_gkey.begin(), g->h_gkey.end(), h_keys);
    if (h_map) std::copy(g->h_map.begin(), g->h_map.end(), h_map);
    return SCOPA_OK;
}

int32_t scopa_chance_tables_reset(scopa_chance *g) {
    if (!g) return SCOPA_EINVAL;
    scopa_ctx *ctx = g->ctx;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    SC_HIP(ctx, hipMemsetAsync(g->d_R, 0, (size_t)g->G * 32, ctx->stream));
    SC_HIP(ctx, hipMemsetAsync(g->d_S, 0, (size_t)g->G * 32, ctx->stream));
    if (int32_t rc = chance_sigma(g)) return rc;
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SCOPA_OK;
}

int32_t scopa_chance_tables_get(scopa_chance *g, double *h_regret, double *h_strategy) {
    if (!g) return SCOPA_EINVAL;
    scopa_ctx *ctx = g->ctx;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    if (h_regret) SC_HIP(ctx, hipMemcpyAsync(h_regret, g->d_R, (size_t)g->G * 32, hipMemcpyDeviceToHost, ctx->stream));
    if (h_strategy) SC_HIP(ctx, hipMemcpyAsync(h_strategy, g->d_S, (size_t)g->G * 32, hipMemcpyDeviceToHost, ctx->stream));
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SCOPA_OK;
}

int32_t scopa_chance_tables_set(scopa_chance *g, const double *h_regret, const double *h_strategy) {
    if (!g) return SCOPA_EINVAL;
    scopa_ctx *ctx = g->ctx;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    if (h_regret) SC_HIP(ctx, hipMemcpyAsync(g->d_R, h_regret, (size_t)g->G * 32, hipMemcpyHostToDevice, ctx->stream));
    if (h_strategy) SC_HIP(ctx, hipMemcpyAsync(g->d_S, h_strategy, (size_t)g->G * 32, hipMemcpyHostToDevice, ctx->stream));
    if (h_regret) { if (int32_t rc = chance_sigma(g)) return rc; }
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SCOPA_OK;
}

int32_t scopa_chance_cfr_iterate_weighted(scopa_chance *g, int32_t n_iters, const double *h_w, int32_t alternating) {
    if (!g || n_iters < 0 || n_iters > (1 << 20) || (alternating != 0 && alternating != 1) || (h_w && !cfr_weights_ok(h_w, n_iters))) return SCOPA_EINVAL;
    scopa_ctx *ctx = g->ctx;
    scopa_multi *m = g->m;
    if (!n_iters) return SCOPA_OK;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t lds = sweep_lds(m->max_infosets);
    SC_REQUIRE(ctx, lds <= (size_t)ctx->lds_limit, SCOPA_ELIMIT, "scopa_chance_cfr_iterate_weighted: a deal's sigma rows do not fit in LDS");
    if (int32_t rc = chance_upload_weights(g, n_iters, h_w, "scopa_chance_cfr_iterate_weighted: no device memory for the weights")) return rc;
    SC_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(k_chance_sweep), hipFuncAttributeMaxDynamicSharedMemorySize, ctx->lds_limit));
    const unsigned reduce_blocks = (unsigned)((g->G * 8 + 255) / 256);
    for (int it = 0; it < n_iters; it++)   // sweep + reduce per (half-)iteration on the context's stream, no host synchronisation in between
        for (int sweep = 0; sweep < (alternating ? 2 : 1); sweep++) {
            const int only = alternating ? sweep : -1;
            hipLaunchKernelGGL(k_chance_sweep, dim3(g->n), dim3(1024), lds, ctx->stream, m->d_infoset, m->d_payoff, g->d_map, g->d_order, g->d_plyoff, m->d_meta,
                               (const double *)g->d_sig, g->d_delta, only, (const int32_t *)nullptr, (long long *)nullptr, 0ll);
            hipLaunchKernelGGL(k_chance_reduce, dim3(reduce_blocks), dim3(256), 0, ctx->stream, g->d_gkey, g->d_occ_off, g->d_occ, (const double *)g->d_delta,
                               g->d_R, g->d_S, g->d_sig, g->G, (const double *)(g->d_w + (size_t)it * 3), only);
        }
    SC_HIP(ctx, hipGetLastError());
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SCOPA_OK;
}

int32_t scopa_chance_cfr_iterate_sampled(scopa_chance *g, int32_t n_iters, int32_t m_deals, const int32_t *h_deals, const double *h_w, int32_t alternating) {
    if (!g || n_iters < 0 || n_iters > (1 << 20) || m_deals < 1 || m_deals > g->n || (n_iters > 0 && !h_deals) || (alternating != 0 && alternating != 1) ||
        (h_w && !cfr_weights_ok(h_w, n_iters)))
        return SCOPA_EINVAL;
    if (!chance_lists_ok(g->n, n_iters, m_deals, h_deals)) return SCOPA_EINVAL;
    scopa_ctx *ctx = g->ctx;
    scopa_multi *m = g->m;
    if (!n_iters) return SCOPA_OK;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t lds = sweep_lds(m->max_infosets);
    SC_REQUIRE(ctx, lds <= (size_t)ctx->lds_limit, SCOPA_ELIMIT, "scopa_chance_cfr_iterate_sampled: a deal's sigma rows do not fit in LDS");
    if (int32_t rc = chance_ensure_stamps(g, "scopa_chance_cfr_iterate_sampled: no device memory for the stamps")) return rc;
    if (int32_t rc = chance_upload_lists(g, (size_t)n_iters * (size_t)m_deals, h_deals, "scopa_chance_cfr_iterate_sampled: no device memory for the lists")) return rc;   // once
    if (int32_t rc = chance_upload_weights(g, n_iters, h_w, "scopa_chance_cfr_iterate_sampled: no device memory for the weights")) return rc;
    SC_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(k_chance_sweep), hipFuncAttributeMaxDynamicSharedMemorySize, ctx->lds_limit));
    const unsigned reduce_blocks = (unsigned)((g->G * 8 + 255) / 256);
    for (int it = 0; it < n_iters; it++)   // as in the weighted call: no host synchronisation in between
        for (int sweep = 0; sweep < (alternating ? 2 : 1); sweep++) {
            const int only = alternating ? sweep : -1;
            const long long serial = ++g->serial;
            hipLaunchKernelGGL(k_chance_sweep, dim3(m_deals), dim3(1024), lds, ctx->stream, m->d_infoset, m->d_payoff, g->d_map, g->d_order, g->d_plyoff, m->d_meta,
                               (const double *)g->d_sig, g->d_delta, only, (const int32_t *)(g->d_list + (size_t)it * m_deals), g->d_stamp, serial);
            hipLaunchKernelGGL(k_chance_reduce_sampled, dim3(reduce_blocks), dim3(256), 0, ctx->stream, g->d_gkey, g->d_occ_off, g->d_occ, (const double *)g->d_delta,
                               (const long long *)g->d_stamp, serial, g->d_R, g->d_S, g->d_sig, g->G, (const double *)(g->d_w + (size_t)it * 3), only);
        }
    SC_HIP(ctx, hipGetLastError());
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SCOPA_OK;
}

int32_t scopa_chance_mccfr_iterate(scopa_chance *g, int32_t n_iters, uint32_t batch, uint64_t seed, int32_t m_deals, const int32_t *h_deals) {
    if (!g || n_iters < 0 || n_iters > (1 << 20) || batch == 0 || batch > (1u << 24) || (unsigned long long)g->n * batch > (1ull << 32)) return SCOPA_EINVAL;
    if (h_deals && (m_deals < 1 || m_deals > g->n || !chance_lists_ok(g->n, n_iters, m_deals, h_deals))) return SCOPA_EINVAL;
    scopa_ctx *ctx = g->ctx;
    scopa_multi *m = g->m;
    if (!n_iters) return SCOPA_OK;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    if (int32_t rc = chance_ensure_stamps(g, "scopa_chance_mccfr_iterate: no device memory for the stamps")) return rc;
    if (!g->d_mc_visits) {
        if (hipMalloc(&g->d_mc_visits, (size_t)g->n * 16) != hipSuccess) { g->d_mc_visits = nullptr; return fail(ctx, SCOPA_ENOMEM, "scopa_chance_mccfr_iterate: no device memory for the visit counters"); }
        SC_HIP(ctx, hipMemsetAsync(g->d_mc_visits, 0, (size_t)g->n * 16, ctx->stream));
    }
    const int slots = h_deals ? m_deals : g->n;
    if (h_deals) {   // the lists, once
        if (int32_t rc = chance_upload_lists(g, (size_t)n_iters * (size_t)m_deals, h_deals, "scopa_chance_mccfr_iterate: no device memory for the lists")) return rc;
    }
    const unsigned reduce_blocks = (unsigned)((g->G * 8 + 255) / 256);
    for (int it = 0; it < n_iters; it++) {   // walks + reduce per iteration on the context's stream, no host synchronisation in between
        const long long serial = ++g->serial;
        if (int32_t rc = launch_mccfr_chance(ctx, slots, m->max_infosets, m->d_infoset, m->d_payoff, m->d_key, g->d_map, m->d_meta, g->d_R, g->d_delta,
                                             h_deals ? g->d_list + (size_t)it * m_deals : nullptr, g->d_stamp, serial, g->d_mc_visits, seed,
                                             g->mccfr_iteration, batch))
            return rc;   // SCOPA_ELIMIT comes from the first launch: nothing has run
        hipLaunchKernelGGL(k_chance_reduce_mccfr, dim3(reduce_blocks), dim3(256), 0, ctx->stream, g->d_gkey, g->d_occ_off, g->d_occ, (const double *)g->d_delta,
                           (const long long *)g->d_stamp, serial, g->d_R, g->d_S, g->d_sig, g->G);
        g->mccfr_iteration++;
    }
    SC_HIP(ctx, hipGetLastError());
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SCOPA_OK;
}

int32_t scopa_chance_mccfr_counters(scopa_chance *g, uint64_t *decision_visits, uint64_t *terminal_visits, uint32_t *iteration) {
    if (!g) return SCOPA_EINVAL;
    scopa_ctx *ctx = g->ctx;
    unsigned long long a = 0, b = 0;
    if (g->d_mc_visits) {
        std::vector<unsigned long long> h((size_t)g->n * 2);
        SC_HIP(ctx, hipSetDevice(ctx->device));
        SC_HIP(ctx, hipMemcpyAsync(h.data(), g->d_mc_visits, h.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
        SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (int d = 0; d < g->n; d++) { a += h[(size_t)d * 2]; b += h[(size_t)d * 2 + 1]; }
    }
    if (decision_visits) *decision_visits = a;
    if (terminal_visits) *terminal_visits = b;
    if (iteration) *iteration = g->mccfr_iteration;
    return SCOPA_OK;
}

int32_t scopa_chance_exploitability(scopa_chance *g, const double *h_policy, double *h_out4, double *h_policy_out) {
    if (!g || !h_out4) return SCOPA_EINVAL;
    scopa_ctx *ctx = g->ctx;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t Gs = (size_t)g->G;
    if (!g->d_reach) {
        const bool ok = hipMalloc(&g->d_reach, (size_t)g->n * kNodes * 8) == hipSuccess && hipMalloc(&g->d_val, (size_t)g->n * kNodes * 8) == hipSuccess &&
                        hipMalloc(&g->d_pol, Gs * 32) == hipSuccess && hipMalloc(&g->d_pin, Gs * 32) == hipSuccess && hipMalloc(&g->d_choice, Gs * 4) == hipSuccess;
        if (!ok) {
            void **bufs[] = {(void **)&g->d_reach, (void **)&g->d_val, (void **)&g->d_pol, (void **)&g->d_pin, (void **)&g->d_choice};
            for (void **b : bufs) if (*b) { (void)hipFree(*b); *b = nullptr; }
            return fail(ctx, SCOPA_ENOMEM, "scopa_chance_exploitability: device allocation failed");
        }
    }
    if (h_policy) SC_HIP(ctx, hipMemcpyAsync(g->d_pin, h_policy, Gs * 32, hipMemcpyHostToDevice, ctx->stream));
    const unsigned row_blocks = (unsigned)((g->G + 255) / 256);
    hipLaunchKernelGGL(k_chance_policy, dim3(row_blocks), dim3(256), 0, ctx->stream, g->d_gkey, (const double *)g->d_S, h_policy ? (const double *)g->d_pin : nullptr,
                       g->d_pol, g->G);
    chance_br_passes(g, 1, g->d_pol, g->d_reach, g->d_val, g->d_delta, g->d_choice, g->d_out, nullptr);   // the q rows go to the sweep's delta image
    SC_HIP(ctx, hipGetLastError());
    SC_HIP(ctx, hipMemcpyAsync(h_out4, g->d_out, 32, hipMemcpyDeviceToHost, ctx->stream));
    if (h_policy_out) SC_HIP(ctx, hipMemcpyAsync(h_policy_out, g->d_pol, Gs * 32, hipMemcpyDeviceToHost, ctx->stream));
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SCOPA_OK;
}

int32_t scopa_chance_policy_for_deal(scopa_chance *g, const double *d_policy_G, int32_t deal, double *d_policy_local) {
    if (!g || !d_policy_G || !d_policy_local || deal < 0 || deal >= g->n) return SCOPA_EINVAL;
    scopa_ctx *ctx = g->ctx;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    int I = 0;
    while (I < kDecision && g->h_map[(size_t)deal * kDecision + I] >= 0) I++;
    hipLaunchKernelGGL(k_chance_scatter, dim3((I * 4 + 255) / 256), dim3(256), 0, ctx->stream, (const int32_t *)(g->d_map + (size_t)deal * kDecision), d_policy_G,
                       d_policy_local, I);
    SC_HIP(ctx, hipGetLastError());
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SCOPA_OK;
}

// ---- Deep CFR over the set of deals (kernels: scopa_sdcfr.hip, scopa_sdcfr_avg.hip) ----------------------------------------------------------------
int32_t scopa_chance_sdcfr_traverse(scopa_chance *g, int32_t traverser, int32_t batch, int32_t m_deals, const int32_t *h_deals, const float *d_image,
                                    float *d_mem_feat, float *d_mem_regret, float *d_mem_mask, int64_t capacity, int64_t write_base, float *d_root_values,
                                    uint32_t iteration, uint32_t b0) {
    if (!g) return SCOPA_EINVAL;
    scopa_ctx *ctx = g->ctx;
    scopa_multi *mu = g->m;
    const int n = g->n;
    SC_REQUIRE(ctx, traverser == 0 || traverser == 1, SCOPA_EINVAL, "scopa_chance_sdcfr_traverse: traverser must be 0 or 1");
    SC_REQUIRE(ctx, h_deals ? (m_deals >= 1 && m_deals <= n) : (m_deals == 0 || m_deals == n), SCOPA_EINVAL,
               "scopa_chance_sdcfr_traverse: a list holds 1 .. n deals; without a list m is 0 (or n): all deals");
    SC_REQUIRE(ctx, batch >= 0 && !(batch == 0 && h_deals), SCOPA_EINVAL, "scopa_chance_sdcfr_traverse: batch must be positive (0 without a list: no-op)");
    if (!batch) return SCOPA_OK;
    const int m = h_deals ? m_deals : n;
    SC_REQUIRE(ctx, d_image && d_mem_feat && d_mem_regret && d_root_values, SCOPA_EINVAL, "scopa_chance_sdcfr_traverse: NULL device pointer");
    SC_REQUIRE(ctx, !h_deals || chance_lists_ok(n, 1, m, h_deals), SCOPA_EINVAL, "scopa_chance_sdcfr_traverse: a listed deal is outside [0, n) or listed twice");
    SC_REQUIRE(ctx, ((uintptr_t)d_image & 15) == 0, SCOPA_EINVAL, "scopa_chance_sdcfr_traverse: the weight image must be 16-byte aligned");
    SC_REQUIRE(ctx, ((uintptr_t)d_mem_feat & 7) == 0 && ((uintptr_t)d_mem_regret & 15) == 0 && ((uintptr_t)d_mem_mask & 15) == 0, SCOPA_EINVAL,
               "scopa_chance_sdcfr_traverse: memory rows are stored 8 / 16 bytes at a time: d_mem_feat must be 8-byte, d_mem_regret / d_mem_mask 16-byte aligned");
    SC_REQUIRE(ctx, capacity >= 41 && capacity < ((int64_t)1 << 30) && write_base >= 0 && write_base < capacity, SCOPA_EINVAL,
               "scopa_chance_sdcfr_traverse: write_base must lie in [0, capacity) and capacity below 2^30 rows");
    SC_REQUIRE(ctx, (int64_t)41 * m * batch <= capacity, SCOPA_EINVAL, "scopa_chance_sdcfr_traverse: memory ring too small for 41 * m * batch rows");
    SC_REQUIRE(ctx, (uint64_t)b0 + (uint64_t)n * (uint64_t)batch <= ((uint64_t)1 << 32), SCOPA_EINVAL,
               "scopa_chance_sdcfr_traverse: traversal ids b0 + n * batch exceed 2^32");
    SC_REQUIRE(ctx, chance_sdcfr_walk_lds() <= (size_t)ctx->lds_limit, SCOPA_ELIMIT, "scopa_chance_sdcfr_traverse: LDS (walk kernel)");
    SC_HIP(ctx, hipSetDevice(ctx->device));
    if (!g->d_sdninfo && hipMalloc(&g->d_sdninfo, (size_t)n * kDecision * 8) != hipSuccess) {
        g->d_sdninfo = nullptr;
        return fail(ctx, SCOPA_ENOMEM, "scopa_chance_sdcfr_traverse: no device memory for the node-info image");
    }
    if (m > g->sdtab_slots) {
        SC_HIP(ctx, hipStreamSynchronize(ctx->stream));   // an earlier call's launches may still read the old tables
        if (g->d_sdtab) { (void)hipFree(g->d_sdtab); g->d_sdtab = nullptr; g->sdtab_slots = 0; }
        if (hipMalloc(&g->d_sdtab, chance_sdcfr_table_bytes(m)) != hipSuccess) { g->d_sdtab = nullptr; return fail(ctx, SCOPA_ENOMEM, "scopa_chance_sdcfr_traverse: no device memory for the policy tables"); }
        g->sdtab_slots = m;
    }
    if (h_deals) {
        // the list reaches the device without a wait for the stream: it is copied into this turn's row of a pinned ring (free once the copy made from it
        // kSdListRing calls ago is done -- the only thing ever waited for) and from there, in stream order behind the previous call's kernels, into d_sdlist
        if (!g->h_sdlist) {
            if (hipMalloc(&g->d_sdlist, (size_t)n * 4) != hipSuccess) { g->d_sdlist = nullptr; return fail(ctx, SCOPA_ENOMEM, "scopa_chance_sdcfr_traverse: no device memory for the list"); }
            if (hipHostMalloc(&g->h_sdlist, (size_t)kSdListRing * n * 4, hipHostMallocDefault) != hipSuccess) { g->h_sdlist = nullptr; return fail(ctx, SCOPA_ENOMEM, "scopa_chance_sdcfr_traverse: no pinned memory for the list"); }
            for (int i = 0; i < kSdListRing; i++) SC_HIP(ctx, hipEventCreateWithFlags(&g->sd_ev[i], hipEventDisableTiming));
        }
        const unsigned turn = g->sd_turn % kSdListRing;
        if (g->sd_turn >= (unsigned)kSdListRing) SC_HIP(ctx, hipEventSynchronize(g->sd_ev[turn]));
        int32_t *row = g->h_sdlist + (size_t)turn * n;
        std::copy(h_deals, h_deals + m, row);
        SC_HIP(ctx, hipMemcpyAsync(g->d_sdlist, row, (size_t)m * 4, hipMemcpyHostToDevice, ctx->stream));
        SC_HIP(ctx, hipEventRecord(g->sd_ev[turn], ctx->stream));
        g->sd_turn++;
        if (g->sd_turn >= 2u * kSdListRing) g->sd_turn -= kSdListRing;   // (stays >= kSdListRing: every row has been used)
    }
    if (int32_t rc = launch_chance_sdcfr(ctx, n, mu->d_states, mu->d_payoff, g->d_sdninfo, &g->sdninfo_built, m, h_deals ? g->d_sdlist : nullptr, g->d_sdtab,
                                         traverser, batch, d_image, d_mem_feat, d_mem_regret, d_mem_mask, (uint32_t)capacity, (uint32_t)write_base, d_root_values,
                                         iteration, b0))
        return rc;
    g->sdcfr_visits += (uint64_t)m * (uint64_t)batch * (traverser == 0 ? 105 : 82);
    return SCOPA_OK;
}

int32_t scopa_chance_sdcfr_visits(scopa_chance *g, uint64_t *decision_visits) {
    if (!g || !decision_visits) return SCOPA_EINVAL;
    *decision_visits = g->sdcfr_visits;   // counted on the host as the launches are made: no wait for the stream
    return SCOPA_OK;
}

int32_t scopa_chance_sdcfr_average_policy(scopa_chance *g, int32_t player, int32_t n_snap, const float *d_w1, const float *d_b1, const float *d_w2,
                                          const float *d_b2, const float *d_w3, const float *d_b3, int32_t max_size, const int32_t *d_slots,
                                          const float *d_coef, double *d_policy_G) {
    if (!g) return SCOPA_EINVAL;
    scopa_ctx *ctx = g->ctx;
    scopa_multi *mu = g->m;
    SC_REQUIRE(ctx, (player == 0 || player == 1) && n_snap >= 0 && max_size >= 0 && n_snap <= max_size && d_policy_G, SCOPA_EINVAL,
               "scopa_chance_sdcfr_average_policy: player in {0, 1}, 0 <= n_snap <= max_size and a policy table are required");
    if (n_snap > 0) {
        SC_REQUIRE(ctx, d_w1 && d_b1 && d_w2 && d_b2 && d_w3 && d_b3 && d_slots && d_coef, SCOPA_EINVAL, "scopa_chance_sdcfr_average_policy: NULL device pointer");
        const uintptr_t any = (uintptr_t)d_b1 | (uintptr_t)d_w2 | (uintptr_t)d_b2 | (uintptr_t)d_w3 | (uintptr_t)d_b3;
        SC_REQUIRE(ctx, (any & 15) == 0, SCOPA_EINVAL, "scopa_chance_sdcfr_average_policy: b1, w2, b2, w3, b3 are read 16 bytes at a time and must be 16-byte aligned");
    }
    SC_HIP(ctx, hipSetDevice(ctx->device));
    if (!g->sdrep_built) {   // once per handle: the keys' representative nodes, per player in ascending global id
        std::vector<int32_t> rank((size_t)g->G);
        int cnt[2] = {0, 0};
        for (long long i = 0; i < g->G; i++) rank[(size_t)i] = cnt[g->h_gkey[(size_t)i] & 1]++;
        int32_t *d_rank = nullptr;
        bool ok = hipMalloc(&d_rank, (size_t)g->G * 4) == hipSuccess;
        for (int p = 0; p < 2 && ok; p++) ok = hipMalloc(&g->d_sdrep[p], (size_t)(cnt[p] ? cnt[p] : 1) * 16) == hipSuccess;
        if (!ok) {
            if (d_rank) (void)hipFree(d_rank);
            for (int p = 0; p < 2; p++) if (g->d_sdrep[p]) { (void)hipFree(g->d_sdrep[p]); g->d_sdrep[p] = nullptr; }
            return fail(ctx, SCOPA_ENOMEM, "scopa_chance_sdcfr_average_policy: no device memory for the key list");
        }
        int32_t rc = SCOPA_OK;
        if (hipMemcpyAsync(d_rank, rank.data(), (size_t)g->G * 4, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) rc = fail(ctx, SCOPA_EHIP, "scopa_chance_sdcfr_average_policy: upload of the key ranks failed");
        if (!rc) rc = launch_chance_sdcfr_reps(ctx, g->G, g->d_gkey, g->d_occ_off, g->d_occ, mu->d_infoset, mu->d_states, d_rank, g->d_sdrep[0], g->d_sdrep[1]);
        const hipError_t e = hipStreamSynchronize(ctx->stream);   // `rank` and d_rank go away below
        (void)hipFree(d_rank);
        if (rc) return rc;
        SC_HIP(ctx, e);
        g->sd_keys[0] = cnt[0]; g->sd_keys[1] = cnt[1];
        g->sdrep_built = true;
    }
    const int n_keys = g->sd_keys[player];
    const size_t bytes = (size_t)n_snap * (size_t)n_keys * 16;
    if (bytes > g->sdterms_bytes) {
        SC_HIP(ctx, hipStreamSynchronize(ctx->stream));   // an earlier call's launches may still read the old buffer
        if (g->d_sdterms) { (void)hipFree(g->d_sdterms); g->d_sdterms = nullptr; g->sdterms_bytes = 0; }
        if (hipMalloc(&g->d_sdterms, bytes) != hipSuccess) { g->d_sdterms = nullptr; return fail(ctx, SCOPA_ENOMEM, "scopa_chance_sdcfr_average_policy: no device memory for the terms"); }
        g->sdterms_bytes = bytes;
    }
    return launch_chance_sdcfr_avg(ctx, n_keys, g->d_sdrep[player], n_snap, d_w1, d_b1, d_w2, d_b2, d_w3, d_b3, max_size, d_slots, d_coef, g->d_sdterms, d_policy_G);
}

}  // extern "C"
