// scopa_full_store_host.h -- THE kernels and host plumbing of a FullScopa infoset store, one definition for its two slot types: FmSlot (one-word keys,
// scopa_full_store.h, behind scopa_full_mccfr_*) and FwSlot (two-word keys, scopa_full_wide.h, behind scopa_full_chance_*).  The slots have one layout,
// so everything here is written once over the handle's common part StoreHandle<Slot>; what differs between the stores is SlotKey<Slot> and nothing else.
// Included by the translation units that launch these kernels or end a call on the counters: scopa_full_mccfr.hip, scopa_full_chance.hip,
// scopa_full_chance_cfr.hip (check_dropped) and scopa_full_chance_xplay.hip (run_match).
//
//   who       the helpers' messages keep the caller's name in front: an entry point's ("scopa_full_chance_tables_set") or, where several entry points
//             share a helper, the solver's (SlotKey<Slot>::kWho).  Argument checks whose limits differ between the entry points stay with them.
#pragma once
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <new>
#include <vector>

#include "scopa_full_store.h"

namespace scopa_full {

template <class Slot>
__global__ void __launch_bounds__(256)
k_full_store_apply(Slot *__restrict__ tab, uint32_t n_slots) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_slots || tab[i].key == 0ull) return;
    Slot &t = tab[i];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        t.regret[a] += t.d_regret[a];
        t.strategy[a] += t.d_strategy[a];
        t.d_regret[a] = 0.0;
        t.d_strategy[a] = 0.0;
    }
    t.count = 0u;
}

// occupied slots, whole lines, to a dense image in arrival order
template <class Slot>
__global__ void __launch_bounds__(256)
k_full_store_export(const Slot *__restrict__ tab, uint32_t n_slots, Slot *__restrict__ out, unsigned long long max_rows, unsigned long long *cnt) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_slots || tab[i].key == 0ull) return;
    const unsigned long long at = atomicAdd(cnt + kCntCursor, 1ull);
    if (at >= max_rows) return;
    const uint4 *src = reinterpret_cast<const uint4 *>(tab + i);
    uint4 *dst = reinterpret_cast<uint4 *>(out + at);
#pragma unroll
    for (int k = 0; k < 8; k++) dst[k] = src[k];
}

template <class Slot>
__global__ void __launch_bounds__(256)
k_full_store_import(Slot *__restrict__ tab, uint32_t mask, const Slot *__restrict__ rows, uint32_t n_rows, unsigned long long *cnt) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows) return;
    const int slot = SlotKey<Slot>::claim(tab, mask, rows[i], cnt);
    if (slot < 0) return;
#pragma unroll
    for (int a = 0; a < 3; a++) { tab[slot].regret[a] = rows[i].regret[a]; tab[slot].strategy[a] = rows[i].strategy[a]; }
}

// fail() with the caller's name in front of the message
template <class H>
int32_t refuse(H *h, const char *who, const char *what, int32_t code = SCOPA_EINVAL, hipError_t e = hipSuccess) {
    char msg[256];
    snprintf(msg, sizeof msg, "%s: %s", who, what);
    return scopa::fail(h->ctx, code, msg, e);
}

template <class H> int rounds_left(const H *h) { return 6 - (int)h->root.round; }
template <class H> int default_cut(const H *h) { return std::min(kMaxCut, rounds_left(h) / 2); }

template <class H>
int32_t set_cut(H *h, const char *who, int32_t cut) {
    if (!h) return SCOPA_EINVAL;
    if (!(cut >= -1 && cut <= std::min(kMaxCut, rounds_left(h)))) return refuse(h, who, "cut outside [-1, min(3, rounds from the root)]");
    h->cut = cut;
    return SCOPA_OK;
}

template <class H>
int32_t read_counters(H *h, unsigned long long c[kCntWords]) {
    SC_HIP(h->ctx, hipMemcpyAsync(c, h->d_cnt, kCntWords * 8, hipMemcpyDeviceToHost, h->ctx->stream));
    SC_HIP(h->ctx, hipStreamSynchronize(h->ctx->stream));
    return SCOPA_OK;
}

// after a call that may have claimed slots: SCOPA_ENOMEM where inserts were dropped during it
template <class H>
int32_t check_dropped(H *h, const char *what) {
    unsigned long long c[kCntWords];
    const int32_t rc = read_counters(h, c);
    if (rc != SCOPA_OK) return rc;
    const bool more = c[kCntDropped] != h->dropped_seen;
    h->dropped_seen = c[kCntDropped];
    return more ? scopa::fail(h->ctx, SCOPA_ENOMEM, what) : SCOPA_OK;
}

template <class H>
int32_t counters_out(H *h, uint64_t *choice_visits, uint64_t *terminal_visits, uint64_t *rows, uint64_t *dropped, uint32_t *iterations) {
    if (!h) return SCOPA_EINVAL;
    SC_HIP(h->ctx, hipSetDevice(h->ctx->device));
    unsigned long long c[kCntWords];
    const int32_t rc = read_counters(h, c);
    if (rc != SCOPA_OK) return rc;
    if (choice_visits) *choice_visits = c[kCntChoice];
    if (terminal_visits) *terminal_visits = c[kCntTerminal];
    if (rows) *rows = c[kCntRows];
    if (dropped) *dropped = c[kCntDropped];
    if (iterations) *iterations = h->iteration;
    return SCOPA_OK;
}

template <class H>
int32_t launch_apply(H *h) {
    const uint32_t n = 1u << h->capacity_log2;
    hipLaunchKernelGGL(k_full_store_apply<typename H::Slot>, dim3((n + 255u) / 256u), dim3(256), 0, h->ctx->stream, h->d_tab, n);
    SC_HIP(h->ctx, hipGetLastError());
    h->iteration++;
    return SCOPA_OK;
}

template <class H>
int32_t clear_store(H *h) {
    SC_HIP(h->ctx, hipMemsetAsync(h->d_tab, 0, sizeof(typename H::Slot) << h->capacity_log2, h->ctx->stream));
    SC_HIP(h->ctx, hipMemsetAsync(h->d_cnt + kCntRows, 0, 8, h->ctx->stream));
    return SCOPA_OK;
}

// the occupied slots as whole lines, in any order
template <class H>
int32_t export_rows(H *h, std::vector<typename H::Slot> &rows) {
    using Slot = typename H::Slot;
    const char *who = SlotKey<Slot>::kWho;
    unsigned long long c[kCntWords];
    int32_t rc = read_counters(h, c);
    if (rc != SCOPA_OK) return rc;
    const unsigned long long n_rows = c[kCntRows];
    rows.clear();
    if (!n_rows) return SCOPA_OK;
    try { rows.resize((size_t)n_rows); } catch (const std::bad_alloc &) { return refuse(h, who, "host image of the rows", SCOPA_ENOMEM); }
    Slot *d_out = nullptr;
    hipError_t e = hipMalloc((void **)&d_out, (size_t)n_rows * sizeof(Slot));
    if (e != hipSuccess) return refuse(h, who, "device image of the rows", SCOPA_ENOMEM, e);
    const uint32_t n = 1u << h->capacity_log2;
    rc = SCOPA_OK;
    if ((e = hipMemsetAsync(h->d_cnt + kCntCursor, 0, 8, h->ctx->stream)) != hipSuccess) rc = scopa::fail(h->ctx, SCOPA_EHIP, "hipMemsetAsync", e);
    if (rc == SCOPA_OK) {
        hipLaunchKernelGGL(k_full_store_export<Slot>, dim3((n + 255u) / 256u), dim3(256), 0, h->ctx->stream, (const Slot *)h->d_tab, n, d_out, n_rows, h->d_cnt);
        if ((e = hipGetLastError()) != hipSuccess) rc = scopa::fail(h->ctx, SCOPA_EHIP, SlotKey<Slot>::kExport, e);
    }
    if (rc == SCOPA_OK && (e = hipMemcpyAsync(rows.data(), d_out, (size_t)n_rows * sizeof(Slot), hipMemcpyDeviceToHost, h->ctx->stream)) != hipSuccess)
        rc = scopa::fail(h->ctx, SCOPA_EHIP, "hipMemcpyAsync(D2H)", e);
    e = hipStreamSynchronize(h->ctx->stream);
    if (rc == SCOPA_OK && e != hipSuccess) rc = scopa::fail(h->ctx, SCOPA_EHIP, "hipStreamSynchronize", e);
    (void)hipFree(d_out);
    return rc;
}

// the body of tables_get (delta = false) and delta_get (delta = true); keys: SlotKey::kWords words a row
template <class H>
int32_t rows_out(H *h, const char *who, int64_t *n_rows, uint64_t *keys, int32_t *n_act, double *a, double *b, uint32_t *counts, bool delta) {
    using K = SlotKey<typename H::Slot>;
    if (!h || !n_rows) return SCOPA_EINVAL;
    SC_HIP(h->ctx, hipSetDevice(h->ctx->device));
    std::vector<typename H::Slot> rows;
    const int32_t rc = export_rows(h, rows);
    if (rc != SCOPA_OK) return rc;
    const int64_t room = *n_rows;
    *n_rows = (int64_t)rows.size();
    if (!keys && !n_act && !a && !b && !counts) return SCOPA_OK;          // the count alone
    if (room < (int64_t)rows.size()) return refuse(h, who, "*n_rows is below the rows occupied (now in *n_rows)");
    for (size_t i = 0; i < rows.size(); i++) {
        if (keys) K::get(rows[i], keys + K::kWords * i);
        if (n_act) n_act[i] = K::actions(rows[i]);
        if (counts) counts[i] = rows[i].count;
        for (int c = 0; c < 3; c++) {
            if (a) a[3 * i + c] = delta ? rows[i].d_regret[c] : rows[i].regret[c];
            if (b) b[3 * i + c] = delta ? rows[i].d_strategy[c] : rows[i].strategy[c];
        }
    }
    return SCOPA_OK;
}

// the device half of tables_set: the store cleared, then the rows claimed and written by one launch
template <class H>
int32_t import_rows(H *h, const char *who, const std::vector<typename H::Slot> &rows) {
    using Slot = typename H::Slot;
    SC_HIP(h->ctx, hipSetDevice(h->ctx->device));
    int32_t rc = clear_store(h);
    const size_t n_rows = rows.size();
    if (rc != SCOPA_OK || !n_rows) return rc;
    Slot *d_rows = nullptr;
    hipError_t e = hipMalloc((void **)&d_rows, n_rows * sizeof(Slot));
    if (e != hipSuccess) return refuse(h, who, "device image of the rows", SCOPA_ENOMEM, e);
    if ((e = hipMemcpyAsync(d_rows, rows.data(), n_rows * sizeof(Slot), hipMemcpyHostToDevice, h->ctx->stream)) != hipSuccess)
        rc = scopa::fail(h->ctx, SCOPA_EHIP, "hipMemcpyAsync(H2D)", e);
    if (rc == SCOPA_OK) {
        hipLaunchKernelGGL(k_full_store_import<Slot>, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, h->ctx->stream, h->d_tab, (1u << h->capacity_log2) - 1u,
                           (const Slot *)d_rows, (uint32_t)n_rows, h->d_cnt);
        if ((e = hipGetLastError()) != hipSuccess) rc = scopa::fail(h->ctx, SCOPA_EHIP, SlotKey<Slot>::kImport, e);
    }
    char full[128];
    snprintf(full, sizeof full, "%s: the store is full along a probe (rows dropped)", who);
    const int32_t rc2 = check_dropped(h, full);                           // synchronises: the image may go
    (void)hipFree(d_rows);
    return rc != SCOPA_OK ? rc : rc2;
}

// the body of tables_set: every row checked on the host before any device work, so a refused call leaves the store as it was
template <class H>
int32_t tables_in(H *h, const char *who, int64_t n_rows, const uint64_t *keys, const int32_t *n_act, const double *regret, const double *strategy) {
    using Slot = typename H::Slot;
    using K = SlotKey<Slot>;
    if (!h) return SCOPA_EINVAL;
    if (!(n_rows >= 0 && n_rows <= (1ll << h->capacity_log2) && (!n_rows || (keys && n_act && regret && strategy))))
        return refuse(h, who, "n_rows outside [0, capacity] or a NULL array");
    std::vector<Slot> rows;
    std::vector<std::array<uint64_t, K::kWords>> sorted;                  // duplicates: equal neighbours of the sorted keys
    try {
        rows.resize((size_t)n_rows);
        sorted.resize((size_t)n_rows);
    } catch (const std::bad_alloc &) { return refuse(h, who, "host image", SCOPA_ENOMEM); }
    for (int64_t i = 0; i < n_rows; i++) memcpy(sorted[(size_t)i].data(), keys + K::kWords * i, 8 * K::kWords);
    std::sort(sorted.begin(), sorted.end());
    for (int64_t i = 0; i < n_rows; i++) {
        Slot &row = rows[(size_t)i];
        memset(&row, 0, sizeof(Slot));
        K::set(row, keys + K::kWords * i);
        const int n = K::actions(row);
        if (!(K::key_ok(row) && (n == 2 || n == 3) && n == n_act[i])) return refuse(h, who, K::kBadKey);
        if (i > 0 && sorted[(size_t)i] == sorted[(size_t)i - 1]) return refuse(h, who, K::kTwice);
        for (int c = 0; c < n; c++) { row.regret[c] = regret[3 * i + c]; row.strategy[c] = strategy[3 * i + c]; }
    }
    return import_rows(h, who, rows);
}

// the tail of a match call, after the entry point's own checks: the optional per-episode buffer, the optional held-out decks (k of them), the sums
// zeroed, launch(d_held or NULL, d_sums, d_r2 or NULL) -- the ONE launch of `kernel` --, the two downloads, one synchronisation
template <class H, class Launch>
int32_t run_match(H *h, const char *who, const char *kernel, int64_t n_episodes, const uint8_t *h_decks, int32_t k, int64_t h_sums[6], int8_t *h_r2, Launch launch) {
    long long *d_sums = match_sums(h->d_cnt);
    int8_t *d_r2 = nullptr;
    uint8_t *d_held = nullptr;
    hipError_t e;
    if (h_r2 && (e = hipMalloc((void **)&d_r2, (size_t)n_episodes)) != hipSuccess) return refuse(h, who, "per-episode output", SCOPA_ENOMEM, e);
    int32_t rc = SCOPA_OK;
    if (h_decks) {
        if ((e = hipMalloc((void **)&d_held, 40 * (size_t)k + 24)) != hipSuccess) rc = refuse(h, who, "the decks", SCOPA_ENOMEM, e);
        else if ((e = hipMemcpyAsync(d_held, h_decks, 40 * (size_t)k, hipMemcpyHostToDevice, h->ctx->stream)) != hipSuccess) rc = scopa::fail(h->ctx, SCOPA_EHIP, "hipMemcpyAsync(H2D)", e);
    }
    if (rc == SCOPA_OK && (e = hipMemsetAsync(d_sums, 0, 8 * 8, h->ctx->stream)) != hipSuccess) rc = scopa::fail(h->ctx, SCOPA_EHIP, "hipMemsetAsync", e);
    if (rc == SCOPA_OK) {
        launch((const uint8_t *)d_held, d_sums, d_r2);
        if ((e = hipGetLastError()) != hipSuccess) rc = scopa::fail(h->ctx, SCOPA_EHIP, kernel, e);
    }
    if (rc == SCOPA_OK && (e = hipMemcpyAsync(h_sums, d_sums, 6 * 8, hipMemcpyDeviceToHost, h->ctx->stream)) != hipSuccess) rc = scopa::fail(h->ctx, SCOPA_EHIP, "hipMemcpyAsync(D2H)", e);
    if (rc == SCOPA_OK && d_r2 && (e = hipMemcpyAsync(h_r2, d_r2, (size_t)n_episodes, hipMemcpyDeviceToHost, h->ctx->stream)) != hipSuccess)
        rc = scopa::fail(h->ctx, SCOPA_EHIP, "hipMemcpyAsync(D2H)", e);
    e = hipStreamSynchronize(h->ctx->stream);
    if (rc == SCOPA_OK && e != hipSuccess) rc = scopa::fail(h->ctx, SCOPA_EHIP, "hipStreamSynchronize", e);
    if (d_r2) (void)hipFree(d_r2);
    if (d_held) (void)hipFree(d_held);
    return rc;
}

}  // namespace scopa_full
