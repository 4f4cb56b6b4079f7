// byrows_kernel.hpp - search by stored rows: the device-side front and back end around the exact search.
// Replaces what a caller of Milvus's search by primary key does here by hand: fetch the row's 3 KB to the host, send it back as a
// query, find and cut its own hit out of the list.
//
// byrows_gather_kernel   one wave per query: the canonical fp32 row of ids[q] -> row q of the query block the exact kernels read,
//                        16-byte loads and stores (dim is a multiple of 32 and both blocks come from hipMalloc: every row is
//                        128-byte aligned, so 16 bytes is the widest vector load there is and it always applies). An id outside
//                        the index writes a ZERO query and flags the query; the row address is formed only behind that test.
// byrows_drop_self_kernel one wave per query over its staged list of len = keep + 1 slots (raw order, padding behind the hits):
//                        the position of the row's own id by ballot (absent: the last slot), the keep-wide outputs with
//                        everything behind the gap moved up by one, then - reweighted - the level weight in double and ONE
//                        stable descending re-sort (emit_outputs' step, finalize.hpp). len = keep skips the removal. A flagged
//                        query is all padding.
// Plain vector loads and stores; nothing data-dependent decides WHETHER a slot is written: the same call twice gives the same
// bytes. No atomics, no scratch. LDS: the drop's adjusted scores, BR_WAVES x 128 doubles = 4 KB static.
#pragma once
#include "byrows_plan.hpp"
#include "finalize.hpp"

namespace icd {

struct ByRowsGatherArgs {
    const float *corpus;      // [n][dim] the canonical fp32 rows
    const long long *ids;     // [nq] global ids
    float *q;                 // [nq][dim] the query block
    int *flag;                // [nq] 1: ids[q] is no row of the index
    long long n, id_base;
    int dim, nq;
};

__global__ __launch_bounds__(BR_THREADS) void byrows_gather_kernel(const ByRowsGatherArgs a) {
    const int lane = threadIdx.x & (BR_WAVE - 1);
    const long long q = (long long)blockIdx.x * BR_WAVES + (threadIdx.x >> 6);
    if (q >= a.nq) return;
    const long long row = br_row_of(a.ids[q], a.id_base, a.n);
    const int quads = a.dim >> 2;
    f32x4 *dst = reinterpret_cast<f32x4 *>(a.q + (size_t)q * a.dim);
    if (row < 0) {
        const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int i = lane; i < quads; i += BR_WAVE) dst[i] = zero;
    } else {
        const f32x4 *src = reinterpret_cast<const f32x4 *>(a.corpus + (size_t)row * a.dim);
        for (int i = lane; i < quads; i += BR_WAVE) dst[i] = src[i];
    }
    if (lane == 0) a.flag[q] = row < 0 ? 1 : 0;
}

struct ByRowsDropArgs {
    const float *st_raw;        // [nq][len] the staged lists, raw order, padding (id -1) behind the hits
    const long long *st_ids;
    const int *st_levels;
    const long long *ids;       // [nq] the rows' own global ids
    const int *flag;            // [nq] the gather's flags
    double *out_adj;            // [nq][keep], reweighted only
    float *out_raw;
    long long *out_ids;
    int *out_levels;            // nullable
    int nq, len, keep, reweighted;
};

#pragma clang fp contract(off)
__global__ __launch_bounds__(BR_THREADS) void byrows_drop_self_kernel(const ByRowsDropArgs a) {
    __shared__ double adjbuf[BR_WAVES][BR_MAX_LIST];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & (BR_WAVE - 1);
    const long long q = (long long)blockIdx.x * BR_WAVES + wave;
    const bool live = q < a.nq;   // (a wave past the batch still meets the barrier)
    const int len = a.len, keep = a.keep;
    const size_t sbase = (size_t)(live ? q : 0) * len;
    const bool flagged = live && a.flag[q] != 0;
    const long long self = live ? a.ids[q] : -1ll;

    // the gap: the lowest slot that holds the row's own id
    int first = BR_MAX_LIST;
#pragma unroll
    for (int e = BR_PER_LANE - 1; e >= 0; --e) {
        const int j = lane + BR_WAVE * e;
        const bool hit = live && len > keep && j < len && a.st_ids[sbase + j] == self;
        const unsigned long long b = __ballot(hit);
        if (b) first = BR_WAVE * e + __builtin_ctzll(b);
    }
    const int gap = br_gap(first, len, keep);

    float raw[BR_PER_LANE];
    long long id[BR_PER_LANE];
    int lv[BR_PER_LANE];
    double adj[BR_PER_LANE];
#pragma unroll
    for (int e = 0; e < BR_PER_LANE; ++e) {
        const int j = lane + BR_WAVE * e;
        raw[e] = -INFINITY; id[e] = -1; lv[e] = 0; adj[e] = -INFINITY;
        if (live && !flagged && j < keep) {
            const size_t s = sbase + br_source(j, gap);   // (< len: plan check)
            const long long sid = a.st_ids[s];
            if (sid >= 0) {
                id[e] = sid; raw[e] = a.st_raw[s]; lv[e] = a.st_levels[s];
                adj[e] = (double)raw[e] * level_weight(lv[e]);
            }
        }
        adjbuf[wave][j] = adj[e];
    }
    __syncthreads();
    if (!live) return;
    const size_t o = (size_t)q * keep;
#pragma unroll
    for (int e = 0; e < BR_PER_LANE; ++e) {
        const int j = lane + BR_WAVE * e;
        if (j >= keep) continue;
        const size_t w = o + (a.reweighted ? br_stable_rank(adjbuf[wave], keep, j) : j);
        if (a.reweighted) a.out_adj[w] = adj[e];
        a.out_raw[w] = raw[e];
        a.out_ids[w] = id[e];
        if (a.out_levels) a.out_levels[w] = lv[e];
    }
}
#pragma clang fp contract(fast)

}  // namespace icd
