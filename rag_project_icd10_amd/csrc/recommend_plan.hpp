// recommend_plan.hpp - the host-visible part of the recommend search: the limits, the strategies, the byte
// budget of one block and the requests and example vectors it holds, the cut of a batch into blocks of WHOLE requests, the
// geometry of the combine kernel, the request table and the workspace layout. No HIP header and no handle: included by
// recommend_kernel.hpp (the kernels call these very functions) and by tests/recommend_plan_check.cpp, which runs them under the
// host sanitizers.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "wide_select_plan.hpp"   // the select over one ordered score per (request, row) is the wide search's: budget, padding, offsets, tiers

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RC_HD __host__ __device__
#else
#define RC_HD
#endif

namespace icd {

constexpr int RC_MAX_EXAMPLES = 16;                 // P + N of one request (ICD_RECOMMEND_MAX_EXAMPLES)
constexpr int RC_AVERAGE_VECTOR = 0;                // ICD_RECOMMEND_*
constexpr int RC_BEST_SCORE = 1;
constexpr int RC_SUM_SCORES = 2;
constexpr long long RC_MAX_REQUESTS = WS_MAX_NQ;    // requests of one workspace
constexpr int RC_COMBINE_THREADS = 256;             // the combine: four waves, every lane four consecutive rows
constexpr int RC_LANE_ROWS = 4;                     // one 16-byte load per example, one 16-byte store
constexpr int RC_SEG_ROWS = RC_COMBINE_THREADS * RC_LANE_ROWS;   // rows of one work-group of the combine
constexpr int RC_EXAMPLE_THREADS = 256;             // the examples kernel: one work-group per written vector

// work-groups of the combine along the rows (n_pad is a multiple of RK_TILE = 128, so a lane's four rows are inside it or past it)
RC_HD inline long long rc_segments(long long n_pad) { return (n_pad + RC_SEG_ROWS - 1) / RC_SEG_ROWS; }

// Bytes of a block per example vector (its row of E, its run of SE) and per request (its run of S, its row of C, a host caller's
// output staging adj f64 + raw f32 + id i64 + level i32).
RC_HD inline size_t rc_example_bytes(long long n, int dim) { return (size_t)dim * 4 + (size_t)ws_padded_rows(n) * 4; }
RC_HD inline size_t rc_request_bytes(long long n, int max_k) { return ws_query_bytes(n, max_k); }
// Example vectors of a block of b requests: the workspace's own examples per request (max_examples / max_requests, rounded up:
// 16 by default, fewer where the caller knows its requests are short), at least one full request's 16, never more than the
// workspace takes per call. The cut (rc_cut) honours both limits, so a block of long requests simply holds fewer of them.
RC_HD inline long long rc_examples_of(long long b, long long max_requests, long long max_examples) {
    long long e = (b * max_examples + max_requests - 1) / max_requests;   // (b <= max_requests <= 2^20, max_examples <= 2^24)
    if (e < RC_MAX_EXAMPLES) e = RC_MAX_EXAMPLES;
    return e < max_examples ? e : max_examples;
}
RC_HD inline size_t rc_block_bytes(long long b, long long max_requests, long long max_examples, long long n, int dim, int max_k) {
    return (size_t)b * rc_request_bytes(n, max_k) + (size_t)rc_examples_of(b, max_requests, max_examples) * rc_example_bytes(n, dim);
}
// Requests of one block: the most whose runs, rows and worst-case example vectors stay inside the wide search's budget, at most
// max_requests. 0: not even one request with its examples fits. (rc_block_bytes grows with b: a bisection.)
RC_HD inline long long rc_block_requests(long long max_requests, long long max_examples, long long n, int dim, int max_k) {
    if (rc_block_bytes(1, max_requests, max_examples, n, dim, max_k) > WS_BLOCK_BUDGET) return 0;
    long long lo = 1, hi = max_requests;   // lo fits
    while (lo < hi) {
        const long long mid = lo + (hi - lo + 1) / 2;
        if (rc_block_bytes(mid, max_requests, max_examples, n, dim, max_k) <= WS_BLOCK_BUDGET) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// The cut: how many requests from r0 on form the next block - whole requests only, at most block_requests of them and at most
// block_examples example vectors. example_off: [nr + 1] from 0, every request of 1 .. 16 examples (checked by the caller), so
// with block_examples >= 16 (or >= every request of the call) the cut is never 0.
inline long long rc_cut(const int64_t *example_off, long long r0, long long nr, long long block_requests, long long block_examples) {
    long long r = r0;
    while (r < nr && r - r0 < block_requests && example_off[r + 1] - example_off[r0] <= block_examples) ++r;
    return r - r0;
}

// The request table of a call as the device reads it, int32 each: off [nr + 1] (first example of a request, in the call's example
// order), npos [nr] (the positives at the head), rows [ne] (a stored example's row, -1 for a caller's vector). One host block, one copy.
RC_HD inline size_t rc_table_npos(long long nr) { return (size_t)nr + 1; }
RC_HD inline size_t rc_table_rows(long long nr) { return (size_t)2 * (size_t)nr + 1; }
RC_HD inline size_t rc_table_words(long long nr, long long ne) { return (size_t)2 * (size_t)nr + 1 + (size_t)ne; }

// Elements of the workspace's arrays for calls of up to max_requests requests with up to max_examples examples in all and
// first + k up to max_k, on an index of n rows and `dim` columns. Everything is allocated at create; a call allocates nothing.
struct RecommendLayout {
    long long block;          // requests of one block (rc_block_requests)
    long long block_examples; // example vectors of one block (rc_examples_of)
    long long n_pad;
    size_t v_floats;     // [max_examples][dim]      a host caller's example vectors
    size_t bounds;       // [max_requests]           a host caller's radius / range_filter, each
    size_t table;        // rc_table_words           the request table (device; the same again in pinned host memory)
    size_t e_floats;     // [block_examples][dim]    E
    size_t se_words;     // [block_examples][n_pad]  SE
    size_t s_words;      // [block][n_pad]           S
    size_t c_keys;       // [block][max_k]           C
    size_t recs;         // [block]                  WideRec
    size_t out_slots;    // [block][max_k]           a host caller's adj, raw, ids, levels, each
    size_t per_request;  // [max_requests]           a host caller's count and selected, each
    size_t bytes;        // all of it (device)
};
RC_HD inline RecommendLayout rc_layout(long long max_requests, long long max_examples, int max_k, long long n, int dim) {
    RecommendLayout l;
    l.block = rc_block_requests(max_requests, max_examples, n, dim, max_k);
    l.block_examples = rc_examples_of(l.block, max_requests, max_examples);
    l.n_pad = ws_padded_rows(n);
    l.v_floats = (size_t)max_examples * (size_t)dim;
    l.bounds = (size_t)max_requests;
    l.table = rc_table_words(max_requests, max_examples);
    l.e_floats = (size_t)l.block_examples * (size_t)dim;
    l.se_words = (size_t)l.block_examples * (size_t)l.n_pad;
    l.s_words = (size_t)l.block * (size_t)l.n_pad;
    l.c_keys = (size_t)l.block * (size_t)max_k;
    l.recs = (size_t)l.block;
    l.out_slots = (size_t)l.block * (size_t)max_k;
    l.per_request = (size_t)max_requests;
    l.bytes = l.v_floats * 4 + l.bounds * 8 + l.table * 4 + l.e_floats * 4 + l.se_words * 4 + l.s_words * 4 + l.c_keys * 8 +
              l.recs * sizeof(WideRec) + l.out_slots * (8 + 4 + 8 + 4) + l.per_request * (4 + 8);
    return l;
}

}  // namespace icd
