// wide_select_plan.hpp - the host-visible part of the wide search: the limits, the byte budget of one score
// block and the queries it holds, the offsets into the score block and the candidate block, the digit split of the radix select,
// the tiers of the sort and the workspace layout. No HIP header and no handle: included by wide_select_kernel.hpp (the kernels
// call these very functions) and by tests/wide_select_plan_check.cpp, which runs them under the host sanitizers.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "rankof_plan.hpp"   // the sweep's geometry (RK_TILE, RK_QUERIES, rk_plan, rk_valid_bits, rk_sweep_lds_bytes) is shared

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WS_HD __host__ __device__
#else
#define WS_HD
#endif

namespace icd {

constexpr int WS_MAX_K = 16384;                     // first + k of one call (ICD_WIDE_MAX_K)
constexpr long long WS_MAX_NQ = 1ll << 20;          // queries of one workspace
constexpr int WS_SELECT_THREADS = 1024;             // threshold, collect: one work-group per query

// The byte budget of ONE score block: everything the workspace holds per query of a block - the query's run of S, its row of C
// and a host caller's output staging - times the block's queries stays under it. A batch longer than a block runs block by block.
constexpr size_t WS_BLOCK_BUDGET = (size_t)256 << 20;
WS_HD inline long long ws_padded_rows(long long n) { return (n + RK_TILE - 1) / RK_TILE * RK_TILE; }
// bytes per query of a block: S u32 [n padded], C u64 [max_k], staging adj f64 + raw f32 + id i64 + level i32 [max_k]
WS_HD inline size_t ws_query_bytes(long long n, int max_k) { return (size_t)ws_padded_rows(n) * 4 + (size_t)max_k * (8 + 8 + 4 + 8 + 4); }
// Queries of one score block: as many as the budget holds, at most max_nq; where that cuts a batch, whole sweep work-groups
// (RK_QUERIES) if it can. 0: not even one query fits (the index is too large for a one-work-group select).
WS_HD inline long long ws_block_queries(long long max_nq, long long n, int max_k) {
    long long b = (long long)(WS_BLOCK_BUDGET / ws_query_bytes(n, max_k));
    if (b >= max_nq) return max_nq;
    if (b >= RK_QUERIES) b = b / RK_QUERIES * RK_QUERIES;
    return b;
}

// element offsets of query `qb` of a block: into S (runs of n padded u32) and into C (rows of `width` = first + k u64)
WS_HD inline size_t ws_s_offset(long long qb, long long n_pad) { return (size_t)qb * (size_t)n_pad; }
WS_HD inline size_t ws_c_offset(long long qb, int width) { return (size_t)qb * (size_t)width; }
// element offset of slot j of query q in an output [nq][k]
WS_HD inline size_t ws_out_offset(long long q, int k, int j) { return (size_t)q * (size_t)k + (size_t)j; }

// The radix select's digits, most significant first: 11 + 11 + 10 bits of the ordered score.
constexpr int WS_PASSES = 3;
constexpr int WS_BINS = 2048;   // bins of the widest digit: the LDS histogram
WS_HD inline int ws_digit_bits(int pass) { return pass < 2 ? 11 : 10; }
WS_HD inline int ws_digit_shift(int pass) { return pass == 0 ? 21 : (pass == 1 ? 10 : 0); }
WS_HD inline uint32_t ws_digit_mask(int pass) { return ((1u << ws_digit_bits(pass)) - 1u) << ws_digit_shift(pass); }

// The sort's tiers by first + k: keys in LDS (8 bytes each), threads of the work-group.
constexpr int WS_TIERS = 3;
WS_HD inline int ws_tier(int width) { return width <= 1024 ? 0 : (width <= 4096 ? 1 : 2); }
WS_HD inline int ws_tier_keys(int tier) { return tier == 0 ? 1024 : (tier == 1 ? 4096 : 16384); }
WS_HD inline int ws_tier_threads(int tier) { return tier == 0 ? 256 : 1024; }
WS_HD inline size_t ws_tier_lds_bytes(int tier) { return (size_t)ws_tier_keys(tier) * 8; }

// What the threshold kernel leaves per query of a block.
struct WideRec {
    uint32_t T;          // the ordered score of the last rank of the answer (no rows rank, or none asked for: 0xFFFFFFFF)
    uint32_t above;      // rows strictly above T
    uint32_t need;       // rows equal to T that belong to the answer: the `need` smallest row ids
    uint32_t selected;   // rows that rank
};

// Elements of the workspace's arrays for calls of up to max_nq queries and first + k up to max_k on an index of n rows and `dim`
// columns. Everything is allocated at create; a call allocates nothing.
struct WideLayout {
    long long block;     // queries of one score block (ws_block_queries)
    long long n_pad;
    size_t q_floats;     // [max_nq][dim]   a host caller's queries
    size_t bounds;       // [max_nq]        a host caller's radius / range_filter, each
    size_t s_words;      // [block][n_pad]  S
    size_t c_keys;       // [block][max_k]  C
    size_t recs;         // [block]         WideRec
    size_t out_slots;    // [block][max_k]  a host caller's adj, raw, ids, levels, each
    size_t per_query;    // [max_nq]        a host caller's count and selected, each
    size_t bytes;        // all of it
};
WS_HD inline WideLayout ws_layout(long long max_nq, int max_k, long long n, int dim) {
    WideLayout l;
    l.block = ws_block_queries(max_nq, n, max_k);
    l.n_pad = ws_padded_rows(n);
    l.q_floats = (size_t)max_nq * (size_t)dim;
    l.bounds = (size_t)max_nq;
    l.s_words = (size_t)l.block * (size_t)l.n_pad;
    l.c_keys = (size_t)l.block * (size_t)max_k;
    l.recs = (size_t)l.block;
    l.out_slots = (size_t)l.block * (size_t)max_k;
    l.per_query = (size_t)max_nq;
    l.bytes = l.q_floats * 4 + l.bounds * 8 + l.s_words * 4 + l.c_keys * 8 + l.recs * sizeof(WideRec) + l.out_slots * (8 + 4 + 8 + 4) +
              l.per_query * (4 + 8);
    return l;
}

}  // namespace icd
