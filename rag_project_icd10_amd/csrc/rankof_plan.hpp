// rankof_plan.hpp - the host-visible part of the rank-of search: the limits, the split of the counting
// sweep into (query tile, row chunk) work-groups, the offsets of the per-(query, target) outputs, the workspace layout and the
// word of a row mask that holds real rows. No HIP header and no handle: included by rankof_kernel.hpp (the kernels call these
// very functions) and by tests/rankof_plan_check.cpp, which runs them under the host sanitizers.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "byrows_plan.hpp"   // br_row_of: the row a global id names

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RK_HD __host__ __device__
#else
#define RK_HD
#endif

namespace icd {

constexpr int RK_MAX_TARGETS = 16;                 // targets of one query (ICD_RANKOF_MAX_TARGETS)
constexpr int RK_TILE = 128;                       // rows of one sweep tile: the exact kernels' BN, a row mask's 16-byte unit
constexpr int RK_WAVES = 4;                        // waves of a sweep work-group
constexpr int RK_QUERIES = RK_WAVES * 32;          // queries of a sweep work-group: 32 per wave, the MFMA's N
constexpr int RK_THREADS = RK_WAVES * 64;
constexpr int RK_BK = 32;                          // floats of K per stage
constexpr int RK_TARGET_THREADS = 256;             // the target kernel: four lanes to a (query, target) slot
constexpr int RK_TARGET_SLOTS = RK_TARGET_THREADS / 4;

// The sweep's grid: mtiles query tiles x chunks row chunks, chunk c = rows [c rows_per_chunk, (c + 1) rows_per_chunk) cut at n.
// rows_per_chunk is a whole number of tiles, every chunk holds at least one row, and the chunks are as many as give every CU a
// work-group while a chunk keeps at least one tile - and no fewer than keep a chunk within RK_MAX_CHUNK_TILES tiles, so that
// rows_per_chunk and a chunk's last row + 1 fit an int at any n below 2^31.
constexpr long long RK_MAX_CHUNK_TILES = 1ll << 22;   // 2^29 rows
struct RankOfPlan {
    int mtiles, chunks, rows_per_chunk;
    long long grid;
};
RK_HD inline RankOfPlan rk_plan(long long nq, long long n, int num_cu) {
    RankOfPlan p;
    p.mtiles = (int)((nq + RK_QUERIES - 1) / RK_QUERIES);
    const long long row_tiles = (n + RK_TILE - 1) / RK_TILE;
    long long want = p.mtiles > 0 ? num_cu / p.mtiles : 1;
    const long long least = (row_tiles + RK_MAX_CHUNK_TILES - 1) / RK_MAX_CHUNK_TILES;
    want = want < least ? least : want;
    want = want < 1 ? 1 : (want > row_tiles ? row_tiles : want);
    const long long per = (row_tiles + want - 1) / want;   // tiles of a chunk
    p.chunks = (int)((row_tiles + per - 1) / per);
    p.rows_per_chunk = (int)(per * RK_TILE);
    p.grid = (long long)p.mtiles * p.chunks;
    return p;
}

// the output slot of target t of query q in a call with nt targets per query
RK_HD inline size_t rk_slot(long long q, int t, int nt) { return (size_t)q * (size_t)nt + (size_t)t; }

// work-groups of the target kernel for nq queries of nt targets
RK_HD inline long long rk_target_blocks(long long nq, int nt) { return (nq * nt + RK_TARGET_SLOTS - 1) / RK_TARGET_SLOTS; }

// The bits of the mask word that starts at row `row0` (a multiple of 32) which name rows of an index of n rows: the sweep counts
// and compares only those, whatever a bitset holds behind row n - 1.
RK_HD inline uint32_t rk_valid_bits(long long row0, long long n) {
    const long long left = n - row0;
    return left >= 32 ? 0xFFFFFFFFu : (left <= 0 ? 0u : ((1u << (int)left) - 1u));
}

// LDS of a sweep work-group: two stages of RK_TILE rows x (RK_BK + 1) floats
RK_HD inline size_t rk_sweep_lds_bytes() { return (size_t)2 * RK_TILE * (RK_BK + 1) * 4; }

// Elements of the workspace's arrays for calls of up to max_nq queries on an index of `dim` columns. Everything is allocated at
// create; a call allocates nothing.
struct RankOfLayout {
    size_t q_floats;    // [max_nq][dim]             a host caller's queries
    size_t slots;       // [max_nq][RK_MAX_TARGETS]  targets, target keys, ranks, adjusted and raw scores, levels; [nq][nt] used
    size_t per_query;   // [max_nq]                  selected
    size_t bytes;       // all of it
};
RK_HD inline RankOfLayout rk_layout(long long max_nq, int dim) {
    RankOfLayout l;
    l.q_floats = (size_t)max_nq * (size_t)dim;
    l.slots = (size_t)max_nq * RK_MAX_TARGETS;
    l.per_query = (size_t)max_nq;
    l.bytes = l.q_floats * 4 + l.slots * (8 + 8 + 8 + 8 + 4 + 4) + l.per_query * 8;
    return l;
}

}  // namespace icd
