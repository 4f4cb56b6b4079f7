// text_match_kernel.hpp - keyword match filters: the row mask of TEXT_MATCH(field, "tokens",
// minimum_should_match = m), one per query of a batch, built from the sparse index's postings on the device.
//
// Replaces, on the device, the bitset a Milvus query node builds for a TEXT_MATCH predicate before the scan; the reference has no
// text predicate and no code of its own for one (services/milvus_service.py:280-285 is its only search call).
//
// text_match_mask_kernel: one work-group of 256 lanes per (query, tile of SP_TILE consecutive rows) - the tile geometry and the
// segment search of sparse_accumulate_select_kernel (sparse_kernel.hpp). The tile's per-row match counters live in LDS as packed
// bytes, four rows per 32-bit word: a posting of row l is ONE LDS atomic add of 1 << 8 * (l & 3) on word l >> 2. A query carries at
// most 64 terms and a term holds a row once, so a byte never exceeds 64 and never carries into its neighbour. Integer counts do
// not depend on the order of the adds: every wave walks its own terms (wave w takes terms w, w + 4, ...) with no barrier between
// terms. Behind ONE barrier lane l owns mask word l of the tile (rows 32 l .. 32 l + 31: counter words 8 l .. 8 l + 7, two 16-byte
// LDS reads), sets bit j where count >= m, clears the rows at or behind n, ANDs the optional base mask's word and writes the word
// with an ordinary vector store; the words' popcounts are summed per wave and added to the mask's row counter with one global
// (vector) atomic add per wave.
//
// The four steps are device functions (tm_segment_search, tm_counter_walk, tm_threshold_word, tm_store_word): filter_mask_kernel
// (filter_mask_kernel.hpp) runs the first three for a TEXT leaf and the last for its final word. The LDS arrays are the kernels'
// own, and so are the barriers between the steps. GUARDED tells the two callers apart at compile time: text_match_mask_kernel
// takes queries a device caller wrote (a term at or behind the vocabulary has no postings, m outside 1 .. SP_MAX_TERMS matches
// nothing; the kernel itself clamps the term count), filter_mask_kernel walks programs the host checked (only m above the leaf's
// term count is left to test).
//
// The bitset is icd_rowmask's (topk_select.hpp): row r = bit r & 31 of word r >> 5, whole 128-row tiles; every word below
// rowmask_tile_words(n) is written, also for a query without a known term or with m above its term count (zero words). The
// ROWMASK_TAIL_WORDS behind them are zeroed by the caller.
//
// LDS: 8 KB counters + 1 KB segment bounds + 256 B terms = 9.3 KB. No scratch.
#pragma once
#include "sparse_kernel.hpp"

namespace icd {

constexpr int TM_COUNT_WORDS = SP_TILE / 4;          // packed byte counters of a tile
constexpr int TM_TILE_WORDS = SP_TILE / 32;          // mask words of a tile: one per lane
static_assert(TM_TILE_WORDS == SP_THREADS, "lane l owns mask word l of the tile");
static_assert(SP_MAX_TERMS <= 127, "a byte counter plus the 0x80 - m bias must stay below 256");

struct TextMatchArgs {
    const long long *post_off;   // [vocab + 1]
    const uint32_t *post_row;    // [nnz] ascending within a term
    long long vocab;
    const long long *q_off;      // [nq + 1]
    const uint32_t *q_terms;     // ascending within a query
    const int *min_match;        // [nq] m of every query, 1 .. SP_MAX_TERMS (anything else matches nothing)
    const uint32_t *const *base; // nullable: [query] -> base bitset (nullable entries: unfiltered)
    uint32_t *bits;              // [nq][stride] the produced bitsets
    long long stride;            // words between two queries' bitsets
    int *count;                  // [nq] rows of every produced mask (zeroed by the caller)
    long long n;                 // rows of the index
    long long mask_words;        // rowmask_tile_words(n)
    int tiles;
};

// 1. the tile's segment of every term's postings: lane 2 t finds its begin, lane 2 t + 1 its end (terms: the nt terms, in LDS)
template <bool GUARDED, typename Args>
__device__ __forceinline__ void tm_segment_search(const Args &a, const uint32_t *terms, int nt, uint32_t tile0, int tid, long long *seg) {
    if (tid < 2 * nt) {
        const uint32_t term = terms[tid >> 1];
        const u64 target = (u64)tile0 + ((tid & 1) ? (u64)SP_TILE : 0ull);
        long long lo = 0, hi = 0;
        bool known = true;
        if constexpr (GUARDED) known = (long long)term < a.vocab;
        if (known) { lo = a.post_off[term]; hi = a.post_off[term + 1]; }
        while (lo < hi) {   // first posting whose row is at or behind target
            const long long mid = (lo + hi) >> 1;
            if ((u64)a.post_row[mid] < target) lo = mid + 1; else hi = mid;
        }
        seg[tid] = lo;
    }
}

// 2. the walk: a wave per term, no barrier between terms (integer adds commute)
template <typename Args>
__device__ __forceinline__ void tm_counter_walk(const Args &a, const long long *seg, int nt, uint32_t tile0, int wave, int lane, uint32_t *cnt) {
    for (int t = wave; t < nt; t += SP_THREADS / 64) {
        const long long lo = seg[2 * t], hi = seg[2 * t + 1];
        for (long long i = lo + lane; i < hi; i += 64) {
            const uint32_t l = a.post_row[i] - tile0;
            if (l < (uint32_t)SP_TILE) atomicAdd(&cnt[l >> 2], 1u << (8 * (l & 3)));   // (always, for postings icd_sparse_pack built)
        }
    }
}

// 3. lane l's mask word: bit j = row 32 l + j of the tile holds at least m of the nt terms
template <bool GUARDED>
__device__ __forceinline__ uint32_t tm_threshold_word(const uint32_t *cnt, int m, int nt, int tid) {
    uint32_t word = 0u;
    if (GUARDED ? (m >= 1 && m <= SP_MAX_TERMS) : (m <= nt)) {   // (checked programs hold m in 1 .. 64; m above nt is the empty set)
        const uint32_t bias = (uint32_t)(0x80 - m) * 0x01010101u;   // count + 0x80 - m sets a byte's top bit iff count >= m
        const uint4 *c4 = reinterpret_cast<const uint4 *>(cnt) + 2 * tid;
        const uint4 c0 = c4[0], c1 = c4[1];
        const uint32_t w8[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
#pragma unroll
        for (int j = 7; j >= 0; --j) {   // (the nibbles shifted in from the top one down: a chain the compiler keeps in 14 registers)
            const uint32_t top = ((w8[j] + bias) >> 7) & 0x01010101u;
            word = (word << 4) | ((top | (top >> 7) | (top >> 14) | (top >> 21)) & 0xFu);
        }
    }
    return word;
}

// 4. the final word of lane `tid`: rows at or behind n cleared, the base mask, the store, the rows counted (one atomic per wave)
template <typename Args>
__device__ __forceinline__ void tm_store_word(const Args &a, uint32_t word, int q, uint32_t tile0, int tid, int lane) {
    const long long gw = (long long)(tile0 >> 5) + tid;   // the word's index in the bitset
    const long long row0 = gw * 32;
    if (row0 + 32 > a.n) word &= row0 < a.n ? (1u << (int)(a.n - row0)) - 1u : 0u;
    if (gw < a.mask_words) {
        const uint32_t *base = a.base ? a.base[q] : nullptr;
        if (base) word &= base[gw];
        a.bits[(size_t)q * a.stride + gw] = word;
    } else {
        word = 0u;
    }
    int pc = __popc(word);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) pc += __shfl_down(pc, off, 64);
    if (lane == 0 && pc) atomicAdd(a.count + q, pc);
}

__global__ __launch_bounds__(SP_THREADS) void text_match_mask_kernel(const TextMatchArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t cnt[TM_COUNT_WORDS];
    __shared__ long long seg[2 * SP_MAX_TERMS];
    __shared__ uint32_t qt[SP_MAX_TERMS];
    const int tid = threadIdx.x;
    const int q = (int)(blockIdx.x / (unsigned)a.tiles), tile = (int)(blockIdx.x - (unsigned)q * (unsigned)a.tiles);
    const uint32_t tile0 = (uint32_t)tile * (uint32_t)SP_TILE;

    // 0. empty counters; the query's terms (a device caller's offsets are clamped: never more than SP_MAX_TERMS, never backwards)
    for (int i = tid; i < TM_COUNT_WORDS; i += SP_THREADS) cnt[i] = 0u;
    const long long qa = a.q_off[q];
    long long qn = a.q_off[q + 1] - qa;
    qn = qn < 0 ? 0 : (qn > SP_MAX_TERMS ? SP_MAX_TERMS : qn);
    const int nt = (int)qn;
    if (tid < nt) qt[tid] = a.q_terms[qa + tid];
    __syncthreads();
    tm_segment_search<true>(a, qt, nt, tile0, tid, seg);
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    tm_counter_walk(a, seg, nt, tile0, wave, lane, cnt);
    __syncthreads();
    const uint32_t word = tm_threshold_word<true>(cnt, a.min_match[q], nt, tid);
    tm_store_word(a, word, q, tile0, tid, lane);
}

}  // namespace icd
