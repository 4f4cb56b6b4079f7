// mask_select_kernel.hpp - the ordered select over a batch of row masks: for every query of a batch the
// number of rows its mask holds and the rows of ranks offset .. offset + limit of that mask in ascending row order. What a Milvus
// `query` / `count(*)` / `query_iterator` does with a filter's bitset once no vector is involved; the reference has no such call
// (services/milvus_service.py:280-285 is its only read of the collection).
//
// Two launches over the same grid, one work-group of MS_THREADS lanes per (query, segment of MS_SEG_ROWS rows), the segment the
// fast index (grid y ends at 65 535, a batch may be longer):
//   mask_count_kernel    lane l reads mask words 2 l and 2 l + 1 of the segment as ONE 8-byte load, clears the bits of rows at or
//                        behind n (whatever the buffer holds there), counts them with one 64-bit population count; the work-group's
//                        sum goes to counts[query][segment]. A NULL mask counts the segment's rows without a load.
//   mask_select_kernel   the work-group sums the counts in front of its segment - its base rank - in chunks of MS_THREADS and stops
//                        as soon as the base lies behind the window; a segment outside [offset, offset + limit) ends there. Inside
//                        it every lane reloads its 64 bits; the exclusive prefix of the lanes' population counts (six shuffle steps
//                        inside a wave, the four waves' sums through LDS) is the rank of the lane's first set row; the lane walks
//                        its set bits and stores the rows whose rank falls into the window at out + (rank - first). The work-group
//                        of segment 0 also sums ALL counts: the query's total, its taken, and -1 behind the taken rows.
// Every output position is written by exactly one lane, at an address that depends on the masks alone: no atomic touches the
// outputs, the result is the same bytes on every run. Ranks and totals are 64-bit; a row is segment * MS_SEG_ROWS + 64 lane + bit
// in 64-bit arithmetic.
//
// LDS: 4 x 8 bytes. No scratch.
#pragma once
#include "mask_select_plan.hpp"

namespace icd {

static_assert(MS_THREADS == 256 && MS_LANE_ROWS == 64, "four waves of 64 lanes, one 64-bit word per lane");

struct MaskSelectArgs {
    const uint32_t *const *masks;   // [nq] -> bitset in icd_rowmask_pack's layout (an entry may be NULL: every row of the index)
    const long long *offsets;       // [nq] (nullptr: 0 for every query)
    int *counts;                    // [nq][segments]
    long long *ids;                 // [nq][limit] (nullptr: count only)
    long long *total;               // [nq]
    int *taken;                     // [nq] (nullable)
    long long n;                    // rows of the index
    long long mask_words;           // rowmask_tile_words(n): the words a mask's buffer holds (a multiple of 4)
    int segments;                   // ms_segments(n)
    int limit;
};

// The 64 rows of lane `tid` of segment `seg` as a bit set: bit b = row seg * MS_SEG_ROWS + 64 tid + b. Rows at or behind n read 0;
// words at or behind mask_words are not loaded.
__device__ __forceinline__ unsigned long long ms_lane_bits(const uint32_t *__restrict__ mask, long long n, long long mask_words, long long seg, int tid) {
    const long long row0 = seg * MS_SEG_ROWS + (long long)tid * MS_LANE_ROWS;
    if (row0 >= n) return 0ull;
    unsigned long long bits = ~0ull;
    if (mask) {
        const long long w = row0 >> 5;   // (even: the pair is 8-byte aligned; mask_words is even, so the pair lies inside or outside)
        if (w >= mask_words) return 0ull;
        const uint2 v = *reinterpret_cast<const uint2 *>(mask + w);
        bits = (unsigned long long)v.x | ((unsigned long long)v.y << 32);
    }
    const long long left = n - row0;
    if (left < MS_LANE_ROWS) bits &= (1ull << left) - 1ull;
    return bits;
}

// sum of v over the work-group, the same value in every lane (two barriers; `lds` holds one entry per wave)
__device__ __forceinline__ long long ms_block_sum(long long v, long long *lds, int tid) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    __syncthreads();   // (whoever still reads lds from the round before)
    if ((tid & 63) == 0) lds[tid >> 6] = v;
    __syncthreads();
    return lds[0] + lds[1] + lds[2] + lds[3];
}

__global__ __launch_bounds__(MS_THREADS) void mask_count_kernel(const MaskSelectArgs a) {
    __shared__ long long lds[MS_THREADS / 64];
    const int tid = threadIdx.x;
    const long long q = blockIdx.x / (unsigned)a.segments, seg = blockIdx.x - (unsigned)q * (unsigned)a.segments;
    const uint32_t *mask = a.masks[q];
    long long count;
    if (!mask) {   // (uniform: no load, no reduction)
        count = ms_segment_rows(a.n, seg);
    } else {
        count = ms_block_sum(__popcll(ms_lane_bits(mask, a.n, a.mask_words, seg, tid)), lds, tid);
    }
    if (tid == 0) a.counts[q * a.segments + seg] = (int)count;
}

__global__ __launch_bounds__(MS_THREADS) void mask_select_kernel(const MaskSelectArgs a) {
    __shared__ long long lds[MS_THREADS / 64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const long long q = blockIdx.x / (unsigned)a.segments, seg = blockIdx.x - (unsigned)q * (unsigned)a.segments;
    const int *__restrict__ counts = a.counts + q * a.segments;
    const long long offset = a.offsets ? a.offsets[q] : 0;

    if (seg == 0) {   // the query's total, its taken, the padding behind the taken rows
        long long total = 0;
        for (long long c = 0; c < a.segments; c += MS_THREADS)
            total += ms_block_sum(c + tid < a.segments ? counts[c + tid] : 0, lds, tid);
        const int taken = ms_taken(total, offset, a.limit);
        if (tid == 0) {
            a.total[q] = total;
            if (a.taken) a.taken[q] = taken;
        }
        if (a.ids)
            for (int j = taken + tid; j < a.limit; j += MS_THREADS) a.ids[q * a.limit + j] = -1;
    }
    if (!a.ids) return;

    // the base rank: the counts in front of this segment (ms_base_rank, MS_THREADS of them per round)
    long long base = 0;
    for (long long c = 0; c < seg; c += MS_THREADS) {
        base += ms_block_sum(c + tid < seg ? counts[c + tid] : 0, lds, tid);
        if (ms_past_window(base, offset, a.limit)) return;   // (the same in every lane)
    }
    const MsPiece piece = ms_intersect(base, counts[seg], offset, a.limit);
    if (piece.count == 0) return;

    const unsigned long long bits = ms_lane_bits(a.masks[q], a.n, a.mask_words, seg, tid);
    const int pc = __popcll(bits);
    int incl = pc;   // inclusive prefix over the wave's lanes
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    __syncthreads();   // (the base rounds' last reads of lds)
    if (lane == 63) lds[wave] = incl;
    __syncthreads();
    int rank = incl - pc;   // rank inside the segment of this lane's first set row
    for (int w = 0; w < wave; ++w) rank += (int)lds[w];

    const int first = piece.first, last = piece.first + piece.count;   // ranks [first, last) are taken
    if (rank + pc <= first || rank >= last) return;
    long long *__restrict__ out = a.ids + q * a.limit + piece.out;
    const long long row0 = seg * MS_SEG_ROWS + (long long)tid * MS_LANE_ROWS;
    unsigned long long rest = bits;
    while (rest && rank < last) {
        const int b = __ffsll((long long)rest) - 1;
        rest &= rest - 1ull;
        if (rank >= first) out[rank - first] = row0 + b;
        ++rank;
    }
}

}  // namespace icd
