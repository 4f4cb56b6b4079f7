// mask_select_plan.hpp - the arithmetic of the ordered select over row masks: how a bitset over n rows is cut
// into segments, the rank of a segment's first set row from the per-segment counts, and which part of a query's window
// [offset, offset + limit) falls into a segment. No HIP header and no handle: included by mask_select_kernel.hpp (the kernels call
// these very functions), by icd_range_mask.hpp (the scratch's size, the launch geometry) and by tests/mask_select_plan_check.cpp,
// which runs them under the host sanitizers.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define MS_HD __host__ __device__
#else
#define MS_HD
#endif

namespace icd {

constexpr int MS_THREADS = 256;                                      // lanes of a work-group: four waves
constexpr int MS_LANE_ROWS = 64;                                     // rows of ONE lane: two mask words, one 64-bit population count
constexpr long long MS_SEG_ROWS = (long long)MS_THREADS * MS_LANE_ROWS;   // rows of a segment: 16 384
constexpr long long MS_SEG_WORDS = MS_SEG_ROWS / 32;                 // its 32-bit mask words: 512
constexpr int MS_MAX_LIMIT = 16384;                                  // include/icd_search.h ICD_SELECT_MAX_LIMIT

// segments of a mask over n rows (0 for n <= 0)
MS_HD inline long long ms_segments(long long n) { return n <= 0 ? 0 : (n - 1) / MS_SEG_ROWS + 1; }

// rows of segment `seg` of an index of n rows: MS_SEG_ROWS, fewer in the last one, 0 behind it
MS_HD inline long long ms_segment_rows(long long n, long long seg) {
    const long long row0 = seg * MS_SEG_ROWS;
    if (seg < 0 || row0 >= n) return 0;
    return n - row0 < MS_SEG_ROWS ? n - row0 : MS_SEG_ROWS;
}

// the rank, among the mask's set rows, of the first set row of segment `seg`: the counts of the segments in front of it
MS_HD inline long long ms_base_rank(const int *counts, long long seg) {
    long long base = 0;
    for (long long s = 0; s < seg; ++s) base += counts[s];
    return base;
}

// the end of the window [offset, offset + limit): saturates instead of wrapping for an offset near 2^63
MS_HD inline long long ms_window_end(long long offset, int limit) {
    return offset > INT64_MAX - (long long)limit ? INT64_MAX : offset + limit;
}

// rows a query takes: clamp(total - offset, 0, limit)
MS_HD inline int ms_taken(long long total, long long offset, int limit) {
    if (total <= offset) return 0;
    const long long left = total - offset;
    return left < limit ? (int)left : limit;
}

// The part of the window that falls into a segment whose set rows hold the ranks [base, base + count).
struct MsPiece {
    int first;       // rank INSIDE the segment (0 .. count) of the first row taken
    int count;       // rows taken from the segment (0: the segment lies outside the window)
    long long out;   // position in the query's output list of that first row (0 .. limit)
};
MS_HD inline MsPiece ms_intersect(long long base, int count, long long offset, int limit) {
    const long long lo = base > offset ? base : offset;
    const long long seg_end = base + count, win_end = ms_window_end(offset, limit);
    const long long hi = seg_end < win_end ? seg_end : win_end;
    if (count <= 0 || limit <= 0 || hi <= lo) return MsPiece{0, 0, 0};
    return MsPiece{(int)(lo - base), (int)(hi - lo), lo - offset};
}

// a segment whose first rank is `base` lies wholly behind the window: so does every later one
MS_HD inline bool ms_past_window(long long base, long long offset, int limit) { return base >= ms_window_end(offset, limit); }

// int32 entries of the per-(query, segment) count scratch of an index of n rows and batches of up to max_nq queries
MS_HD inline long long ms_scratch_counts(long long n, long long max_nq) { return ms_segments(n) * (max_nq < 0 ? 0 : max_nq); }

// id slots of the staging a call with HOST outputs writes through (nq * limit above it: device outputs). 64 rows for every query
// of a full batch, and never less than four full windows.
MS_HD inline long long ms_host_slots(long long max_nq) {
    const long long per = (max_nq < 0 ? 0 : max_nq) * 64, least = 4ll * MS_MAX_LIMIT;
    return per > least ? per : least;
}

}  // namespace icd
