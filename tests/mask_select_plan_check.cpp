// Checker for rag_project_icd10_amd/csrc/mask_select_plan.hpp (host only; built by tests/test_mask_select_cpu.py with g++ and
// -fsanitize=address,undefined): the segment count, the base rank of a segment from a count array, the window / segment
// intersection at both edges, and - over random masks - that the pieces of all segments tile exactly the window a brute-force walk
// over the mask selects. The count arrays are heap blocks of exactly `segments` entries: a read past the last count in front of a
// segment is an ASan report.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "mask_select_plan.hpp"

using namespace icd;

static int fails = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++fails; } } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

static void check_segments() {
    const long long S = MS_SEG_ROWS;
    EXPECT(S == 16384 && MS_SEG_WORDS * 32 == S && (long long)MS_THREADS * MS_LANE_ROWS == S);
    EXPECT(ms_segments(0) == 0 && ms_segments(-5) == 0);
    EXPECT(ms_segments(1) == 1);
    EXPECT(ms_segments(S - 1) == 1);
    EXPECT(ms_segments(S) == 1);
    EXPECT(ms_segments(S + 1) == 2);
    EXPECT(ms_segments(2 * S) == 2);
    EXPECT(ms_segments(2 * S + 1) == 3);
    const long long big = (1ll << 31) + 5;
    EXPECT(ms_segments(big) == (1ll << 31) / S + 1);   // 131 073: the five rows behind 2^31 open a segment of their own
    for (long long n : {1ll, S - 1, S, S + 1, 2 * S, 2 * S + 33, big}) {
        long long rows = 0;
        const long long segs = ms_segments(n);
        for (long long s = (segs > 4 ? segs - 4 : 0); s < segs; ++s) rows += ms_segment_rows(n, s);
        rows += (segs > 4 ? segs - 4 : 0) * S;
        EXPECT(rows == n);                                   // the segments hold every row once
        EXPECT(ms_segment_rows(n, segs - 1) >= 1 && ms_segment_rows(n, segs - 1) <= S);
        EXPECT(ms_segment_rows(n, segs) == 0 && ms_segment_rows(n, -1) == 0);
    }
    EXPECT(ms_scratch_counts(2 * S + 33, 300) == 900 && ms_scratch_counts(1, 0) == 0 && ms_scratch_counts(0, 7) == 0);
    EXPECT(ms_host_slots(16384) == 16384ll * 64 && ms_host_slots(8) == 4ll * MS_MAX_LIMIT && ms_host_slots(-1) == 4ll * MS_MAX_LIMIT);
}

static void check_base_ranks() {
    int *counts = new int[5]{7, 0, 16384, 3, 100};
    EXPECT(ms_base_rank(counts, 0) == 0);
    EXPECT(ms_base_rank(counts, 1) == 7);
    EXPECT(ms_base_rank(counts, 2) == 7);
    EXPECT(ms_base_rank(counts, 3) == 16391);
    EXPECT(ms_base_rank(counts, 4) == 16394);
    EXPECT(ms_base_rank(counts, 5) == 16494);   // (the total)
    delete[] counts;
    // more than 2^31 rows in front of a segment: the rank is 64-bit
    const long long segs = 140000;
    int *full = new int[segs];
    for (long long s = 0; s < segs; ++s) full[s] = (int)MS_SEG_ROWS;
    EXPECT(ms_base_rank(full, segs) == segs * MS_SEG_ROWS && ms_base_rank(full, segs) > (1ll << 31));
    delete[] full;
}

static void check_intersections() {
    // a segment with ranks [100, 150)
    MsPiece p = ms_intersect(100, 50, 0, 100);       // the window ends where the segment begins
    EXPECT(p.count == 0);
    p = ms_intersect(100, 50, 0, 101);               // ... one further: the segment's first row is the window's last
    EXPECT(p.first == 0 && p.count == 1 && p.out == 100);
    p = ms_intersect(100, 50, 149, 10);              // the window begins at the segment's last row
    EXPECT(p.first == 49 && p.count == 1 && p.out == 0);
    p = ms_intersect(100, 50, 150, 10);              // ... and one behind it
    EXPECT(p.count == 0);
    p = ms_intersect(100, 50, 100, 50);              // exactly the segment
    EXPECT(p.first == 0 && p.count == 50 && p.out == 0);
    p = ms_intersect(100, 50, 99, 52);               // the segment inside the window
    EXPECT(p.first == 0 && p.count == 50 && p.out == 1);
    p = ms_intersect(100, 50, 120, 5);               // the window inside the segment
    EXPECT(p.first == 20 && p.count == 5 && p.out == 0);
    p = ms_intersect(100, 0, 100, 5);                // an empty segment
    EXPECT(p.count == 0);
    p = ms_intersect(100, 50, 120, 0);               // an empty window
    EXPECT(p.count == 0);
    p = ms_intersect(100, 50, 1000, 16384);          // a window past the total
    EXPECT(p.count == 0);
    p = ms_intersect(100, 50, INT64_MAX - 3, 16384); // ... at the end of the offsets: no wrap
    EXPECT(p.count == 0);
    EXPECT(ms_window_end(INT64_MAX - 3, 16384) == INT64_MAX && ms_window_end(5, 7) == 12);
    EXPECT(ms_past_window(12, 5, 7) && !ms_past_window(11, 5, 7) && !ms_past_window(INT64_MAX - 1, INT64_MAX - 3, 16384));
    EXPECT(ms_taken(10, 0, 3) == 3 && ms_taken(10, 8, 3) == 2 && ms_taken(10, 10, 3) == 0 && ms_taken(10, 15, 3) == 0 && ms_taken(0, 0, 16384) == 0);
    EXPECT(ms_taken((1ll << 40), 5, 16384) == 16384 && ms_taken(10, INT64_MAX, 1) == 0);
}

// the pieces of all segments against a walk over the mask: every output position of the window is covered exactly once, by the row
// the walk puts there
static void check_tiling() {
    long cases = 0;
    for (int round = 0; round < 200; ++round) {
        const long long segs = 1 + (long long)(rng() % 6);
        const long long S = 64;   // (the arithmetic does not know the segment's size: small ones keep the walk short)
        std::vector<int> counts((size_t)segs);
        std::vector<long long> rows;   // the "set rows": segment s holds counts[s] of them, row = s * S + j
        for (long long s = 0; s < segs; ++s) {
            counts[(size_t)s] = (int)(rng() % 4 == 0 ? 0 : rng() % (S + 1));
            for (int j = 0; j < counts[(size_t)s]; ++j) rows.push_back(s * S + j);
        }
        const long long total = (long long)rows.size();
        EXPECT(ms_base_rank(counts.data(), segs) == total);
        const long long offsets[] = {0, 1, total / 2, total > 0 ? total - 1 : 0, total, total + 5};
        const int limits[] = {1, 7, 64, 16384};
        for (long long offset : offsets)
            for (int limit : limits) {
                const int taken = ms_taken(total, offset, limit);
                std::vector<long long> out((size_t)taken, -1);
                int covered = 0;
                bool past = false;
                for (long long s = 0; s < segs; ++s) {
                    const long long base = ms_base_rank(counts.data(), s);
                    const MsPiece p = ms_intersect(base, counts[(size_t)s], offset, limit);
                    if (past) EXPECT(p.count == 0);
                    if (ms_past_window(base, offset, limit)) past = true;
                    if (past) EXPECT(p.count == 0);
                    EXPECT(p.count >= 0 && p.first >= 0 && p.first + p.count <= counts[(size_t)s]);
                    for (int j = 0; j < p.count; ++j) {
                        EXPECT(p.out + j < taken);
                        if (p.out + j < taken) {
                            EXPECT(out[(size_t)(p.out + j)] == -1);
                            out[(size_t)(p.out + j)] = s * S + p.first + j;
                            ++covered;
                        }
                    }
                }
                EXPECT(covered == taken);
                for (int j = 0; j < taken; ++j) EXPECT(out[(size_t)j] == rows[(size_t)(offset + j)]);
                ++cases;
            }
    }
    printf("%ld windows tiled\n", cases);
}

int main() {
    check_segments();
    check_base_ranks();
    check_intersections();
    check_tiling();
    if (fails) { printf("%d checks FAILED\n", fails); return 1; }
    printf("mask select plan ok\n");
    return 0;
}
