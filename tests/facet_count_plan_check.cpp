// Checker for rag_project_icd10_amd/csrc/facet_count_plan.hpp (host only; built by tests/test_facet_cpu.py with g++ and
// -fsanitize=address,undefined): the segment and lane of a row against mask_select_plan.hpp's segments, the choice of the
// accumulation form at the bound, the queries a result block holds, and the passes of a batch - that they cover every query once
// and never exceed the block or the grid. A walk over random masks and groupings then counts the way the kernel does - per
// (segment, lane), the lane's 64 bits, runs of equal groups - into heap blocks of exactly G entries (a bin out of range is an ASan
// report) and compares with a plain loop over the rows.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "facet_count_plan.hpp"

using namespace icd;

static int fails = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++fails; } } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

static void check_rows() {
    const long long S = MS_SEG_ROWS;
    EXPECT(fc_segment_of(0) == 0 && fc_lane_of(0) == 0);
    EXPECT(fc_segment_of(63) == 0 && fc_lane_of(63) == 0 && fc_lane_of(64) == 1);
    EXPECT(fc_segment_of(S - 1) == 0 && fc_lane_of(S - 1) == MS_THREADS - 1);
    EXPECT(fc_segment_of(S) == 1 && fc_lane_of(S) == 0);
    EXPECT(fc_segment_of(2 * S + 32) == 2 && fc_lane_of(2 * S + 32) == 0);
    const long long last = (1ll << 31) - 2;   // the last row a grouping can hold
    EXPECT(fc_segment_of(last) == ms_segments(last + 1) - 1 && fc_lane_of(last) == MS_THREADS - 1);
    for (long long n : {1ll, 33ll, S - 1, S, S + 1, 2 * S + 33}) {
        EXPECT(fc_segment_of(n - 1) == ms_segments(n) - 1);   // the last row lies in the last segment
        for (long long r = 0; r < n; r += 61) {
            const long long row0 = fc_segment_of(r) * S + (long long)fc_lane_of(r) * MS_LANE_ROWS;
            EXPECT(row0 <= r && r < row0 + MS_LANE_ROWS);
        }
    }
}

static void check_form() {
    EXPECT(FC_LDS_GROUPS * 4 <= 64 * 1024);
    EXPECT(fc_lds_form(1) && fc_lds_form(FC_LDS_GROUPS - 1) && fc_lds_form(FC_LDS_GROUPS));
    EXPECT(!fc_lds_form(FC_LDS_GROUPS + 1) && !fc_lds_form(1ll << 31) && !fc_lds_form(0) && !fc_lds_form(-3));
}

static void check_passes() {
    // the grouping's key block: qb x G x 8 bytes hold 2 qb queries of G int32 counts
    EXPECT(fc_block_queries(512ll * 17000 * 8, 17000) == 1024);
    EXPECT(fc_block_queries(32ll * 1 * 8, 1) == 64);
    EXPECT(fc_block_queries(0, 5) == 0 && fc_block_queries(100, 0) == 0 && fc_block_queries(19, 5) == 0 && fc_block_queries(20, 5) == 1);
    EXPECT(fc_block_queries(64ll * ((1ll << 31) - 1) * 8, (1ll << 31) - 1) == 128);   // no 32-bit product
    // device outputs (no block): one pass unless the grid says otherwise
    EXPECT(fc_pass_queries(300, -1, 3) == 300 && fc_passes(300, 300) == 1);
    EXPECT(fc_pass_queries(300, 64, 3) == 64 && fc_passes(300, 64) == 5);
    EXPECT(fc_pass_queries(64, 64, 3) == 64 && fc_passes(64, 64) == 1 && fc_passes(65, 64) == 2);
    EXPECT(fc_pass_queries(0, 64, 3) == 0 && fc_passes(0, 64) == 0 && fc_passes(-2, 64) == 0);
    EXPECT(fc_pass_queries(5, 0, 3) == 0 && fc_passes(5, 0) == -1);
    const long long segs = ms_segments((1ll << 31) - 1);   // 131 072
    EXPECT(fc_pass_queries(1ll << 20, -1, segs) == FC_MAX_GRID / segs && fc_pass_queries(1ll << 20, -1, segs) * segs <= FC_MAX_GRID);
    EXPECT(fc_pass_queries(7, -1, FC_MAX_GRID + 1) == 0);
    for (int round = 0; round < 500; ++round) {
        const long long nq = 1 + (long long)(rng() % 5000), block = (long long)(rng() % 3) == 0 ? -1 : 1 + (long long)(rng() % 700);
        const long long segments = 1 + (long long)(rng() % 1000000);
        const long long per = fc_pass_queries(nq, block, segments), passes = fc_passes(nq, per);
        EXPECT(per >= 1 && per <= nq && (block < 0 || per <= block) && per * segments <= FC_MAX_GRID);
        long long covered = 0;
        for (long long p = 0, q0 = 0; p < passes; ++p, q0 += per) covered += (nq - q0 < per ? nq - q0 : per);
        EXPECT(covered == nq && (passes - 1) * per < nq);
    }
}

// the kernel's walk on the host: per (segment, lane) the lane's 64 bits clipped at n, set rows in ascending order, runs of one group
// added at once
static void check_walk() {
    long cases = 0;
    for (int round = 0; round < 60; ++round) {
        const long long sizes[] = {1, 31, 32, 33, 64, 65, 257, MS_SEG_ROWS - 1, MS_SEG_ROWS, MS_SEG_ROWS + 1, 2 * MS_SEG_ROWS + 33};
        const long long n = sizes[round % 11];
        const int G = 1 + (int)(rng() % (round % 3 == 0 ? 3 : 700));
        int *dense_of = new int[n];
        for (long long r = 0; r < n; ++r) dense_of[r] = round % 2 ? (int)(r * G / n) : (int)(rng() % G);   // sorted (long runs) or random
        const long long words = (n + 63) / 64 * 2;
        uint32_t *mask = new uint32_t[words];
        for (long long w = 0; w < words; ++w) mask[w] = round % 5 == 0 ? 0xFFFFFFFFu : (uint32_t)rng() & (uint32_t)rng();   // (tail bits set: they must not count)
        int *got = new int[G](), *want = new int[G]();
        long long adds = 0;
        for (long long r = 0; r < n; ++r)
            if (mask[r >> 5] >> (r & 31) & 1) ++want[dense_of[r]];
        for (long long seg = 0; seg < ms_segments(n); ++seg)
            for (int lane = 0; lane < MS_THREADS; ++lane) {
                const long long row0 = seg * MS_SEG_ROWS + (long long)lane * MS_LANE_ROWS;
                if (row0 >= n) continue;
                unsigned long long bits = (unsigned long long)mask[row0 >> 5] | ((unsigned long long)mask[(row0 >> 5) + 1] << 32);
                if (n - row0 < MS_LANE_ROWS) bits &= (1ull << (n - row0)) - 1ull;
                int run_g = -1, run_c = 0;
                for (int b = 0; b < 64; ++b) {
                    if (!(bits >> b & 1)) continue;
                    EXPECT(fc_segment_of(row0 + b) == seg && fc_lane_of(row0 + b) == lane);
                    const int g = dense_of[row0 + b];
                    if (g == run_g) { ++run_c; continue; }
                    if (run_c) { got[run_g] += run_c; ++adds; }
                    run_g = g; run_c = 1;
                }
                if (run_c) { got[run_g] += run_c; ++adds; }
            }
        for (int g = 0; g < G; ++g) EXPECT(got[g] == want[g]);
        if (G == 1) EXPECT(adds <= (n + 63) / 64);   // one add per lane
        delete[] dense_of; delete[] mask; delete[] got; delete[] want;
        ++cases;
    }
    printf("%ld masks walked\n", cases);
}

int main() {
    check_rows();
    check_form();
    check_passes();
    check_walk();
    if (fails) { printf("%d checks FAILED\n", fails); return 1; }
    printf("facet count plan ok\n");
    return 0;
}
