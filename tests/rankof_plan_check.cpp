// rankof_plan_check.cpp - host check of rag_project_icd10_amd/csrc/rankof_plan.hpp, built with
// -fsanitize=address,undefined and run by tests/test_rankof_cpu.py: the limits, the sweep's split into query tiles and row chunks
// (every row in exactly one chunk, whole tiles, no empty chunk, the grid within 2^31), the output offsets, the valid bits of a
// mask word at every distance from the end of the index, and the workspace layout. It then replays the sweep's bookkeeping with
// the header's own functions - chunk by chunk, tile by tile, mask word by mask word, on heap buffers of EXACTLY the sizes the
// kernel may touch - against a plain count.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rankof_plan.hpp"

using namespace icd;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

// the sweep's walk for one query: admitted rows ahead of the target, and `selected`, summed over the plan's chunks
static void sweep_walk(const RankOfPlan &p, long long n, const std::vector<uint32_t> &mask, const std::vector<int> &score, int target,
                       long long *ahead, long long *selected) {
    *ahead = 0;
    *selected = 0;
    std::vector<int> seen((size_t)n, 0);
    for (int chunk = 0; chunk < p.chunks; ++chunk) {
        const long long row_begin = (long long)chunk * p.rows_per_chunk;
        const long long row_end = row_begin + p.rows_per_chunk < n ? row_begin + p.rows_per_chunk : n;
        CHECK(row_begin < row_end);   // no empty chunk
        for (long long tile = row_begin; tile < row_end; tile += RK_TILE) {
            CHECK(tile % RK_TILE == 0);
            for (int t = 0; t < 4; ++t) {
                const uint32_t w = mask.at((size_t)((tile >> 5) + t)) & rk_valid_bits(tile + 32 * t, n);   // (.at: a word past the bitset throws)
                *selected += __builtin_popcount(w);
                for (int b = 0; b < 32; ++b) {
                    const long long row = tile + 32 * t + b;
                    if (row < n) ++seen.at((size_t)row);
                    if (!((w >> b) & 1u)) continue;
                    CHECK(row < n);
                    if (score.at((size_t)row) > score.at((size_t)target) || (score.at((size_t)row) == score.at((size_t)target) && row < target)) ++*ahead;
                }
            }
        }
    }
    for (long long r = 0; r < n; ++r) CHECK(seen[(size_t)r] == 1);   // every row in exactly one chunk
}

int main() {
    // limits and geometry
    CHECK(RK_MAX_TARGETS == 16 && RK_TILE == 128 && RK_QUERIES == 128 && RK_THREADS == 256 && RK_TARGET_SLOTS == 64);
    CHECK(rk_sweep_lds_bytes() == 33792 && rk_sweep_lds_bytes() <= 65536);
    CHECK(rk_target_blocks(1, 1) == 1 && rk_target_blocks(4, 16) == 1 && rk_target_blocks(5, 16) == 2 && rk_target_blocks(300, 16) == 75);
    CHECK(rk_slot(0, 0, 16) == 0 && rk_slot(3, 5, 16) == 53 && rk_slot(7, 0, 1) == 7 && rk_slot(0x7FFFFFFll, 15, 16) == (size_t)0x7FFFFFFll * 16 + 15);
    // the plan: every nq and n around the tile edges, several CU counts
    const long long ns[] = {1, 2, 63, 64, 65, 127, 128, 129, 257, 261, 4099, 40474, 1250000, 0x7FFFFFFFll};
    const long long nqs[] = {1, 5, 40, 127, 128, 129, 300, 1000, 16384};
    const int cus[] = {1, 64, 256, 304};
    for (long long n : ns)
        for (long long nq : nqs)
            for (int cu : cus) {
                const RankOfPlan p = rk_plan(nq, n, cu);
                const long long row_tiles = (n + RK_TILE - 1) / RK_TILE;
                CHECK(p.mtiles == (nq + RK_QUERIES - 1) / RK_QUERIES && (long long)p.mtiles * RK_QUERIES >= nq);
                CHECK(p.chunks >= 1 && p.chunks <= row_tiles && p.rows_per_chunk % RK_TILE == 0 && p.rows_per_chunk >= RK_TILE);
                CHECK((long long)p.chunks * p.rows_per_chunk >= n);                 // the chunks cover the index ...
                CHECK((long long)(p.chunks - 1) * p.rows_per_chunk < n);           // ... and the last one holds a row
                CHECK(p.grid == (long long)p.mtiles * p.chunks && p.grid <= 0x7FFFFFFFll);
                const long long least = (row_tiles + RK_MAX_CHUNK_TILES - 1) / RK_MAX_CHUNK_TILES;
                const long long per_cu = cu / p.mtiles > 1 ? cu / p.mtiles : 1;
                CHECK(p.chunks <= (per_cu > least ? per_cu : least));               // no more chunks than give every CU a work-group ...
                CHECK((long long)p.rows_per_chunk <= RK_MAX_CHUNK_TILES * RK_TILE);  // ... unless a chunk would outgrow an int
            }
    // the valid bits of a mask word
    for (long long n = 1; n <= 300; ++n)
        for (long long row0 = 0; row0 < 384; row0 += 32) {
            const uint32_t v = rk_valid_bits(row0, n);
            for (int b = 0; b < 32; ++b) CHECK(((v >> b) & 1u) == (row0 + b < n ? 1u : 0u));
        }
    CHECK(rk_valid_bits(0x7FFFFFE0ll, 0x7FFFFFFFll) == 0x7FFFFFFFu);
    // the layout: no 32-bit wrap at the largest workspace icd_rankof_create accepts
    {
        const RankOfLayout l = rk_layout(300, 768);
        CHECK(l.q_floats == (size_t)300 * 768 && l.slots == (size_t)300 * 16 && l.per_query == 300);
        CHECK(l.bytes == l.q_floats * 4 + l.slots * 40 + l.per_query * 8);
        const RankOfLayout big = rk_layout(0x7FFFFFFFll / 16, 4096);
        CHECK(big.q_floats == (size_t)(0x7FFFFFFFll / 16) * 4096 && big.bytes > big.q_floats * 4);
    }
    // the sweep's bookkeeping against a plain count: masks with garbage behind row n - 1, ties, every target position
    std::srand(11);
    for (long long n : {1ll, 2ll, 63ll, 64ll, 65ll, 127ll, 128ll, 129ll, 257ll, 261ll, 700ll})
        for (int cu : {1, 3, 256}) {
            const RankOfPlan p = rk_plan(5, n, cu);
            std::vector<uint32_t> mask((size_t)((n + RK_TILE - 1) / RK_TILE * 4));
            for (uint32_t &w : mask) w = (uint32_t)std::rand() * 2654435761u;   // (bits behind n - 1 too: rk_valid_bits cuts them)
            std::vector<int> score((size_t)n);
            for (int &s : score) s = std::rand() % 5;
            for (long long target : {0ll, n - 1, n / 2, (long long)RK_TILE - 1, (long long)RK_TILE}) {
                if (target >= n) continue;
                long long want_ahead = 0, want_sel = 0;
                for (long long r = 0; r < n; ++r) {
                    if (!((mask[(size_t)(r >> 5)] >> (r & 31)) & 1u)) continue;
                    ++want_sel;
                    if (score[(size_t)r] > score[(size_t)target] || (score[(size_t)r] == score[(size_t)target] && r < target)) ++want_ahead;
                }
                long long ahead, sel;
                sweep_walk(p, n, mask, score, (int)target, &ahead, &sel);
                CHECK(ahead == want_ahead && sel == want_sel);
            }
        }
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("rankof plan ok\n");
    return 0;
}
