// wide_select_plan.hpp on the host, under ASan and UBSan (tests/test_wide_cpu.py builds and runs this): the score block against
// its byte budget, the tier choice at every edge, the offsets at the largest index and batch without 32-bit overflow, and the digit
// split covering all 32 bits.
#include <cstdio>
#include <cstdlib>

#include "wide_select_plan.hpp"

using namespace icd;

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            std::exit(1);                                                   \
        }                                                                   \
    } while (0)

int main() {
    // the score block: within the budget, at most max_nq, whole sweep work-groups where it cuts a batch
    const long long ns[] = {1, 127, 128, 129, 40474, 1000000, 50000000, 0x7FFFFFFFll};
    const int ks[] = {1, 128, 1024, 4096, 16384};
    const long long nqs[] = {1, 5, 127, 128, 129, 1000, 16384, WS_MAX_NQ};
    for (long long n : ns)
        for (int k : ks)
            for (long long nq : nqs) {
                const long long b = ws_block_queries(nq, n, k);
                const size_t per = ws_query_bytes(n, k);
                CHECK(per >= (size_t)n * 4 && ws_padded_rows(n) % RK_TILE == 0 && ws_padded_rows(n) >= n && ws_padded_rows(n) < n + RK_TILE);
                CHECK(b >= 0 && b <= nq);
                CHECK((size_t)b * per <= WS_BLOCK_BUDGET || b == nq);
                if (b == nq) CHECK((size_t)nq * per <= WS_BLOCK_BUDGET || WS_BLOCK_BUDGET / per >= (size_t)nq);
                if (b < nq) {
                    CHECK((size_t)(b + 1) * per > WS_BLOCK_BUDGET || b % RK_QUERIES == 0);
                    CHECK(b < RK_QUERIES || b % RK_QUERIES == 0);
                }
                CHECK((b == 0) == (per > WS_BLOCK_BUDGET));
                if (b > 0) {
                    const WideLayout l = ws_layout(nq, k, n, 768);
                    CHECK(l.block == b && l.n_pad == ws_padded_rows(n));
                    CHECK(l.s_words * 4 + l.c_keys * 8 + l.out_slots * 24 <= WS_BLOCK_BUDGET);
                    CHECK(l.bytes > l.s_words * 4 && l.q_floats == (size_t)nq * 768 && l.recs == (size_t)b);
                }
            }
    CHECK(ws_block_queries(1000, 40474, 16384) == 384);          // 256 MiB / (40 576 x 4 + 16 384 x 32) = 390 -> three work-groups
    CHECK(ws_block_queries(1, 0x7FFFFFFFll, 1) == 0);            // 8 GiB of scores for one query: refused at create
    CHECK(ws_block_queries(4, 50000000, 16384) == 1);

    // tiers
    CHECK(ws_tier(1) == 0 && ws_tier(1024) == 0 && ws_tier(1025) == 1 && ws_tier(4096) == 1 && ws_tier(4097) == 2 && ws_tier(16384) == 2);
    for (int t = 0; t < WS_TIERS; ++t) {
        CHECK(ws_tier(ws_tier_keys(t)) == t && ws_tier_lds_bytes(t) == (size_t)ws_tier_keys(t) * 8);
        CHECK((ws_tier_keys(t) & (ws_tier_keys(t) - 1)) == 0 && ws_tier_threads(t) % 64 == 0 && ws_tier_threads(t) <= 1024);
        CHECK(ws_tier_keys(t) >= 2 * ws_tier_threads(t));       // every thread has a pair in every bitonic step of a full tier
    }
    CHECK(ws_tier_keys(WS_TIERS - 1) == WS_MAX_K && ws_tier_lds_bytes(WS_TIERS - 1) == 128 * 1024);   // of the CU's 160 KiB

    // offsets: no 32-bit overflow at the largest index, batch and k
    const long long n_pad = ws_padded_rows(0x7FFFFFFFll);
    CHECK(n_pad == 0x80000000ll);
    CHECK(ws_s_offset(WS_MAX_NQ - 1, n_pad) == (size_t)(WS_MAX_NQ - 1) * 0x80000000ull);
    CHECK(ws_s_offset(3, n_pad) == 0x180000000ull);
    CHECK(ws_c_offset(WS_MAX_NQ - 1, WS_MAX_K) == (size_t)(WS_MAX_NQ - 1) * 16384ull && ws_c_offset(WS_MAX_NQ - 1, WS_MAX_K) > 0xFFFFFFFFull);
    CHECK(ws_out_offset(WS_MAX_NQ - 1, WS_MAX_K, WS_MAX_K - 1) == (size_t)WS_MAX_NQ * 16384ull - 1);

    // the digits: disjoint, most significant first, all 32 bits, none wider than the histogram
    uint32_t all = 0u;
    int bits = 0;
    for (int p = 0; p < WS_PASSES; ++p) {
        const uint32_t m = ws_digit_mask(p);
        CHECK((all & m) == 0u && (1 << ws_digit_bits(p)) <= WS_BINS && (1 << ws_digit_bits(p)) % 64 == 0);
        CHECK(m == (((1ull << ws_digit_bits(p)) - 1ull) << ws_digit_shift(p)));
        if (p > 0) CHECK(ws_digit_shift(p) + ws_digit_bits(p) == ws_digit_shift(p - 1));
        all |= m;
        bits += ws_digit_bits(p);
    }
    CHECK(all == 0xFFFFFFFFu && bits == 32 && ws_digit_shift(0) + ws_digit_bits(0) == 32 && ws_digit_shift(WS_PASSES - 1) == 0);
    std::printf("wide select plan ok\n");
    return 0;
}
