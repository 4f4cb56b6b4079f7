// recommend_plan.hpp on the host, under ASan and UBSan (tests/test_recommend_cpu.py builds and runs this): the block against the
// byte budget, the cut of a batch into blocks of whole requests, the request table's parts, the combine's geometry and the layout
// at the largest index without 32-bit overflow.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "recommend_plan.hpp"

using namespace icd;

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            std::exit(1);                                                   \
        }                                                                   \
    } while (0)

int main() {
    static_assert(RC_SEG_ROWS == 1024 && RC_LANE_ROWS * 4 == 16 && RK_TILE % RC_LANE_ROWS == 0, "a lane's rows are one 16-byte word group inside a tile");
    // the block: within the budget, at most max_requests, the largest that fits; its example vectors cover 16 per request
    const long long ns[] = {1, 127, 128, 129, 1025, 40474, 1000000, 50000000, 0x7FFFFFFFll};
    const int ks[] = {1, 128, 1024, 16384};
    const long long reqs[] = {1, 2, 43, 1000, 16384, RC_MAX_REQUESTS};
    const int dims[] = {32, 768, 4096};
    for (long long n : ns)
        for (int k : ks)
            for (long long nr : reqs)
                for (int dim : dims)
                    for (long long me : {nr, nr * 3, nr * RC_MAX_EXAMPLES}) {
                        const long long b = rc_block_requests(nr, me, n, dim, k);
                        CHECK(b >= 0 && b <= nr);
                        CHECK((b == 0) == (rc_block_bytes(1, nr, me, n, dim, k) > WS_BLOCK_BUDGET));
                        if (b == 0) continue;
                        CHECK(rc_block_bytes(b, nr, me, n, dim, k) <= WS_BLOCK_BUDGET);
                        if (b < nr) CHECK(rc_block_bytes(b + 1, nr, me, n, dim, k) > WS_BLOCK_BUDGET);
                        if (b > 1) CHECK(rc_block_bytes(b - 1, nr, me, n, dim, k) <= rc_block_bytes(b, nr, me, n, dim, k));   // it grows with b
                        const RecommendLayout l = rc_layout(nr, me, k, n, dim);
                        CHECK(l.block == b && l.n_pad == ws_padded_rows(n) && l.block_examples == rc_examples_of(b, nr, me));
                        CHECK(l.block_examples >= (me < RC_MAX_EXAMPLES ? me : RC_MAX_EXAMPLES) && l.block_examples <= me && l.block_examples >= b);
                        CHECK(l.e_floats * 4 + l.se_words * 4 + l.s_words * 4 + l.c_keys * 8 + l.out_slots * 24 <= WS_BLOCK_BUDGET);
                        CHECK(l.bytes > l.se_words * 4 + l.s_words * 4 && l.v_floats == (size_t)me * dim && l.table == rc_table_words(nr, me));
                    }
    CHECK(rc_block_requests(1, 16, 0x7FFFFFFFll, 32, 1) == 0);       // 8 GiB of scores per run: refused at create
    // 40 474 x 768, k = 1 024, 16 examples a request: (40 576 x 4 + 1 024 x 32) + 16 x (768 x 4 + 40 576 x 4) bytes a request -> 94;
    // a workspace made for 5 examples a request holds 262 (section 28.7's probe), and never less than one request of 16
    CHECK(rc_block_requests(1000, 16000, 40474, 768, 1024) == 94);
    CHECK(rc_block_requests(1000, 5000, 40474, 768, 1024) == 262 && rc_examples_of(262, 1000, 5000) == 1310);
    CHECK(rc_examples_of(1, 1000, 5000) == 16 && rc_examples_of(1, 4, 10) == 10 && rc_examples_of(1000, 1000, 5000) == 5000);
    CHECK(rc_block_requests(1000, 16000, 40474, 768, 1024) == (long long)(WS_BLOCK_BUDGET / (rc_request_bytes(40474, 1024) + 16 * rc_example_bytes(40474, 768))));

    // the cut: whole requests, both limits, every request lands in exactly one block, never an empty block
    unsigned seed = 12345u;
    auto next = [&]() { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
    for (int round = 0; round < 200; ++round) {
        const long long nr = 1 + next() % 300;
        std::vector<int64_t> off(nr + 1, 0);
        for (long long r = 0; r < nr; ++r) off[r + 1] = off[r] + 1 + next() % RC_MAX_EXAMPLES;
        const long long br = 1 + next() % 64;
        const long long be = RC_MAX_EXAMPLES + next() % 200;
        long long r0 = 0, blocks = 0;
        while (r0 < nr) {
            const long long nb = rc_cut(off.data(), r0, nr, br, be);
            CHECK(nb >= 1 && nb <= br && r0 + nb <= nr);
            CHECK(off[r0 + nb] - off[r0] <= be);
            if (r0 + nb < nr && nb < br) CHECK(off[r0 + nb + 1] - off[r0] > be);   // the next request did not fit
            r0 += nb;
            ++blocks;
        }
        CHECK(r0 == nr && blocks >= (nr + br - 1) / br);
    }
    {   // 43 requests of 3 examples in blocks of 16 requests / 40 examples: 13 requests a block
        std::vector<int64_t> off(44);
        for (int r = 0; r <= 43; ++r) off[r] = 3 * r;
        CHECK(rc_cut(off.data(), 0, 43, 16, 40) == 13 && rc_cut(off.data(), 39, 43, 16, 40) == 4 && rc_cut(off.data(), 0, 43, 5, 40) == 5);
    }

    // the request table: three parts, back to back
    CHECK(rc_table_npos(7) == 8 && rc_table_rows(7) == 15 && rc_table_words(7, 20) == 35);
    CHECK(rc_table_words(RC_MAX_REQUESTS, RC_MAX_REQUESTS * RC_MAX_EXAMPLES) == (size_t)RC_MAX_REQUESTS * 18 + 1);
    CHECK(RC_MAX_REQUESTS * RC_MAX_EXAMPLES < 0x7FFFFFFFll);          // offsets and rows travel as int32

    // the combine's segments cover n padded; offsets at the largest index do not overflow 32 bits
    for (long long n : ns) {
        const long long n_pad = ws_padded_rows(n), segs = rc_segments(n_pad);
        CHECK(segs * RC_SEG_ROWS >= n_pad && (segs - 1) * RC_SEG_ROWS < n_pad && n_pad % RC_LANE_ROWS == 0);
    }
    CHECK(rc_segments(0x80000000ll) == 0x200000ll);
    CHECK(ws_s_offset(RC_MAX_EXAMPLES * 4 - 1, 0x80000000ll) == 63ull * 0x80000000ull);
    std::printf("recommend plan ok\n");
    return 0;
}
