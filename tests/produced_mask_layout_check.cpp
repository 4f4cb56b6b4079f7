// Checker for rag_project_icd10_amd/csrc/produced_mask_layout.hpp (host only; built by tests/test_filter_device_cpu.py with g++ and
// -fsanitize=address,undefined). For every (nq, n, base table or none, staged-region sizes) of the lists below: the regions are
// aligned, disjoint, in order and end at the total; the cleared span is exactly bitsets + counters. Every region is then written
// with a tag of its own, as far as its elements reach, in a heap block of exactly `total` bytes (a write past the end is an ASan
// report) and read back (an overlap changes a tag).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "produced_mask_layout.hpp"

static int fails = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("FAILED line %d: %s (nq=%lld n=%lld base=%d)\n", __LINE__, #cond, (long long)nq, (long long)n, (int)any_base); ++fails; } } while (0)

struct Region { size_t at, bytes, align; };

static void check(int64_t nq, int64_t n, bool any_base, const size_t *staged, int n_staged) {
    const ProducedMaskLayout l = produced_mask_layout(nq, n, any_base, staged, n_staged);
    EXPECT(l.words == (size_t)((n + 127) / 128 * 4 + 4));   // whole 128-row tiles of 4 words, 4 tail words
    EXPECT(l.words * 32 >= (size_t)n + 128 && l.words % 4 == 0);
    for (int64_t q = 0; q < nq; ++q) EXPECT((l.bits + (size_t)q * l.words * 4) % 16 == 0);

    std::vector<Region> r;   // in the order the block holds them; what each NEEDS, not what it was given
    r.push_back({l.bits, (size_t)nq * l.words * 4, 16});
    r.push_back({l.counters, (size_t)nq * 4, 4});
    r.push_back({l.base, any_base ? (size_t)nq * 8 : 0, 8});
    for (int i = 0; i < n_staged; ++i) r.push_back({l.staged[i], staged[i], 16});
    EXPECT(r[0].at == 0);
    for (size_t i = 0; i < r.size(); ++i) {
        EXPECT(r[i].at % r[i].align == 0);
        EXPECT(r[i].at % 16 == 0);   // (what the header promises for every region)
        const size_t next = i + 1 < r.size() ? r[i + 1].at : l.total;
        EXPECT(r[i].at + r[i].bytes <= next);        // disjoint and in order
        EXPECT(next - (r[i].at + r[i].bytes) < 16);  // nothing but padding between two regions
    }
    EXPECT(l.total == (r.back().at + r.back().bytes + 15) / 16 * 16);   // the total is the (padded) end of the last region
    // the cleared span: from the start, all of bitsets and counters, nothing of what follows
    EXPECT(l.zeroed >= l.counters + (size_t)nq * 4 && l.zeroed == r[2].at && l.zeroed <= l.total);

    unsigned char *block = new unsigned char[l.total];
    memset(block, 0xEE, l.total);
    for (size_t i = 0; i < r.size(); ++i) memset(block + r[i].at, (int)(i + 1), r[i].bytes);
    for (size_t i = 0; i < r.size(); ++i)
        for (size_t b = 0; b < r[i].bytes; b += (r[i].bytes > 64 ? r[i].bytes - 1 : 1)) EXPECT(block[r[i].at + b] == (unsigned char)(i + 1));
    delete[] block;
}

int main() {
    const int64_t nqs[] = {1, 2, 3, 5, 300};
    const int64_t ns[] = {1, 31, 32, 33, 127, 128, 129, 8191, 8192, 8193, 16389};
    long cases = 0;
    for (int64_t nq : nqs)
        for (int64_t n : ns)
            for (int any_base = 0; any_base < 2; ++any_base) {
                const size_t sizes[4] = {0, 4, 12, 8 * ((size_t)nq + 1)};
                for (int n_staged = 0; n_staged <= PM_MAX_STAGED; ++n_staged) {
                    int combos = 1;
                    for (int i = 0; i < n_staged; ++i) combos *= 4;
                    for (int c = 0; c < combos; ++c) {
                        size_t staged[PM_MAX_STAGED] = {0, 0, 0};
                        for (int i = 0, d = c; i < n_staged; ++i, d /= 4) staged[i] = sizes[d % 4];
                        check(nq, n, any_base != 0, staged, n_staged);
                        ++cases;
                    }
                }
            }
    if (fails) { printf("%d checks FAILED\n", fails); return 1; }
    printf("%ld produced-mask layouts ok\n", cases);
    return 0;
}
