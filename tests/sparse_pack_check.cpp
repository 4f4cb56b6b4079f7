// Checker for rag_project_icd10_amd/csrc/sparse_pack.hpp (host only; built by tests/test_sparse_cpu.py with g++, there also with
// -fsanitize=address,undefined). Packs random CSR rows and compares with a per-term scan of the rows; walks the refusals and
// checks that a refused input writes nothing.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "sparse_pack.hpp"

using namespace icd;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 32);
}

struct Csr {
    std::vector<int64_t> off;
    std::vector<uint32_t> terms;
    std::vector<float> vals;
};

static Csr random_rows(int64_t n, int64_t vocab, int density_pct) {
    Csr c;
    c.off.push_back(0);
    for (int64_t i = 0; i < n; ++i) {
        for (int64_t t = 0; t < vocab; ++t)
            if ((int)(rnd() % 100) < density_pct) {
                c.terms.push_back((uint32_t)t);
                c.vals.push_back((float)(rnd() % 2000 + 1) / 64.0f * ((rnd() & 1) ? 1.0f : -1.0f));
            }
        c.off.push_back((int64_t)c.terms.size());
    }
    return c;
}

static int fails = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++fails; } } while (0)

static void check_pack(int64_t n, int64_t vocab, int density_pct) {
    const Csr c = random_rows(n, vocab, density_pct);
    const size_t nnz = c.terms.size();
    std::vector<int64_t> post_off((size_t)vocab + 1, -7);
    std::vector<uint32_t> post_row(nnz + 1, 0xDEADu);
    std::vector<float> post_val(nnz + 1, -1.0f);
    char msg[200] = "";
    const int rc = sparse_pack_rows(c.off.data(), c.terms.data(), c.vals.data(), n, vocab, post_off.data(), post_row.data(), post_val.data(), msg, sizeof msg);
    EXPECT(rc == SPARSE_OK);
    EXPECT(post_off[0] == 0 && post_off[(size_t)vocab] == (int64_t)nnz);
    EXPECT(post_row[nnz] == 0xDEADu && post_val[nnz] == -1.0f);   // nothing behind the end
    size_t at = 0;
    for (int64_t t = 0; t < vocab; ++t) {
        EXPECT(post_off[(size_t)t] == (int64_t)at);
        for (int64_t i = 0; i < n; ++i)
            for (int64_t p = c.off[(size_t)i]; p < c.off[(size_t)i + 1]; ++p)
                if (c.terms[(size_t)p] == (uint32_t)t) {
                    EXPECT(at < nnz && post_row[at] == (uint32_t)i && post_val[at] == c.vals[(size_t)p]);
                    ++at;
                }
    }
    EXPECT(at == nnz);
}

static void check_refusals() {
    const int64_t off[] = {0, 2, 2, 3};
    const uint32_t terms[] = {1, 4, 0};
    const float vals[] = {1.0f, -2.0f, 0.5f};
    int64_t post_off[6];
    uint32_t post_row[3];
    float post_val[3];
    char msg[200];
    auto pack = [&](const int64_t *o, const uint32_t *t, const float *v, int64_t n, int64_t vocab) {
        for (auto &x : post_off) x = -7;
        const int rc = sparse_pack_rows(o, t, v, n, vocab, post_off, post_row, post_val, msg, sizeof msg);
        if (rc != SPARSE_OK) for (auto x : post_off) EXPECT(x == -7);   // a refused input writes nothing
        return rc;
    };
    EXPECT(pack(off, terms, vals, 3, 5) == SPARSE_OK);
    EXPECT(post_off[0] == 0 && post_off[1] == 1 && post_off[2] == 2 && post_off[4] == 2 && post_off[5] == 3);
    EXPECT(post_row[0] == 2 && post_row[1] == 0 && post_row[2] == 0 && post_val[2] == -2.0f);
    EXPECT(pack(off, terms, vals, 3, 4) == SPARSE_BAD);          // term 4 >= vocab
    EXPECT(pack(off, terms, vals, 0, 5) == SPARSE_BAD);          // no rows
    EXPECT(pack(nullptr, terms, vals, 3, 5) == SPARSE_BAD);
    EXPECT(pack(off, nullptr, vals, 3, 5) == SPARSE_BAD);
    EXPECT(pack(off, terms, vals, 3, 0) == SPARSE_BAD);
    const uint32_t dup[] = {1, 1, 0}, unsorted[] = {4, 1, 0};
    EXPECT(pack(off, dup, vals, 3, 5) == SPARSE_BAD);
    EXPECT(pack(off, unsorted, vals, 3, 5) == SPARSE_BAD);
    const float zero[] = {1.0f, 0.0f, 0.5f}, nan_[] = {1.0f, NAN, 0.5f}, inf_[] = {std::numeric_limits<float>::infinity(), 1.0f, 0.5f};
    EXPECT(pack(off, terms, zero, 3, 5) == SPARSE_BAD);
    EXPECT(pack(off, terms, nan_, 3, 5) == SPARSE_BAD);
    EXPECT(pack(off, terms, inf_, 3, 5) == SPARSE_BAD);
    const int64_t back[] = {0, 2, 1, 3}, late[] = {1, 2, 2, 3};
    EXPECT(pack(back, terms, vals, 3, 5) == SPARSE_BAD);
    EXPECT(pack(late, terms, vals, 3, 5) == SPARSE_BAD);
    // a query's rules: the same, and a length limit
    EXPECT(sparse_check_csr(off, terms, vals, 3, 5, 2, "query", msg, sizeof msg) == SPARSE_OK);
    EXPECT(sparse_check_csr(off, terms, vals, 3, 5, 1, "query", msg, sizeof msg) == SPARSE_BAD);
    const int64_t none[] = {0, 0};
    EXPECT(sparse_check_csr(none, nullptr, nullptr, 1, 5, 64, "query", msg, sizeof msg) == SPARSE_OK);
}

int main() {
    check_refusals();
    const int64_t shapes[][3] = {{1, 1, 100}, {1, 7, 0}, {5, 1, 50}, {33, 37, 10}, {200, 64, 3}, {257, 300, 1}, {64, 5, 100}};
    for (const auto &s : shapes) check_pack(s[0], s[1], (int)s[2]);
    if (fails) { printf("%d checks failed\n", fails); return 1; }
    printf("sparse pack cases ok\n");
    return 0;
}
