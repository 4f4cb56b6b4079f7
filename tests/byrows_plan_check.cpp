// byrows_plan_check.cpp - host check of rag_project_icd10_amd/csrc/byrows_plan.hpp, built with
// -fsanitize=address,undefined and run by tests/test_byrows_cpu.py. It replays the drop step of byrows_drop_self_kernel with the
// header's own functions - lane by lane, two entries per lane, on heap buffers of EXACTLY the sizes the kernel may touch, so an
// index one past either list is a sanitizer report - against a plain erase-and-sort over every k, every gap position, short
// lists with padding, all-tied scores, and ids at the edges of the index.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "byrows_plan.hpp"

using namespace icd;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

struct Entry {
    float raw;
    long long id;
    int lv;
};
static double weight(int lv) { return lv == 1 ? 1.2 : (lv == 3 ? 0.8 : 1.0); }

// the kernel's walk over one query: staged list of `len` slots -> `keep` outputs
static void kernel_walk(const std::vector<Entry> &list, int keep, long long self, bool reweighted, std::vector<Entry> &out, std::vector<double> &out_adj) {
    const int len = (int)list.size();
    int first = BR_MAX_LIST;
    for (int e = BR_PER_LANE - 1; e >= 0; --e) {   // the ballots: the lowest lane of the lowest half wins
        int lowest = -1;
        for (int lane = BR_WAVE - 1; lane >= 0; --lane) {
            const int j = lane + BR_WAVE * e;
            if (len > keep && j < len && list[(size_t)j].id == self) lowest = lane;
        }
        if (lowest >= 0) first = BR_WAVE * e + lowest;
    }
    const int gap = br_gap(first, len, keep);
    std::vector<Entry> got((size_t)keep);
    std::vector<double> adj((size_t)BR_MAX_LIST, -std::numeric_limits<double>::infinity());
    for (int j = 0; j < keep; ++j) {
        Entry v{-std::numeric_limits<float>::infinity(), -1, 0};
        const Entry &s = list.at((size_t)br_source(j, gap));   // (.at: a source past the list throws)
        if (s.id >= 0) v = s;
        got[(size_t)j] = v;
        adj[(size_t)j] = v.id >= 0 ? (double)v.raw * weight(v.lv) : -std::numeric_limits<double>::infinity();
    }
    out.assign((size_t)keep, Entry{0, 0, 0});
    out_adj.assign((size_t)keep, 0.0);
    std::vector<int> written((size_t)keep, 0);
    for (int j = 0; j < keep; ++j) {
        const int w = reweighted ? br_stable_rank(adj.data(), keep, j) : j;
        CHECK(w >= 0 && w < keep);
        if (w < 0 || w >= keep) continue;
        out[(size_t)w] = got[(size_t)j];
        out_adj[(size_t)w] = adj[(size_t)j];
        ++written[(size_t)w];
    }
    for (int j = 0; j < keep; ++j) CHECK(written[(size_t)j] == 1);   // a permutation: every slot written once
}

// the contract: erase self (or the last entry), then one stable descending sort of the adjusted scores
static void plain(const std::vector<Entry> &list, int keep, long long self, bool reweighted, std::vector<Entry> &out, std::vector<double> &out_adj) {
    std::vector<Entry> l = list;
    if ((int)l.size() > keep) {
        size_t at = l.size() - 1;
        for (size_t j = 0; j < l.size(); ++j)
            if (l[j].id == self) { at = j; break; }
        l.erase(l.begin() + (long)at);
    }
    for (Entry &e : l)
        if (e.id < 0) e = Entry{-std::numeric_limits<float>::infinity(), -1, 0};
    std::vector<int> order(l.size());
    for (size_t j = 0; j < l.size(); ++j) order[j] = (int)j;
    auto adj_of = [&](int j) { return l[(size_t)j].id >= 0 ? (double)l[(size_t)j].raw * weight(l[(size_t)j].lv) : -std::numeric_limits<double>::infinity(); };
    if (reweighted) std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return adj_of(a) > adj_of(b); });
    out.clear();
    out_adj.clear();
    for (int j : order) { out.push_back(l[(size_t)j]); out_adj.push_back(adj_of(j)); }
}

static void compare(const std::vector<Entry> &list, int keep, long long self) {
    for (int rw = 0; rw < 2; ++rw) {
        std::vector<Entry> a, b;
        std::vector<double> aa, ba;
        kernel_walk(list, keep, self, rw != 0, a, aa);
        plain(list, keep, self, rw != 0, b, ba);
        CHECK(a.size() == b.size() && a.size() == (size_t)keep);
        for (size_t j = 0; j < a.size() && j < b.size(); ++j) {
            CHECK(a[j].id == b[j].id && a[j].lv == b[j].lv);
            CHECK(a[j].raw == b[j].raw || (a[j].raw != a[j].raw && b[j].raw != b[j].raw));
            CHECK(aa[j] == ba[j]);
        }
    }
}

int main() {
    // geometry and layout
    CHECK(BR_MAX_K == 127 && BR_PER_LANE == 2 && BR_THREADS == 256);
    CHECK(br_blocks(0) == 0 && br_blocks(1) == 1 && br_blocks(4) == 1 && br_blocks(5) == 2 && br_blocks(300) == 75);
    {
        const ByRowsLayout l = br_layout(300, 768);
        CHECK(l.q_floats == (size_t)300 * 768 && l.list_slots == (size_t)300 * 128 && l.out_slots == l.list_slots && l.per_query == 300);
        CHECK(l.bytes == l.q_floats * 4 + l.list_slots * 16 + l.out_slots * 24 + l.per_query * 12);
        const ByRowsLayout big = br_layout(0x7FFFFFFFll / 128, 4096);   // the largest workspace icd_byrows_create accepts: no 32-bit wrap
        CHECK(big.q_floats == (size_t)(0x7FFFFFFFll / 128) * 4096 && big.bytes > big.q_floats * 4);
    }
    // ids -> rows: the edges of the index, a non-zero base, and ids whose distance from the base does not fit a signed 64
    CHECK(br_row_of(0, 0, 1) == 0 && br_row_of(1, 0, 1) == -1 && br_row_of(-1, 0, 1) == -1);
    CHECK(br_row_of(5000000000ll, 5000000000ll, 129) == 0 && br_row_of(5000000128ll, 5000000000ll, 129) == 128);
    CHECK(br_row_of(5000000129ll, 5000000000ll, 129) == -1 && br_row_of(4999999999ll, 5000000000ll, 129) == -1);
    CHECK(br_row_of(std::numeric_limits<long long>::min(), 5, 100) == -1 && br_row_of(std::numeric_limits<long long>::max(), -5, 100) == -1);
    CHECK(br_row_of(std::numeric_limits<long long>::max(), std::numeric_limits<long long>::max() - 3, 100) == 3);
    // the gap and the source slot, every k and every position
    for (int k = 1; k <= BR_MAX_K; ++k) {
        const int len = k + 1;
        for (int p = 0; p <= len + 2; ++p) {
            const int gap = br_gap(p, len, k);
            CHECK(gap == (p < len ? p : k));
            for (int j = 0; j < k; ++j) {
                const int s = br_source(j, gap);
                CHECK(s >= 0 && s < len && s != gap && (j == 0 || s > br_source(j - 1, gap)));
            }
        }
        CHECK(br_gap(BR_MAX_LIST, k, k) == k);   // include_self: the list is k wide and nothing moves
        for (int j = 0; j < k; ++j) CHECK(br_source(j, k) == j);
    }
    // whole lists: self first, in the middle, last, absent; short lists with padding; all tied; repeated for every k
    std::srand(7);
    for (int k = 1; k <= BR_MAX_K; ++k) {
        for (int trial = 0; trial < 12; ++trial) {
            const int len = k + 1;
            const int hits = trial % 4 == 3 ? std::rand() % (len + 1) : len;   // a short list: padding behind the hits
            std::vector<Entry> list((size_t)len, Entry{-std::numeric_limits<float>::infinity(), -1, 0});
            const bool tied = trial % 3 == 2;
            float s = 1.0f;
            for (int j = 0; j < hits; ++j) {
                if (!tied && std::rand() % 3) s -= 0.015625f * (float)(std::rand() % 3);
                list[(size_t)j] = Entry{s, 1000 + 3 * j, 1 + std::rand() % 3};
            }
            const long long selfs[4] = {1000, 1000 + 3 * (hits / 2), 1000 + 3 * (hits - 1), 7};   // first, middle, last, absent
            for (long long self : selfs) compare(list, k, self);
            std::vector<Entry> same(list.begin(), list.begin() + k);
            compare(same, k, 1000);   // include_self: len = keep, the id is in the list and stays
        }
    }
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("byrows plan ok\n");
    return 0;
}
