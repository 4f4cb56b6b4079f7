// Checker for rag_project_icd10_amd/csrc/search_policy.hpp (built by tests/test_search_policy.py with g++): the adaptive
// rules of the AUTO search path, driven exactly like search_device drives them - take in the previous search's counters
// when they have arrived and the stream is not being captured, decide, note what this search was.
// Every expected value below is a literal read off the rules as search_device and icd_index_create stated them before
// they moved into the header (2048-query large batches, 4 f0 > n and 2 f2 < f0 to enter wide mode, 20 f0 <= n to leave it,
// every 64th wide search narrow; 4 clean searches of at most 24 flagged queries disarm the second pass; 96 clean searches
// disarm the streaming pair, doubling up to 65536; a second pass applies below 320 first-pass candidates per query) - none
// is computed from the header's own constants.
// `search_policy_check GROUP` runs one group (wide, pass2, sparse, capturing, reset, unplanned); no argument: all of them.
#include <cstdio>
#include <cstring>

#include "search_policy.hpp"

using namespace icd;

static int g_failed = 0, g_checks = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        ++g_checks;                                                             \
        if (!(cond)) { ++g_failed; printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); } \
    } while (0)

struct Knobs { bool adapt = true, pass2 = true; int chunks_override = 0; };
struct Search {
    long long nq = 10000; int k = 10;
    int cand = 5 * 16;         // candidates per query of the first pass (10 000 queries: 5 lists of 16)
    bool capturing = false;
    bool arrived = true;       // the previous search has completed: its counters are in host memory
};

// one AUTO search; `prev`: the counters the PREVIOUS search left. The second pass is planned (p2 > 0) when it is armed.
static SearchDecision search(SearchPolicy &p, const Knobs &kn, const Search &s, SearchCounters prev) {
    if (!s.capturing && s.arrived) policy_take_counters(p, prev);
    const SearchDecision d = policy_decide(p, kn.adapt, s.nq, s.k, kn.chunks_override);
    const int p2 = (kn.pass2 && p.pass2_armed()) ? 20 : 0;
    policy_note_search(p, kn.adapt, kn.pass2, s.nq, p2, d.wide_now, kn.chunks_override, s.cand);
    return d;
}

static bool same(const SearchPolicy &a, const SearchPolicy &b) {
    return a.wide_mode == b.wide_mode && a.wide_runs == b.wide_runs && a.last_narrow_large == b.last_narrow_large &&
           a.last_narrow_nq == b.last_narrow_nq && a.p2_clean == b.p2_clean && a.p2_eval_pending == b.p2_eval_pending &&
           a.sparse_need == b.sparse_need && a.sparse_run_seen == b.sparse_run_seen && a.sparse_disarmed == b.sparse_disarmed;
}

// does a large narrow batch of n queries that left (f0, f2) put a fresh index into wide mode?
static bool enters(long long n, int f0, int f2) {
    SearchPolicy p; Knobs kn; Search s; s.nq = n;
    search(p, kn, s, {0, 0, 0});
    search(p, kn, s, {f0, f2, 0});
    return p.wide_mode;
}

static void group_wide() {
    // entered iff 4 f0 > n and 2 f2 < f0
    CHECK(enters(10000, 2501, 1250));
    CHECK(!enters(10000, 2500, 0));       // 4 f0 == n
    CHECK(!enters(10000, 2501, 1251));    // 2 f2 > f0
    CHECK(!enters(10000, 2502, 1251));    // 2 f2 == f0
    CHECK(enters(2048, 513, 0));
    CHECK(!enters(2048, 512, 0));
    {   // a batch below 2048 queries is not "large": its counters are never judged
        SearchPolicy p; Knobs kn; Search s; s.nq = 2047;
        search(p, kn, s, {0, 0, 0});
        CHECK(!p.last_narrow_large);
        search(p, kn, s, {2047, 0, 0});
        CHECK(!p.wide_mode);
    }
    {   // judged against the size of the batch the counters belong to, not the current one
        SearchPolicy p; Knobs kn; Search big, small; big.nq = 10000; small.nq = 2048;
        search(p, kn, big, {0, 0, 0});
        search(p, kn, small, {600, 0, 0});     // 4 * 600 > 2048 but not > 10 000
        CHECK(!p.wide_mode);
        search(p, kn, big, {600, 0, 0});       // ... these belong to the 2048-query batch
        CHECK(p.wide_mode);
    }
    {   // in wide mode: large searches plan wide, every 64th narrow; the narrow one's counters decide anew (left iff 20 f0 <= n)
        SearchPolicy p; Knobs kn; Search s;
        search(p, kn, s, {0, 0, 0});
        SearchDecision d = search(p, kn, s, {5000, 100, 0});
        CHECK(p.wide_mode && d.wide_now && p.wide_runs == 1);
        int narrow_at = -1;
        for (int i = 2; i <= 64; ++i) {
            d = search(p, kn, s, {9999, 9999, 0});   // (counters of wide searches are not judged)
            CHECK(p.wide_mode);
            if (!d.wide_now && narrow_at < 0) narrow_at = i;
        }
        CHECK(narrow_at == 64);
        CHECK(p.last_narrow_large && p.last_narrow_nq == 10000);
        SearchPolicy q = p;
        search(q, kn, s, {501, 0, 0});         // 20 * 501 > 10 000: stays
        CHECK(q.wide_mode);
        q = p;
        d = search(q, kn, s, {500, 0, 0});     // 20 * 500 <= 10 000: left
        CHECK(!q.wide_mode && !d.wide_now);
        q = p;
        d = search(q, kn, s, {501, 0, 0});
        CHECK(d.wide_now && q.wide_runs == 65);   // (the count goes on: the next narrow search is the 128th)
    }
    {   // small batches in wide mode neither plan wide nor count
        SearchPolicy p; p.wide_mode = true; Knobs kn; Search s; s.nq = 2047;
        CHECK(!search(p, kn, s, {0, 0, 0}).wide_now && p.wide_runs == 0);
    }
    {   // chunks_override != 0 or k > 32 never plans wide (and does not count)
        SearchPolicy p; p.wide_mode = true; Knobs kn; Search s;
        kn.chunks_override = 8;
        CHECK(!search(p, kn, s, {0, 0, 0}).wide_now && p.wide_runs == 0);
        CHECK(!p.last_narrow_large);           // (... and an overridden plan is not a probe of the corpus)
        kn.chunks_override = 0; s.k = 33;
        CHECK(!search(p, kn, s, {0, 0, 0}).wide_now && p.wide_runs == 0);
        CHECK(p.last_narrow_large);            // OBSERVATION: a k > 32 batch in wide mode is noted as a narrow probe all the same
        s.k = 32;
        CHECK(search(p, kn, s, {5000, 0, 0}).wide_now);
    }
    {   // adapt_enabled = false: no batch is noted, wide mode is never entered
        SearchPolicy p; Knobs kn; kn.adapt = false; Search s;
        search(p, kn, s, {0, 0, 0});
        CHECK(!p.last_narrow_large);
        search(p, kn, s, {9000, 0, 0});
        CHECK(!p.wide_mode);
    }
    {   // a search without a second pass behind it (disarmed) is not a probe
        SearchPolicy p; p.p2_clean = 4; Knobs kn; Search s;
        search(p, kn, s, {0, 0, 0});
        CHECK(!p.last_narrow_large);
    }
}

static void group_pass2() {
    SearchPolicy p; Knobs kn; Search s;
    CHECK(p.pass2_armed());
    search(p, kn, s, {0, 0, 0});               // the first search: nothing pending, nothing evaluated
    CHECK(p.p2_clean == 0 && p.p2_eval_pending);
    for (int i = 1; i <= 3; ++i) { search(p, kn, s, {24, 0, 0}); CHECK(p.p2_clean == i && p.pass2_armed()); }
    {   // a search whose counters have not arrived changes nothing
        SearchPolicy q = p; Search late = s; late.arrived = false;
        search(q, kn, late, {0, 0, 0});
        CHECK(q.p2_clean == 3 && q.p2_eval_pending && q.pass2_armed());
    }
    search(p, kn, s, {24, 0, 0});              // the 4th consecutive one with f0 <= 24
    CHECK(p.p2_clean == 4 && !p.pass2_armed());
    search(p, kn, s, {0, 0, 0});
    CHECK(p.p2_clean == 5 && !p.pass2_armed());
    search(p, kn, s, {25, 0, 0});              // one with more re-arms
    CHECK(p.p2_clean == 0 && p.pass2_armed());
    {   // a search the second pass does not apply to (pc * kp >= 320) is not evaluated
        SearchPolicy q; Search mid = s; mid.nq = 1000; mid.cand = 320;
        search(q, kn, mid, {0, 0, 0});
        CHECK(!q.p2_eval_pending);
        search(q, kn, mid, {0, 0, 0});
        CHECK(q.p2_clean == 0);
        mid.cand = 319;
        search(q, kn, mid, {0, 0, 0});
        CHECK(q.p2_eval_pending);
        search(q, kn, mid, {0, 0, 0});
        CHECK(q.p2_clean == 1);
    }
    {   // pass2_enabled = false: never evaluated
        SearchPolicy q; Knobs off; off.pass2 = false;
        search(q, off, s, {0, 0, 0}); search(q, off, s, {0, 0, 0});
        CHECK(!q.p2_eval_pending && q.p2_clean == 0);
    }
    {   // icd_index_set_second_pass re-arms
        SearchPolicy q = p; q.p2_clean = 7; q.p2_eval_pending = true; q.wide_mode = true; q.sparse_need = 384; q.sparse_run_seen = 500; q.sparse_disarmed = true;
        SearchPolicy r = q;
        q.rearm(true);
        CHECK(q.p2_clean == 0 && !q.p2_eval_pending && q.wide_mode && q.sparse_need == 96 && q.sparse_run_seen == 0 && !q.sparse_disarmed);
        r.last_narrow_large = true;
        r.rearm(false);
        CHECK(!r.wide_mode && !r.last_narrow_large && r.p2_clean == 0);
    }
}

static void group_sparse() {
    SearchPolicy p; Knobs kn; Search s;
    CHECK(p.sparse_need == 96);
    CHECK(!search(p, kn, s, {0, 0, 95}).sparse_off && !p.sparse_disarmed);
    CHECK(search(p, kn, s, {0, 0, 96}).sparse_off && p.sparse_disarmed);       // the device's clean run reaches sparse_need
    CHECK(search(p, kn, s, {0, 0, 97}).sparse_off && p.sparse_need == 96);
    // an incident while disarmed (the run restarted on the device) doubles the requirement
    CHECK(!search(p, kn, s, {3, 0, 0}).sparse_off && p.sparse_need == 192 && !p.sparse_disarmed);
    CHECK(!search(p, kn, s, {0, 0, 1}).sparse_off && p.sparse_need == 192);    // (armed: a short run is no incident)
    CHECK(!search(p, kn, s, {0, 0, 191}).sparse_off);
    CHECK(search(p, kn, s, {0, 0, 192}).sparse_off);
    CHECK(!search(p, kn, s, {0, 0, 5}).sparse_off && p.sparse_need == 384);
    {   // ... up to 1 << 16
        SearchPolicy q; q.sparse_need = 40000; q.sparse_disarmed = true;
        search(q, kn, s, {0, 0, 0});
        CHECK(q.sparse_need == 65536);
        q.sparse_disarmed = true;
        search(q, kn, s, {0, 0, 0});
        CHECK(q.sparse_need == 65536);
    }
    {   // counters that have not arrived: the last run length seen decides
        SearchPolicy q; Search late = s; late.arrived = false;
        CHECK(!search(q, kn, late, {0, 0, 500}).sparse_off && q.sparse_run_seen == 0);
        CHECK(search(q, kn, s, {0, 0, 500}).sparse_off);
        CHECK(search(q, kn, late, {0, 0, 0}).sparse_off && q.sparse_need == 96);
    }
    {   // adapt_enabled = false never disarms
        SearchPolicy q; Knobs off; off.adapt = false;
        CHECK(!search(q, off, s, {0, 0, 100000}).sparse_off && !q.sparse_disarmed && q.sparse_need == 96);
    }
}

static void group_capturing() {
    // while a search is captured into a HIP graph nothing is read: whatever the pinned counters hold, what is decided from
    // them stays as it is
    SearchPolicy p; Knobs kn; Search s;
    search(p, kn, s, {0, 0, 0});
    search(p, kn, s, {10, 0, 50});
    const SearchPolicy before = p;
    Search cap = s; cap.capturing = true;
    const SearchDecision d = search(p, kn, cap, {9000, 0, 100000});
    CHECK(!d.sparse_off && !d.wide_now);
    CHECK(same(p, before));
    {   // OBSERVATION: the captured search is still decided and noted like any other - in wide mode it advances wide_runs, and
        // it leaves p2_eval_pending / last_narrow_large for the counters of whichever search completes next
        SearchPolicy q; q.wide_mode = true;
        CHECK(search(q, kn, cap, {0, 0, 0}).wide_now && q.wide_runs == 1 && q.p2_eval_pending);
        SearchPolicy r;
        search(r, kn, cap, {0, 0, 0});
        CHECK(r.last_narrow_large && r.last_narrow_nq == 10000 && r.p2_eval_pending);
    }
}

static void group_reset() {
    // the corpus-shape probe of icd_index_create: ONE 2048-query search on a fresh index, its counters taken in, reset()
    for (int family = 0; family < 2; ++family) {
        SearchPolicy p; Knobs kn; Search s; s.nq = 2048;
        search(p, kn, s, {0, 0, 0});
        CHECK(p.last_narrow_large && p.last_narrow_nq == 2048);
        policy_take_counters(p, family ? SearchCounters{1500, 40, 0} : SearchCounters{0, 0, 1});
        p.reset();
        SearchPolicy fresh;
        fresh.wide_mode = family != 0;         // 4 * 1500 > 2048 and 2 * 40 < 1500
        CHECK(same(p, fresh));
        CHECK(p.sparse_need == 96 && p.pass2_armed());
    }
}

// a search that does not go through the plan (MODE_EXACT, a one-query call): search_device hands over the counters the last
// planned search left if they have arrived; the unplanned search then leaves f0 = 0 behind itself
static void unplanned(SearchPolicy &p, bool arrived, SearchCounters left) { policy_unplanned_search(p, arrived ? &left : nullptr); }

static void group_unplanned() {
    Knobs kn; Search s; s.nq = 2048; s.cand = 14 * 16;
    {   // narrow large batch, MODE_EXACT, large batch: the narrow batch's own counters decide, not the zeros behind the exact search
        SearchPolicy p;
        search(p, kn, s, {0, 0, 0});
        CHECK(p.last_narrow_large && p.p2_eval_pending);
        unplanned(p, true, {2000, 0, 0});
        CHECK(p.wide_mode && p.wide_runs == 0 && !p.last_narrow_large && !p.p2_eval_pending && p.p2_clean == 0);
        CHECK(search(p, kn, s, {0, 0, 0}).wide_now && p.wide_mode);
    }
    {   // the narrow re-probe of a family corpus, then MODE_EXACT: wide mode stays (it left: 20 * 0 <= n)
        SearchPolicy p; p.wide_mode = true; p.wide_runs = 63;
        CHECK(!search(p, kn, s, {0, 0, 0}).wide_now && p.last_narrow_large);
        unplanned(p, true, {2000, 0, 0});
        CHECK(p.wide_mode);
        CHECK(search(p, kn, s, {0, 0, 0}).wide_now && p.wide_mode && p.wide_runs == 65);
    }
    {   // ... and a re-probe that certified 95 % leaves it, judged at the unplanned search
        SearchPolicy p; p.wide_mode = true; p.wide_runs = 63;
        search(p, kn, s, {0, 0, 0});
        unplanned(p, true, {102, 0, 0});       // 20 * 102 <= 2048
        CHECK(!p.wide_mode);
    }
    {   // counters that have not arrived (or a capture): both verdicts are dropped, the zeros are never judged
        SearchPolicy p; p.wide_mode = true; p.wide_runs = 63;
        search(p, kn, s, {0, 0, 0});
        unplanned(p, false, {0, 0, 0});
        CHECK(p.wide_mode && !p.last_narrow_large && !p.p2_eval_pending);
        CHECK(search(p, kn, s, {0, 0, 0}).wide_now && p.wide_mode && p.p2_clean == 0);
    }
    {   // the second pass's clean count: a batch that flagged 25 is not clean because an exact search followed it
        SearchPolicy p; p.p2_clean = 3;
        search(p, kn, s, {0, 0, 0});           // (nothing pending before it)
        CHECK(p.p2_clean == 3);
        unplanned(p, true, {25, 0, 0});
        CHECK(p.p2_clean == 0);
        search(p, kn, s, {0, 0, 0});           // the exact search's zeros: nothing pending, nothing counted
        CHECK(p.p2_clean == 0 && p.pass2_armed());
    }
    {   // the streaming pair's run length is not taken in here (the next planned search does, once)
        SearchPolicy p; p.sparse_disarmed = true;
        search(p, kn, s, {0, 0, 96});
        const int need = p.sparse_need, seen = p.sparse_run_seen;
        unplanned(p, true, {0, 0, 0});
        CHECK(p.sparse_need == need && p.sparse_run_seen == seen);
    }
    {   // nothing pending: nothing changes
        SearchPolicy p; p.wide_mode = true; p.wide_runs = 5; p.p2_clean = 2;
        const SearchPolicy before = p;
        unplanned(p, true, {0, 0, 0});
        CHECK(same(p, before));
    }
}

int main(int argc, char **argv) {
    const char *only = argc > 1 ? argv[1] : nullptr;
    struct { const char *name; void (*run)(); } groups[] = {
        {"wide", group_wide}, {"pass2", group_pass2}, {"sparse", group_sparse}, {"capturing", group_capturing}, {"reset", group_reset},
        {"unplanned", group_unplanned}};
    int ran = 0;
    for (auto &g : groups)
        if (!only || !strcmp(only, g.name)) { g.run(); ++ran; }
    if (!ran) { printf("unknown group %s\n", only); return 2; }
    if (g_failed) { printf("%d of %d checks FAILED\n", g_failed, g_checks); return 1; }
    printf("%d checks ok\n", g_checks);
    return 0;
}
