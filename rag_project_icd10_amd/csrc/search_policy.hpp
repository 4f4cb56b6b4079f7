// search_policy.hpp — the adaptive rules of the AUTO search path as plain C++ (no HIP types): what an index remembers between
// searches and how the counters of the PREVIOUS search change the plan of the next one. Shared by search_device, the
// corpus-shape probe of icd_index_create and tests/search_policy_check.cpp (built with g++ by tests/test_search_policy.py).
// Performance decisions only: a search returns the exact top-k whatever this state holds.
#pragma once
#include <algorithm>

#include "flat_partition.hpp"   // PASS2_BELOW

namespace icd {

constexpr int PASS2_SKIP = 24;       // ... and leaves this many flagged queries (or fewer) to the streaming kernel: 35 us per 8
constexpr int SPARSE_DISARM_AFTER = 96; // the streaming kernel's two fallback launches are dropped after this many consecutive searches with NO flagged query (doubles at every incident)
constexpr int SPARSE_NEED_MAX = 1 << 16;
constexpr int PASS2_DISARM_AFTER = 4; // the second pass's two launches are dropped after this many consecutive searches that needed neither
constexpr int WIDE_MIN_NQ = 2048;    // "large batch": below it a query has 16+ lists anyway
constexpr int WIDE_REPROBE = 64;

// The counters every search leaves in pinned host memory behind its last kernel (icd_index::h_nflag): queries flagged by the
// first finalize [0], after its wide-window retry [1], after the second coarse pass [2], and [4] the consecutive fast-path
// searches whose exact re-search had nothing to do (kept by the device, so searches the host never looked at count too).
struct SearchCounters { int f0, f2, clean_run; };
inline SearchCounters search_counters(const int *h_nflag) { return SearchCounters{h_nflag[0], h_nflag[2], h_nflag[4]}; }

struct SearchPolicy {
    // adaptive list count of LARGE batches (>= WIDE_MIN_NQ queries): when the second coarse pass had to rescue most of the
    // previous large batch (a corpus of tight families), the first pass is planned with its list count right away
    bool wide_mode = false;        // plan the first pass with PASS2_CHUNKS lists per query
    int wide_runs = 0;             // large searches since wide_mode was entered (every WIDE_REPROBE-th runs narrow again)
    bool last_narrow_large = false; // the last search was a large batch with the narrow plan and the second pass behind it
    long long last_narrow_nq = 0;   // ... and its size: the flagged counters read at the NEXT search are fractions of THIS batch
    // The second pass costs a search that flags nothing two launches that read a counter and leave (~9 us per 10 000-query
    // step). They are armed while nothing is known about the corpus (the first searches of an index) and whenever a recent
    // search flagged more queries than the streaming kernel takes cheaply; after PASS2_DISARM_AFTER consecutive searches
    // that flagged fewer they are left out (a batch that then flags many takes the exact re-search once and re-arms them).
    int p2_clean = 0;              // consecutive evaluated searches with <= PASS2_SKIP queries flagged by the first finalize
    bool p2_eval_pending = false;  // the last search's counters have not been looked at yet
    // The exact re-search behind every search is four launches: streaming kernel + list reduction (few flagged queries:
    // one corpus sweep per 8) and fp32-MFMA kernel + finalize (many). With nothing flagged each reads a counter and leaves.
    // After `sparse_need` consecutive searches whose re-search had nothing to do (counted on the device, so searches the
    // host never looked at count too) the streaming pair is left out and the MFMA kernel takes any count >= 1. Measured at
    // 10 000 x 37 000 (profiles/r03_sparse_fallback_policy.log): the pair costs a clean search ~3.4 us (0.5 %); without it
    // a search with 1-8 flagged queries takes 1.25 instead of 0.72 ms, once - the run restarts and the requirement
    // doubles. The break-even of the two is ~150 clean searches (ski rental); 96 stays below it (at most 2.6 x the
    // cost of the best fixed choice in hindsight, 2 x at the break-even).
    int sparse_need = SPARSE_DISARM_AFTER;
    int sparse_run_seen = 0;       // the device's run length when the host last saw a completed search
    bool sparse_disarmed = false;  // the last fast-path search went without the streaming pair

    // after the corpus-shape probe (and nowhere else): everything the probe's own search left behind goes, its verdict stays
    void reset() { const bool w = wide_mode; *this = SearchPolicy{}; wide_mode = w; }
    // icd_index_set_second_pass: second pass and streaming pair re-armed; wide mode only survives with both switches on
    void rearm(bool keep_wide) {
        if (!keep_wide) { wide_mode = false; last_narrow_large = false; }
        p2_clean = 0; p2_eval_pending = false;
        sparse_need = SPARSE_DISARM_AFTER; sparse_run_seen = 0; sparse_disarmed = false;
    }
    bool pass2_armed() const { return p2_clean < PASS2_DISARM_AFTER; }
};

// The previous search's counters have arrived (its copy event has completed; never called while a search is being captured
// into a HIP graph, where nothing may be queried). If that search was a large batch on the narrow plan and its second coarse
// pass had to take in a quarter of the queries and certified most of them, the corpus is one of tight families (ICD sibling
// codes): large batches then start with the second pass's list count (1.5 instead of 2.2 ms per 10 000 queries there; 7 %
// slower on Gaussian data, which is why it is not the default).
inline void policy_take_verdicts(SearchPolicy &p, const SearchCounters &c);
inline void policy_take_counters(SearchPolicy &p, const SearchCounters &c) {
    if (p.sparse_disarmed && c.clean_run < p.sparse_need) p.sparse_need = std::min(p.sparse_need * 2, SPARSE_NEED_MAX);   // an incident
    p.sparse_run_seen = c.clean_run;
    policy_take_verdicts(p, c);
}

// ... its two verdicts on the search the counters belong to: was the second pass needed, is the corpus one of families
inline void policy_take_verdicts(SearchPolicy &p, const SearchCounters &c) {
    if (p.p2_eval_pending) {
        p.p2_clean = c.f0 > PASS2_SKIP ? 0 : std::min(p.p2_clean + 1, 1 << 20);
        p.p2_eval_pending = false;
    }
    if (p.last_narrow_large) {
        const long long n_prev = p.last_narrow_nq;   // (the size of the batch the counters belong to, not the current one's: ADVICE r3)
        if (n_prev > 0) {
            if (!p.wide_mode && (long long)c.f0 * 4 > n_prev && (long long)c.f2 * 2 < c.f0) { p.wide_mode = true; p.wide_runs = 0; }
            else if (p.wide_mode && (long long)c.f0 * 20 <= n_prev) p.wide_mode = false;   // (a narrow re-probe that certified 95 %)
        }
        p.last_narrow_large = false;
    }
}

// A search that is not planned here (MODE_EXACT, a banded search, k above the fast path's, the few-query streaming forms) clears
// counter [0] and leaves the counters behind itself like every search: whoever reads them next reads ITS zero, not what the last
// planned search flagged. Unjudged, a narrow large batch followed by one MODE_EXACT or one-query call never switched the index to
// wide mode, and a narrow re-probe followed by one switched a family corpus OUT of it (20 * 0 <= n). Called before such a search
// is enqueued: `arrived` the counters in host memory if the last search has completed (they are the planned search's, any
// unplanned one in between came through here), else nullptr and the two verdicts are dropped. The streaming pair's run length
// [4] passes through unplanned searches untouched and is taken in by the next planned one.
inline void policy_unplanned_search(SearchPolicy &p, const SearchCounters *arrived) {
    if (arrived) policy_take_verdicts(p, *arrived);
    p.last_narrow_large = false;
    p.p2_eval_pending = false;
}

// This search's plan. Every WIDE_REPROBE-th large search in wide mode runs narrow again and decides anew. (Also called while
// capturing: the plan is the one the host state gives now, and it is frozen into the graph.)
struct SearchDecision { bool sparse_off, wide_now; };
inline SearchDecision policy_decide(SearchPolicy &p, bool adapt_enabled, long long nq, int k, int chunks_override) {
    SearchDecision d{};
    d.sparse_off = adapt_enabled && p.sparse_run_seen >= p.sparse_need;
    p.sparse_disarmed = d.sparse_off;
    if (nq >= WIDE_MIN_NQ && p.wide_mode && chunks_override == 0 && k <= 32) d.wide_now = (++p.wide_runs % WIDE_REPROBE) != 0;
    return d;
}

// What this search was, for the counters it leaves: `p2` the lists per query of its second pass (0: none was planned),
// `first_pass_cand` the candidates per query of its first pass (pc * kp).
inline void policy_note_search(SearchPolicy &p, bool adapt_enabled, bool pass2_enabled, long long nq, int p2, bool wide_now,
                               int chunks_override, int first_pass_cand) {
    p.last_narrow_large = adapt_enabled && nq >= WIDE_MIN_NQ && p2 > 0 && !wide_now && chunks_override == 0;
    if (p.last_narrow_large) p.last_narrow_nq = nq;
    p.p2_eval_pending = pass2_enabled && first_pass_cand < PASS2_BELOW;   // (a search the second pass applies to, armed or not)
}

}  // namespace icd
