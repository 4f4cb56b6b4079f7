// byrows_plan.hpp - the host-visible part of the search by stored rows: the workspace layout, the launch
// geometry, and the three index rules of the drop step - where the gap is, which slot of the (k + 1)-wide list an output slot
// reads, and the stable descending rank of the level reweight. No HIP header and no handle: included by byrows_kernel.hpp (the
// kernels call these very functions) and by tests/byrows_plan_check.cpp, which runs them under the host sanitizers.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BR_HD __host__ __device__
#else
#define BR_HD
#endif

namespace icd {

constexpr int BR_MAX_LIST = 128;                  // slots of one staged list (ICD_MAX_K): k + 1 <= BR_MAX_LIST
constexpr int BR_MAX_K = BR_MAX_LIST - 1;         // largest k of a search that removes the row's own hit
constexpr int BR_WAVE = 64;                       // one wave per query, in both kernels
constexpr int BR_WAVES = 4;                       // waves (queries) of one work-group
constexpr int BR_THREADS = BR_WAVE * BR_WAVES;
constexpr int BR_PER_LANE = BR_MAX_LIST / BR_WAVE;   // list entries a lane owns: lane and lane + 64

// work-groups of either kernel for nq queries
BR_HD inline long long br_blocks(long long nq) { return (nq + BR_WAVES - 1) / BR_WAVES; }

// Elements of the workspace's arrays for calls of up to max_nq queries on an index of `dim` columns. Everything is allocated at
// create; a search allocates nothing.
struct ByRowsLayout {
    size_t q_floats;      // [max_nq][dim]          the query block the exact kernels read
    size_t list_slots;    // [max_nq][BR_MAX_LIST]  the staged lists of a call: raw, ids, levels, [nq][k + 1] used
    size_t out_slots;     // [max_nq][BR_MAX_LIST]  a host caller's outputs: adj, raw, ids, levels, [nq][k] used
    size_t per_query;     // [max_nq]               the ids of a host caller, and the flag of every query
    size_t bytes;         // all of it
};
BR_HD inline ByRowsLayout br_layout(long long max_nq, int dim) {
    ByRowsLayout l;
    l.q_floats = (size_t)max_nq * (size_t)dim;
    l.list_slots = (size_t)max_nq * BR_MAX_LIST;
    l.out_slots = (size_t)max_nq * BR_MAX_LIST;
    l.per_query = (size_t)max_nq;
    l.bytes = l.q_floats * 4 + l.list_slots * (4 + 8 + 4) + l.out_slots * (8 + 4 + 8 + 4) + l.per_query * (8 + 4);
    return l;
}

// The row of the index a global id names, or -1 for an id outside [id_base, id_base + n). Unsigned arithmetic: no id, however
// wild (only a device caller can send one), overflows, and no address is formed from a row this refuses.
BR_HD inline long long br_row_of(long long id, long long id_base, long long n) {
    const unsigned long long r = (unsigned long long)id - (unsigned long long)id_base;
    return r < (unsigned long long)n ? (long long)r : -1ll;
}

// The gap: the position of the query's own id in its list of `len` slots, or `keep` (the list's last slot when len = keep + 1;
// no slot at all when len = keep) when it is absent. `first_hit` is the lowest position whose id equals the row's, len or more
// when there is none: what a ballot's lowest set bit gives.
BR_HD inline int br_gap(int first_hit, int len, int keep) { return first_hit < len ? first_hit : keep; }

// the slot of the staged list output slot j reads: everything behind the gap moves up by one
BR_HD inline int br_source(int j, int gap) { return j < gap ? j : j + 1; }

// The level reweight's order (icd_index_search_reweighted's step): the rank of entry j among adj[0 .. count) under ONE stable
// descending sort - the entries that are greater, and the equal ones in front of it. Padding (-inf) sits behind the hits and
// stays there: nothing is smaller, and equal entries keep their order.
BR_HD inline int br_stable_rank(const double *adj, int count, int j) {
    const double mine = adj[j];
    int pos = 0;
    for (int i = 0; i < count; ++i) {
        const double ai = adj[i];
        pos += (ai > mine || (ai == mine && i < j)) ? 1 : 0;
    }
    return pos;
}

}  // namespace icd
