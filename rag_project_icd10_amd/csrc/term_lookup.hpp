// term_lookup.hpp — the ICD terminology scan of the confidence service on the device.
//
// Reference (services/multidimensional_confidence_service.py):
//   :677-694  _get_term_specificity_from_icd: on a miss of the exact lookup, the first name of the terminology cache (dict
//             order: first occurrence in the CSV) with `term in name or name in term` and len(term) >= 2, len(name) >= 2
//
// One work-group of 256 threads (four wave64s) per term. The term sits in LDS; every pass, each lane tests one name of a
// 256-name block in cache order with a plain compare loop over code points (Python str containment on int32 code points).
// After each block the work-group takes the minimum index of the block's hits (an LDS atomicMin) and stops at the first
// block that holds one. The answer is a minimum, so it does not depend on how the lanes are scheduled. Lane 0 stores it.
#pragma once
#include <hip/hip_runtime.h>
#include <climits>

namespace icd {

constexpr int TERM_MAX_LEN = 32;     // ICD_TERM_MAX_LEN: code points of a term the kernel takes
constexpr int TERM_BLOCK = 256;

struct TermArgs {
    const int *key_cp;    // code points of every name, back to back
    const int *key_off;   // [n_keys + 1]
    int n_keys;
    const int *term_cp;
    const int *term_off;  // [n_terms + 1], every term 0 .. TERM_MAX_LEN code points (checked by the caller)
    int n_terms;
    int *out_first;       // [n_terms]: the first index, or -1
};

// does the string a[0 .. la) contain b[0 .. lb) (lb <= la)? a in global memory, b in LDS, or the other way round
template <typename PA, typename PB>
__device__ __forceinline__ bool contains(PA a, int la, PB b, int lb) {
    for (int s = 0; s + lb <= la; ++s) {
        int j = 0;
        while (j < lb && a[s + j] == b[j]) ++j;
        if (j == lb) return true;
    }
    return false;
}

__global__ __launch_bounds__(TERM_BLOCK) void term_first_match_kernel(TermArgs a) {
    __shared__ int term[TERM_MAX_LEN];
    __shared__ int best;
    const int t = blockIdx.x;
    const int tid = threadIdx.x;
    const int t0 = a.term_off[t];
    const int lt = a.term_off[t + 1] - t0;
    if (tid < lt) term[tid] = a.term_cp[t0 + tid];
    if (tid == 0) best = INT_MAX;
    __syncthreads();
    if (lt >= 2) {   // (the reference's condition needs len(term) >= 2: shorter terms find nothing)
        for (int base = 0; base < a.n_keys; base += TERM_BLOCK) {
            const int i = base + tid;
            if (i < a.n_keys) {
                const int k0 = a.key_off[i];
                const int lk = a.key_off[i + 1] - k0;
                const int *key = a.key_cp + k0;
                bool hit = false;
                if (lk >= 2) hit = lt <= lk ? contains(key, lk, (const int *)term, lt) : contains((const int *)term, lt, key, lk);
                if (hit) atomicMin(&best, i);
            }
            __syncthreads();
            const int found = best;
            __syncthreads();   // (every lane has read `best` before any lane of the next block may write it)
            if (found != INT_MAX) break;
        }
    }
    if (tid == 0) a.out_first[t] = best == INT_MAX ? -1 : best;
}

}  // namespace icd
