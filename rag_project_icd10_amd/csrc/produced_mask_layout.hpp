// produced_mask_layout.hpp - where the parts of a produced-mask block lie (DESIGN.md sections 17.3 and 18.3): the ONE allocation
// that holds the nq masks of an icd_sparse_match_rowmasks / icd_filter_rowmasks call and what its kernel reads. Host only, no HIP
// header: included by icd_range_mask.hpp (ProducedMasks) and by tests/produced_mask_layout_check.cpp.
#pragma once
#include <cstddef>
#include <cstdint>

constexpr int PM_MAX_STAGED = 3;   // regions of its own an entry may stage behind the base pointers

// Byte offsets into the block. Every region starts 16-byte aligned; a region of no bytes takes none.
struct ProducedMaskLayout {
    size_t words;                   // 32-bit words of ONE bitset: whole 128-row tiles plus the 4 zero tail words (icd_rowmask's form)
    size_t bits;                    // [nq][words] bitsets (words is a multiple of 4: every bitset starts 16-byte aligned)
    size_t counters;                // [nq] int row counters
    size_t base;                    // [nq] base bitset pointers (with a base mask; else empty)
    size_t staged[PM_MAX_STAGED];   // the caller's regions, in its order
    size_t zeroed;                  // bytes from the block's start that are cleared before the launch: exactly bitsets + counters
    size_t total;
};

inline ProducedMaskLayout produced_mask_layout(int64_t nq, int64_t n, bool any_base, const size_t *staged_bytes, int n_staged) {
    const auto up16 = [](size_t b) { return (b + 15) / 16 * 16; };
    ProducedMaskLayout l{};
    l.words = (size_t)((n + 127) / 128 * 4 + 4);
    l.counters = (size_t)nq * l.words * 4;
    l.base = l.zeroed = l.counters + up16((size_t)nq * 4);
    size_t at = l.base + (any_base ? up16((size_t)nq * 8) : 0);
    for (int i = 0; i < n_staged && i < PM_MAX_STAGED; ++i) {
        l.staged[i] = at;
        at += up16(staged_bytes[i]);
    }
    l.total = at;
    return l;
}
