// icd_boost.hpp - boosted search (icd_boost_*, icd_index_search_boosted). Part of icd_search.hip's
// translation unit (fail(), HIP_TRY, the owned-handle and request helpers, the band and mask checks, search_banded); included there
// and nowhere else.
#pragma once

static_assert(ICD_MAX_BOOSTS == BOOST_SLOTS, "include/icd_search.h and topk_select.hpp disagree");

// A boost workspace belongs to the index it was created for but keeps no pointer into it: handle and identity are compared, never
// followed. It holds what a call's boost table needs - the pinned block the host fills, its device copy, the event that guards
// the block, the all-zero bitset the MFMA kernel reads in an unused slot's place - allocated here, never in a search. One stream
// at a time: the block is refilled per call, behind the event of the call before.
struct icd_boost : OwnedHandle {
    static constexpr uint32_t MAGIC = 0x1CD3B057u;
    static constexpr const char *NOUN = "boost";
    int64_t max_nq = 0;
    BoostQ *h_tab = nullptr, *d_tab = nullptr;   // [max_nq] each
    uint32_t *zeros = nullptr;                   // [rowmask_tile_words(n) + ROWMASK_TAIL_WORDS]
    hipEvent_t ev = nullptr;
    bool copy_pending = false;
};

// The boost table of one call as its entry point checked it: [nq][ICD_MAX_BOOSTS] masks (NULL = slot unused) and weights.
struct BoostRequest {
    icd_boost *ws;
    icd_rowmask *const *masks;
    const float *weights;
};

// The table goes to the device as the mask table does (stage_masks): filled in the pinned block under the index's mutex, one copy
// per call, an event right behind the copy that the next call waits for before it refills the block.
static int stage_boosts(const BoostRequest &r, int nq, hipStream_t s, BoostDev *out) {
    icd_boost *b = r.ws;
    if (b->copy_pending) { HIP_TRY(hipEventSynchronize(b->ev)); b->copy_pending = false; }
    for (int q = 0; q < nq; ++q) {
        BoostQ &e = b->h_tab[q];
        for (int j = 0; j < ICD_MAX_BOOSTS; ++j) {
            const icd_rowmask *m = r.masks[(size_t)q * ICD_MAX_BOOSTS + j];
            e.m[j] = m ? m->bits : nullptr;
            e.w[j] = m ? r.weights[(size_t)q * ICD_MAX_BOOSTS + j] : 1.0f;
        }
    }
    const hipError_t ec = hipMemcpyAsync(b->d_tab, b->h_tab, (size_t)nq * sizeof(BoostQ), hipMemcpyHostToDevice, s);
    const hipError_t ee = hipEventRecord(b->ev, s);   // (also behind a copy that failed to enqueue, as in stage_masks)
    b->copy_pending = ee == hipSuccess;
    if (ec != hipSuccess || ee != hipSuccess) {
        hipStreamSynchronize(s);
        b->copy_pending = false;
        return fail(ICD_ERR_HIP, "boost table: %s", hipGetErrorString(ec != hipSuccess ? ec : ee));
    }
    out->q = b->d_tab;
    out->zeros = b->zeros;
    return ICD_OK;
}

extern "C" {

int icd_boost_create(icd_index *idx, int64_t max_nq, icd_boost **out) {
    if (!out) return fail(ICD_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!valid(idx)) return fail(ICD_ERR_STATE, "invalid handle");
    if (max_nq <= 0 || max_nq > 0x7FFFFFFFll / (int64_t)sizeof(BoostQ)) return fail(ICD_ERR_INVALID, "max_nq=%lld", (long long)max_nq);
    if (idx->row_map) return fail(ICD_ERR_UNSUPPORTED, "a boosted search on a view is not supported: mask the parent");
    HIP_TRY(hipSetDevice(idx->device));
    icd_boost *b = new_handle<icd_boost>(idx);
    if (!b) return fail(ICD_ERR_NOMEM, "host allocation failed");
    b->max_nq = max_nq;
    const size_t words = (size_t)rowmask_tile_words(idx->n) + ROWMASK_TAIL_WORDS;
#define BO_TRY(expr) HIP_TRY_OR((b->ev ? (void)hipEventDestroy(b->ev) : (void)0, free_handle(b)), expr)
    BO_TRY(b->alloc(&b->d_tab, (size_t)max_nq));
    BO_TRY(b->alloc(&b->zeros, words));
    BO_TRY(hipMemset(b->zeros, 0, words * sizeof(uint32_t)));
    void *pin = nullptr;
    BO_TRY(hipHostMalloc(&pin, (size_t)max_nq * sizeof(BoostQ), hipHostMallocDefault));
    b->pinned.push_back(pin);
    b->h_tab = reinterpret_cast<BoostQ *>(pin);
    BO_TRY(hipEventCreateWithFlags(&b->ev, hipEventDisableTiming));
#undef BO_TRY
    b->bytes = (size_t)max_nq * sizeof(BoostQ) * 2 + words * sizeof(uint32_t);
    *out = b;
    return ICD_OK;
}

int icd_boost_destroy(icd_boost *b) {
    hipEvent_t ev = valid_handle(b) ? b->ev : nullptr;
    const int rc = destroy_handle(b);   // (synchronises the workspace's device first)
    if (ev) hipEventDestroy(ev);
    return rc;
}

int icd_boost_stats(icd_boost *b, int64_t *out_max_nq, int64_t *out_bytes) {
    if (!valid_handle(b)) return fail(ICD_ERR_STATE, "invalid boost handle");
    if (out_max_nq) *out_max_nq = b->max_nq;
    if (out_bytes) *out_bytes = (int64_t)b->bytes;
    return ICD_OK;
}

// A table whose every slot is NULL is the masked search (which such a table equals bit for bit), under its name and through its
// request: the workspace is checked and left alone.
int icd_index_search_boosted(icd_index *idx, icd_boost *ws, icd_rowmask *const *masks, icd_rowmask *const *boost_masks,
                             const float *boost_weights, const float *queries, int64_t nq, int32_t k, int32_t queries_on_device,
                             const float *radius, const float *range_filter, const float *after_scores, const int64_t *after_ids,
                             int32_t bounds_on_device, int32_t reweighted, double *out_adj, float *out_raw, int64_t *out_ids,
                             int32_t *out_levels, int32_t out_on_device, void *stream) {
    // every check comes before the first device call
    if (!valid(idx)) return fail(ICD_ERR_STATE, "invalid handle");
    if (!valid_handle(ws)) return fail(ICD_ERR_STATE, "invalid boost handle");
    if (idx->row_map) return fail(ICD_ERR_UNSUPPORTED, "a boosted search on a view is not supported: mask the parent");
    int rc = check_owner(ws->at, idx, "the boost handle");
    if (rc) return rc;
    if (nq < 0) return fail(ICD_ERR_INVALID, "nq=%lld", (long long)nq);
    if (nq > ws->max_nq) return fail(ICD_ERR_INVALID, "nq=%lld exceeds the boost handle's max_nq=%lld", (long long)nq, (long long)ws->max_nq);
    if (nq > idx->max_nq) return fail(ICD_ERR_INVALID, "nq=%lld exceeds max_nq=%d", (long long)nq, idx->max_nq);   // (before a table is read)
    bool any_boost = false;
    for (int64_t i = 0; boost_masks && i < nq * ICD_MAX_BOOSTS; ++i) {
        const icd_rowmask *m = boost_masks[i];
        if (!m) continue;
        any_boost = true;
        const long long q = i / ICD_MAX_BOOSTS, j = i % ICD_MAX_BOOSTS;
        if (!valid_handle(m)) return fail(ICD_ERR_STATE, "boost_masks[%lld][%lld]: invalid row mask handle", q, j);
        char name[48];
        snprintf(name, sizeof name, "boost_masks[%lld][%lld]", q, j);
        if ((rc = check_owner(m->at, idx, name))) return rc;
        if (!boost_weights) return fail(ICD_ERR_INVALID, "boost_weights is NULL");
        const float w = boost_weights[i];
        if (!(std::fpclassify(w) == FP_NORMAL && w > 0.0f))
            return fail(ICD_ERR_INVALID, "boost_weights[%lld][%lld]=%g: a weight is a positive normal float", q, j, (double)w);
    }
    bool any_mask = false;
    if (masks && (rc = check_masks(idx, masks, nq, "boosted search", &any_mask))) return rc;
    // (whatever the table holds: the entry point's contract does not depend on its arguments' values)
    if (stream_capturing(reinterpret_cast<hipStream_t>(stream)))
        return fail(ICD_ERR_INVALID, "a boosted search stages its boost table on the host at call time: it cannot be captured into a graph");
    const RangeBounds rb{radius, range_filter, after_scores, reinterpret_cast<const long long *>(after_ids), bounds_on_device != 0};
    const BoostRequest br{ws, boost_masks, boost_weights};
    return search_banded(idx, any_mask ? masks : nullptr, any_boost ? "boosted" : (any_mask ? "masked" : "range"), queries, nq, k, queries_on_device,
                         rb, reweighted, out_adj, out_raw, out_ids, out_levels, out_on_device, stream, any_boost ? &br : nullptr);
}

}  // extern "C"
