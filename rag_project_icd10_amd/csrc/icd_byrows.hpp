// icd_byrows.hpp - search by stored rows (icd_byrows_*, icd_index_search_by_rows). Part of icd_search.hip's
// translation unit (fail(), HIP_TRY, the owned-handle, request and host-call helpers, run_search, the band and mask checks);
// included there and nowhere else.
#pragma once

// A by-rows workspace belongs to the index it was created for but keeps no pointer into it: handle and identity are compared,
// never followed. The query block, the staged lists, a host caller's ids and outputs are allocated here, never in a search.
struct icd_byrows : OwnedHandle {
    static constexpr uint32_t MAGIC = 0x1CD0B405u;
    static constexpr const char *NOUN = "by-rows";
    int64_t max_nq = 0;
    float *q = nullptr;                                                            // [max_nq][dim] the gathered rows
    long long *ids = nullptr; int *flag = nullptr;                                 // [max_nq] a host caller's ids; 1: no row of the index
    float *st_raw = nullptr; long long *st_ids = nullptr; int *st_lv = nullptr;    // [max_nq][BR_MAX_LIST] the lists of a call, [nq][k + 1] used
    double *o_adj = nullptr; float *o_raw = nullptr; long long *o_ids = nullptr; int *o_lv = nullptr;   // [max_nq][BR_MAX_LIST] a host caller's outputs
    std::mutex mu;
};

extern "C" {

int icd_byrows_create(icd_index *idx, int64_t max_nq, icd_byrows **out) {
    static_assert(BR_MAX_LIST == ICD_MAX_K, "include/icd_search.h and byrows_plan.hpp disagree");
    if (!out) return fail(ICD_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!valid(idx)) return fail(ICD_ERR_STATE, "invalid handle");
    if (max_nq <= 0 || max_nq > 0x7FFFFFFFll / ICD_MAX_K) return fail(ICD_ERR_INVALID, "max_nq=%lld", (long long)max_nq);
    if (idx->row_map) return fail(ICD_ERR_UNSUPPORTED, "a search by rows on a view is not supported: mask the parent");
    HIP_TRY(hipSetDevice(idx->device));
    icd_byrows *w = new_handle<icd_byrows>(idx);
    if (!w) return fail(ICD_ERR_NOMEM, "host allocation failed");
    w->max_nq = max_nq;
    const ByRowsLayout l = br_layout(max_nq, idx->dim);
#define BR_TRY(expr) HIP_TRY_OR(free_handle(w), expr)
    BR_TRY(w->alloc(&w->q, l.q_floats));
    BR_TRY(w->alloc(&w->ids, l.per_query)); BR_TRY(w->alloc(&w->flag, l.per_query));
    BR_TRY(w->alloc(&w->st_raw, l.list_slots)); BR_TRY(w->alloc(&w->st_ids, l.list_slots)); BR_TRY(w->alloc(&w->st_lv, l.list_slots));
    BR_TRY(w->alloc(&w->o_adj, l.out_slots)); BR_TRY(w->alloc(&w->o_raw, l.out_slots)); BR_TRY(w->alloc(&w->o_ids, l.out_slots)); BR_TRY(w->alloc(&w->o_lv, l.out_slots));
#undef BR_TRY
    w->bytes = l.bytes;
    *out = w;
    return ICD_OK;
}

int icd_byrows_destroy(icd_byrows *ws) { return destroy_handle(ws); }

int icd_byrows_stats(icd_byrows *ws, int64_t *out_max_nq, int64_t *out_bytes) {
    if (!valid_handle(ws)) return fail(ICD_ERR_STATE, "invalid by-rows handle");
    if (out_max_nq) *out_max_nq = ws->max_nq;
    if (out_bytes) *out_bytes = (int64_t)ws->bytes;
    return ICD_OK;
}

int icd_index_search_by_rows(icd_index *idx, icd_byrows *ws, icd_rowmask *const *masks, const int64_t *ids, int64_t nq, int32_t k,
                             int32_t ids_on_device, int32_t include_self, const float *radius, const float *range_filter,
                             int32_t bounds_on_device, int32_t reweighted, double *out_adj, float *out_raw, int64_t *out_ids,
                             int32_t *out_levels, int32_t out_on_device, void *stream) {
    // every check comes before the first device call
    if (!valid(idx)) return fail(ICD_ERR_STATE, "invalid handle");
    if (!valid_handle(ws)) return fail(ICD_ERR_STATE, "invalid by-rows handle");
    icd_byrows *w = ws;
    if (idx->row_map) return fail(ICD_ERR_UNSUPPORTED, "a search by rows on a view is not supported: mask the parent");
    int rc = check_owner(w->at, idx, "the by-rows handle");
    if (rc) return rc;
    const int len = include_self ? k : k + 1;   // the slots of the sub-search: the row's own hit takes one
    if (k < 1 || len > ICD_MAX_K)
        return fail(ICD_ERR_INVALID, "k=%d: a search by rows returns 1 .. %d hits per query (%d with include_self)", k, ICD_MAX_K - 1, ICD_MAX_K);
    if (len > idx->max_k) return fail(ICD_ERR_INVALID, "k=%d: the search runs at %d, above the index's max_k=%d", k, len, idx->max_k);
    if (nq < 0) return fail(ICD_ERR_INVALID, "nq=%lld", (long long)nq);
    if (nq > w->max_nq) return fail(ICD_ERR_INVALID, "nq=%lld exceeds the by-rows handle's max_nq=%lld", (long long)nq, (long long)w->max_nq);
    if (nq > idx->max_nq) return fail(ICD_ERR_INVALID, "nq=%lld exceeds the index's max_nq=%d", (long long)nq, idx->max_nq);
    if (!out_raw || !out_ids || (reweighted && !out_adj)) return fail(ICD_ERR_INVALID, "output pointer is NULL");
    if (nq > 0 && !ids) return fail(ICD_ERR_INVALID, "ids is NULL");
    if (!ids_on_device)
        for (int64_t q = 0; q < nq; ++q)
            if (br_row_of(ids[q], idx->id_base, idx->n) < 0)
                return fail(ICD_ERR_INVALID, "ids[%lld]=%lld outside the index's [%lld, %lld)", (long long)q, (long long)ids[q], (long long)idx->id_base, (long long)(idx->id_base + idx->n));
    const RangeBounds rb{radius, range_filter, nullptr, nullptr, bounds_on_device != 0};
    if ((rc = check_bands(rb, nq, "query"))) return rc;
    bool any_mask = false;
    if (masks && (rc = check_masks(idx, masks, nq, "masked search by rows", &any_mask))) return rc;
    if (nq == 0) return ICD_OK;
    std::lock_guard<std::mutex> guard(w->mu);
    HIP_TRY(hipSetDevice(idx->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const HostCall hc{s, ids_on_device != 0, out_on_device != 0};
    const bool host_bands = !bounds_on_device;   // (as run_search sees a banded request: the bands, unbounded ones too, are packed on the host)
    bool capturing;
    if ((rc = check_capture(s, !ids_on_device || !out_on_device, host_bands, any_mask, &capturing))) return rc;
    // step 1: the rows -> the query block
    const long long *dids = reinterpret_cast<const long long *>(ids);
    if (!ids_on_device) {
        HIP_TRY(hipMemcpyAsync(w->ids, ids, (size_t)nq * sizeof(long long), hipMemcpyHostToDevice, s));
        dids = w->ids;
    }
    const dim3 grid((unsigned)br_blocks(nq));
    ByRowsGatherArgs g{};
    g.corpus = idx->corpus; g.ids = dids; g.q = w->q; g.flag = w->flag;
    g.n = idx->n; g.id_base = idx->id_base; g.dim = idx->dim; g.nq = (int)nq;
    hipLaunchKernelGGL(byrows_gather_kernel, grid, dim3(BR_THREADS), 0, s, g);
    HIP_TRY(hipGetLastError());
    // step 2 (its capture checks are the ones made above): icd_index_search_masked's request, raw form, at k + 1 - device queries,
    // device outputs: the staging
    rc = run_search(idx, SearchRequest{w->q, nq, len, true, true, ICD_MODE_EXACT,
                                       outs_for(false, nullptr, w->st_raw, reinterpret_cast<int64_t *>(w->st_ids), w->st_lv), &rb,
                                       any_mask ? masks : nullptr, s, &capturing});
    if (rc) return rc;
    // step 3: the drop (and the level reweight of the k that stay)
    ByRowsDropArgs a{};
    a.st_raw = w->st_raw; a.st_ids = w->st_ids; a.st_levels = w->st_lv; a.ids = dids; a.flag = w->flag;
    a.out_adj = reweighted ? hc.target(out_adj, w->o_adj) : nullptr;
    a.out_raw = hc.target(out_raw, w->o_raw);
    a.out_ids = hc.target(reinterpret_cast<long long *>(out_ids), w->o_ids);
    a.out_levels = hc.target(out_levels, w->o_lv);
    a.nq = (int)nq; a.len = len; a.keep = k; a.reweighted = reweighted ? 1 : 0;
    hipLaunchKernelGGL(byrows_drop_self_kernel, grid, dim3(BR_THREADS), 0, s, a);
    HIP_TRY(hipGetLastError());
    if ((rc = hc.copy_back({{reweighted ? out_adj : nullptr, a.out_adj, 8}, {out_raw, a.out_raw, 4}, {out_ids, a.out_ids, 8},
                            {out_levels, a.out_levels, 4}},
                           (size_t)nq * k)))
        return rc;
    return hc.finish();
}

}  // extern "C"
