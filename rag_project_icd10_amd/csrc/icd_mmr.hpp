// icd_mmr.hpp - MMR search (icd_mmr_*, icd_index_search_mmr). Part of icd_search.hip's translation unit
// (fail(), HIP_TRY, the owned-handle, request and host-call helpers, run_search, the band and mask checks); included there and
// nowhere else.
#pragma once

// An MMR handle belongs to the index it was created for but keeps no pointer into it: handle and identity are compared, never
// followed. Its workspace - the staging of the candidate lists, the staging of host callers' outputs - is allocated here, never
// in a search.
struct icd_mmr : OwnedHandle {
    static constexpr uint32_t MAGIC = 0x1CD33A21u;
    static constexpr const char *NOUN = "mmr";
    int64_t max_nq = 0;
    float *st_raw = nullptr; long long *st_ids = nullptr; int *st_lv = nullptr;   // [max_nq][ICD_MAX_K] the candidate lists of a call, [nq][fetch_k] used
    double *o_adj = nullptr, *o_mmr = nullptr; float *o_raw = nullptr; long long *o_ids = nullptr; int *o_lv = nullptr;   // [max_nq][ICD_MAX_K] a host caller's outputs
    std::mutex mu;
};

extern "C" {

int icd_mmr_create(icd_index *idx, int64_t max_nq, icd_mmr **out) {
    if (!out) return fail(ICD_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!valid(idx)) return fail(ICD_ERR_STATE, "invalid handle");
    if (max_nq <= 0 || max_nq > 0x7FFFFFFFll / ICD_MAX_K) return fail(ICD_ERR_INVALID, "max_nq=%lld", (long long)max_nq);
    if (idx->row_map) return fail(ICD_ERR_UNSUPPORTED, "an MMR search on a view is not supported: mask the parent");
    HIP_TRY(hipSetDevice(idx->device));
    icd_mmr *m = new_handle<icd_mmr>(idx);
    if (!m) return fail(ICD_ERR_NOMEM, "host allocation failed");
    m->max_nq = max_nq;
    const size_t no = (size_t)max_nq * ICD_MAX_K;
#define MM_TRY(expr) HIP_TRY_OR(free_handle(m), expr)
    MM_TRY(m->alloc(&m->st_raw, no)); MM_TRY(m->alloc(&m->st_ids, no)); MM_TRY(m->alloc(&m->st_lv, no));
    MM_TRY(m->alloc(&m->o_adj, no)); MM_TRY(m->alloc(&m->o_mmr, no)); MM_TRY(m->alloc(&m->o_raw, no)); MM_TRY(m->alloc(&m->o_ids, no)); MM_TRY(m->alloc(&m->o_lv, no));
#undef MM_TRY
    m->bytes = no * (4 + 8 + 4) + no * (8 + 8 + 4 + 8 + 4);
    *out = m;
    return ICD_OK;
}

int icd_mmr_destroy(icd_mmr *mmr) { return destroy_handle(mmr); }

int icd_mmr_stats(icd_mmr *mmr, int64_t *out_max_nq, int64_t *out_bytes) {
    if (!valid_handle(mmr)) return fail(ICD_ERR_STATE, "invalid mmr handle");
    if (out_max_nq) *out_max_nq = mmr->max_nq;
    if (out_bytes) *out_bytes = (int64_t)mmr->bytes;
    return ICD_OK;
}

int icd_index_search_mmr(icd_index *idx, icd_mmr *mmr, icd_rowmask *const *masks, const float *queries, int64_t nq, int32_t k,
                         int32_t fetch_k, double lambda, int32_t queries_on_device, const float *radius, const float *range_filter,
                         int32_t bounds_on_device, int32_t reweighted, double *out_adj, float *out_raw, int64_t *out_ids,
                         int32_t *out_levels, double *out_mmr, int32_t out_on_device, void *stream) {
    // every check comes before the first device call
    if (!valid(idx)) return fail(ICD_ERR_STATE, "invalid handle");
    if (!valid_handle(mmr)) return fail(ICD_ERR_STATE, "invalid mmr handle");
    icd_mmr *m = mmr;
    if (idx->row_map) return fail(ICD_ERR_UNSUPPORTED, "an MMR search on a view is not supported: mask the parent");
    int rc = check_owner(m->at, idx, "the mmr handle");
    if (rc) return rc;
    if (fetch_k < 1 || fetch_k > ICD_MAX_K) return fail(ICD_ERR_INVALID, "fetch_k=%d: an MMR search fetches 1 .. %d candidates per query", fetch_k, ICD_MAX_K);
    if (k < 1 || k > fetch_k) return fail(ICD_ERR_INVALID, "k=%d: an MMR search returns 1 .. fetch_k=%d hits per query", k, fetch_k);
    if (fetch_k > idx->max_k) return fail(ICD_ERR_INVALID, "fetch_k=%d exceeds the index's max_k=%d", fetch_k, idx->max_k);
    if (nq < 0) return fail(ICD_ERR_INVALID, "nq=%lld", (long long)nq);
    if (nq > m->max_nq) return fail(ICD_ERR_INVALID, "nq=%lld exceeds the mmr handle's max_nq=%lld", (long long)nq, (long long)m->max_nq);
    if (nq > idx->max_nq) return fail(ICD_ERR_INVALID, "nq=%lld exceeds the index's max_nq=%d", (long long)nq, idx->max_nq);
    if (!(lambda >= 0.0 && lambda <= 1.0)) return fail(ICD_ERR_INVALID, "lambda=%g: the relevance weight lies in [0, 1]", lambda);
    if (!out_raw || !out_ids || (reweighted && !out_adj)) return fail(ICD_ERR_INVALID, "output pointer is NULL");
    const RangeBounds rb{radius, range_filter, nullptr, nullptr, bounds_on_device != 0};
    if ((rc = check_bands(rb, nq, "query"))) return rc;
    bool any_mask = false;
    if (masks && (rc = check_masks(idx, masks, nq, "masked MMR search", &any_mask))) return rc;
    if (nq == 0) return ICD_OK;
    if (!queries) return fail(ICD_ERR_INVALID, "queries is NULL");
    std::lock_guard<std::mutex> guard(m->mu);
    HIP_TRY(hipSetDevice(idx->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const HostCall hc{s, queries_on_device != 0, out_on_device != 0};
    const bool host_bands = !bounds_on_device;   // (as run_search sees a banded request: the bands, unbounded ones too, are packed on the host)
    bool capturing;
    if ((rc = check_capture(s, !queries_on_device || !out_on_device, host_bands, any_mask, &capturing))) return rc;
    // step 1 (its capture checks are the ones made above): ONE sub-search at fetch_k into the staging - icd_index_search_masked's
    // request, raw form: the banded EXACT search, with the table when it holds a mask. Host queries go through the index's own
    // staging, as for every search.
    rc = run_search(idx, SearchRequest{queries, nq, fetch_k, queries_on_device != 0, true, ICD_MODE_EXACT,
                                       outs_for(false, nullptr, m->st_raw, reinterpret_cast<int64_t *>(m->st_ids), m->st_lv), &rb,
                                       any_mask ? masks : nullptr, s, &capturing});
    if (rc) return rc;
    // step 2: the select
    MmrArgs a{};
    a.st_raw = m->st_raw; a.st_ids = m->st_ids; a.st_levels = m->st_lv;
    a.corpus = idx->corpus; a.n = idx->n; a.id_base = idx->id_base;
    a.dim = idx->dim; a.k = k; a.fetch_k = fetch_k; a.reweighted = reweighted ? 1 : 0;
    a.lambda = lambda; a.one_minus = 1.0 - lambda;
    a.out_adj = reweighted ? hc.target(out_adj, m->o_adj) : nullptr;
    a.out_raw = hc.target(out_raw, m->o_raw);
    a.out_ids = hc.target(reinterpret_cast<long long *>(out_ids), m->o_ids);
    a.out_levels = hc.target(out_levels, m->o_lv);
    a.out_mmr = hc.target(out_mmr, m->o_mmr);
    hipLaunchKernelGGL(mmr_select_kernel, dim3((unsigned)nq), dim3(MMR_THREADS), (size_t)idx->dim * sizeof(float), s, a);
    HIP_TRY(hipGetLastError());
    if ((rc = hc.copy_back({{reweighted ? out_adj : nullptr, a.out_adj, 8}, {out_raw, a.out_raw, 4}, {out_ids, a.out_ids, 8},
                            {out_levels, a.out_levels, 4}, {out_mmr, a.out_mmr, 8}},
                           (size_t)nq * k)))
        return rc;
    return hc.finish();
}

}  // extern "C"
