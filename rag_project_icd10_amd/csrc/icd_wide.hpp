// icd_wide.hpp - wide search (icd_wide_*, icd_index_search_wide). Part of icd_search.hip's translation unit
// (fail(), HIP_TRY, the owned-handle and host-call helpers, launch_lds, the mask checks and the mask table's staging); included
// there and nowhere else.
#pragma once

// A wide-search workspace belongs to the index it was created for but keeps no pointer into it: handle and identity are compared,
// never followed. The score block, the candidate block, the threshold records and a host caller's queries, bounds and outputs
// are allocated here, never in a call.
struct icd_wide : OwnedHandle {
    static constexpr uint32_t MAGIC = 0x1CD0B17Eu;
    static constexpr const char *NOUN = "wide-search";
    int64_t max_nq = 0;
    int max_k = 0;
    WideLayout l{};
    float *q = nullptr;                                      // [max_nq][dim] a host caller's queries
    float *lo = nullptr, *hi = nullptr;                      // [max_nq] a host caller's bounds
    uint32_t *S = nullptr;                                   // [block][n_pad]
    u64 *C = nullptr;                                        // [block][max_k]
    WideRec *rec = nullptr;                                  // [block]
    double *o_adj = nullptr; float *o_raw = nullptr; long long *o_ids = nullptr; int *o_lv = nullptr;   // [block][max_k] a host caller's outputs
    int *o_count = nullptr; long long *o_sel = nullptr;      // [max_nq]
    std::mutex mu;
};

static hipError_t launch_wide_sort_emit(int device, int tier, unsigned blocks, hipStream_t s, const WideEmitArgs &e) {
    const size_t lds = ws_tier_lds_bytes(tier);
    const dim3 grid(blocks), block((unsigned)ws_tier_threads(tier));
    if (tier == 0) return launch_lds<wide_sort_emit_kernel<0>>(device, lds, grid, block, lds, s, e);
    if (tier == 1) return launch_lds<wide_sort_emit_kernel<1>>(device, lds, grid, block, lds, s, e);
    return launch_lds<wide_sort_emit_kernel<2>>(device, lds, grid, block, lds, s, e);
}

extern "C" {

int icd_wide_create(icd_index *idx, int64_t max_nq, int32_t max_k, icd_wide **out) {
    static_assert(WS_MAX_K == ICD_WIDE_MAX_K, "include/icd_search.h and wide_select_plan.hpp disagree");
    if (!out) return fail(ICD_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!valid(idx)) return fail(ICD_ERR_STATE, "invalid handle");
    if (max_nq <= 0 || max_nq > WS_MAX_NQ) return fail(ICD_ERR_INVALID, "max_nq=%lld: 1 .. %lld", (long long)max_nq, WS_MAX_NQ);
    if (max_k < 1 || max_k > ICD_WIDE_MAX_K) return fail(ICD_ERR_INVALID, "max_k=%d: 1 .. %d", max_k, ICD_WIDE_MAX_K);
    if (idx->row_map) return fail(ICD_ERR_UNSUPPORTED, "a wide search on a view is not supported: mask the parent");
    if (idx->n >= 0x80000000ll) return fail(ICD_ERR_UNSUPPORTED, "a wide search needs fewer than 2^31 rows");
    const WideLayout l = ws_layout(max_nq, max_k, idx->n, idx->dim);
    if (l.block < 1) return fail(ICD_ERR_UNSUPPORTED, "a wide search of %lld rows does not fit one score block of %zu bytes", (long long)idx->n, WS_BLOCK_BUDGET);
    HIP_TRY(hipSetDevice(idx->device));
    icd_wide *w = new_handle<icd_wide>(idx);
    if (!w) return fail(ICD_ERR_NOMEM, "host allocation failed");
    w->max_nq = max_nq; w->max_k = max_k; w->l = l;
#define WS_TRY(expr) HIP_TRY_OR(free_handle(w), expr)
    WS_TRY(w->alloc(&w->q, l.q_floats));
    WS_TRY(w->alloc(&w->lo, l.bounds)); WS_TRY(w->alloc(&w->hi, l.bounds));
    WS_TRY(w->alloc(&w->S, l.s_words)); WS_TRY(w->alloc(&w->C, l.c_keys)); WS_TRY(w->alloc(&w->rec, l.recs));
    WS_TRY(w->alloc(&w->o_adj, l.out_slots)); WS_TRY(w->alloc(&w->o_raw, l.out_slots)); WS_TRY(w->alloc(&w->o_ids, l.out_slots)); WS_TRY(w->alloc(&w->o_lv, l.out_slots));
    WS_TRY(w->alloc(&w->o_count, l.per_query)); WS_TRY(w->alloc(&w->o_sel, l.per_query));
#undef WS_TRY
    w->bytes = l.bytes;
    *out = w;
    return ICD_OK;
}

int icd_wide_destroy(icd_wide *ws) { return destroy_handle(ws); }

int icd_wide_stats(icd_wide *ws, int64_t *out_max_nq, int64_t *out_max_k, int64_t *out_bytes) {
    if (!valid_handle(ws)) return fail(ICD_ERR_STATE, "invalid wide-search handle");
    if (out_max_nq) *out_max_nq = ws->max_nq;
    if (out_max_k) *out_max_k = ws->max_k;
    if (out_bytes) *out_bytes = (int64_t)ws->bytes;
    return ICD_OK;
}

int icd_index_search_wide(icd_index *idx, icd_wide *ws, icd_rowmask *const *masks, const float *queries, int64_t nq, int32_t k, int32_t first,
                          int32_t queries_on_device, const float *lo, const float *hi, int32_t bounds_on_device, int32_t reweighted,
                          double *out_adj, float *out_raw, int64_t *out_ids, int32_t *out_levels, int32_t *out_count, int64_t *out_selected,
                          int32_t outputs_on_device, void *stream) {
    // every check comes before the first device call
    if (!valid(idx)) return fail(ICD_ERR_STATE, "invalid handle");
    if (!valid_handle(ws)) return fail(ICD_ERR_STATE, "invalid wide-search handle");
    icd_wide *w = ws;
    if (idx->row_map) return fail(ICD_ERR_UNSUPPORTED, "a wide search on a view is not supported: mask the parent");
    int rc = check_owner(w->at, idx, "the wide-search handle");
    if (rc) return rc;
    if (k < 1 || k > ICD_WIDE_MAX_K) return fail(ICD_ERR_INVALID, "k=%d outside 1..%d", k, ICD_WIDE_MAX_K);
    if (first < 0) return fail(ICD_ERR_INVALID, "first=%d is negative", first);
    if ((long long)first + k > ICD_WIDE_MAX_K) return fail(ICD_ERR_INVALID, "first=%d + k=%d exceeds %d", first, k, ICD_WIDE_MAX_K);
    if (first + k > w->max_k) return fail(ICD_ERR_INVALID, "first=%d + k=%d exceeds the wide-search handle's max_k=%d", first, k, w->max_k);
    if (nq < 0) return fail(ICD_ERR_INVALID, "nq=%lld", (long long)nq);
    if (nq > w->max_nq) return fail(ICD_ERR_INVALID, "nq=%lld exceeds the wide-search handle's max_nq=%lld", (long long)nq, (long long)w->max_nq);
    if (reweighted && !out_adj) return fail(ICD_ERR_INVALID, "out_adj is NULL in a reweighted search");
    if (!out_raw || !out_ids || !out_levels || !out_count || !out_selected)
        return fail(ICD_ERR_INVALID, "out_raw, out_ids, out_levels, out_count or out_selected is NULL");
    const RangeBounds rb{lo, hi, nullptr, nullptr, bounds_on_device != 0};
    if ((lo || hi) && (rc = check_bands(rb, nq, "query"))) return rc;
    bool any_mask = false;
    if (masks && (rc = check_masks(idx, masks, nq, "masked wide search", &any_mask))) return rc;
    if (nq == 0) return ICD_OK;
    if (!queries) return fail(ICD_ERR_INVALID, "queries is NULL");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool host_bounds = (lo || hi) && !bounds_on_device;
    if (stream_capturing(s)) {   // device in, device out enqueues only; whatever is staged on the host or synchronises is refused
        if (!queries_on_device || !outputs_on_device) return fail(ICD_ERR_INVALID, "a wide search with host buffers synchronises: it cannot be captured into a graph");
        if (host_bounds) return fail(ICD_ERR_INVALID, "a wide search with host bounds is staged at call time: it cannot be captured into a graph");
        if (any_mask) return fail(ICD_ERR_INVALID, "a masked wide search stages its mask table on the host at call time: it cannot be captured into a graph");
    }
    std::lock_guard<std::mutex> guard(w->mu);
    std::lock_guard<std::mutex> index_guard(idx->mu);   // (the mask table's pinned block is the index's)
    HIP_TRY(hipSetDevice(idx->device));
    const HostCall hc{s, queries_on_device != 0, outputs_on_device != 0};
    const float *dq = nullptr;
    if ((rc = hc.upload(queries, w->q, (size_t)nq * idx->dim, &dq))) return rc;
    const float *dlo = lo, *dhi = hi;
    if (host_bounds) {
        if (lo) { HIP_TRY(hipMemcpyAsync(w->lo, lo, (size_t)nq * sizeof(float), hipMemcpyHostToDevice, s)); dlo = w->lo; }
        if (hi) { HIP_TRY(hipMemcpyAsync(w->hi, hi, (size_t)nq * sizeof(float), hipMemcpyHostToDevice, s)); dhi = w->hi; }
    }
    if (any_mask && (rc = stage_masks(idx, masks, (int)nq, s))) return rc;
    const int width = first + k, tier = ws_tier(width);
    int *d_count = hc.target(out_count, w->o_count);
    long long *d_sel = hc.target(reinterpret_cast<long long *>(out_selected), w->o_sel);
    for (int64_t q0 = 0; q0 < nq; q0 += w->l.block) {   // one score block at a time
        const int nb = (int)std::min<int64_t>(w->l.block, nq - q0);
        // step 1: the block's ordered scores
        const RankOfPlan p = rk_plan(nb, idx->n, idx->num_cu);
        WideScoreArgs a{};
        a.corpus = idx->corpus; a.queries = dq + (size_t)q0 * idx->dim; a.mask = any_mask ? idx->mask_dev + q0 : nullptr;
        a.lo = dlo ? dlo + q0 : nullptr; a.hi = dhi ? dhi + q0 : nullptr;
        a.S = w->S; a.n_pad = w->l.n_pad; a.nq = nb; a.n = (int)idx->n; a.dim = idx->dim; a.chunks = p.chunks; a.rows_per_chunk = p.rows_per_chunk;
        HIP_TRY(launch_lds<wide_scores_kernel>(idx->device, rk_sweep_lds_bytes(), dim3((unsigned)p.grid), dim3(RK_THREADS), rk_sweep_lds_bytes(), s, a));
        // steps 2 and 3: the threshold of every query, then its candidates
        WideSelectArgs sel{};
        sel.S = w->S; sel.rec = w->rec; sel.C = w->C; sel.n_pad = w->l.n_pad; sel.width = width;
        hipLaunchKernelGGL(wide_threshold_kernel, dim3((unsigned)nb), dim3(WS_SELECT_THREADS), 0, s, sel);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(wide_collect_kernel, dim3((unsigned)nb), dim3(WS_SELECT_THREADS), 0, s, sel);
        HIP_TRY(hipGetLastError());
        // step 4: sort and emit - a host caller's block goes through the staging and is copied back behind the kernel
        const size_t o0 = hc.out_on_device ? (size_t)q0 * (size_t)k : 0;
        WideEmitArgs e{};
        e.C = w->C; e.rec = w->rec; e.levels = idx->levels;
        e.out_adj = reweighted ? hc.target(out_adj, w->o_adj) + o0 : nullptr;
        e.out_raw = hc.target(out_raw, w->o_raw) + o0;
        e.out_ids = hc.target(reinterpret_cast<long long *>(out_ids), w->o_ids) + o0;
        e.out_levels = hc.target(out_levels, w->o_lv) + o0;
        e.out_count = d_count + q0; e.out_selected = d_sel + q0;
        e.id_base = idx->id_base; e.width = width; e.first = first; e.k = k; e.reweighted = reweighted ? 1 : 0;
        HIP_TRY(launch_wide_sort_emit(idx->device, tier, (unsigned)nb, s, e));
        const size_t h0 = (size_t)q0 * (size_t)k;
        if ((rc = hc.copy_back({{reweighted ? out_adj + h0 : nullptr, w->o_adj, 8}, {out_raw + h0, w->o_raw, 4}, {out_ids + h0, w->o_ids, 8}, {out_levels + h0, w->o_lv, 4}},
                               (size_t)nb * (size_t)k))) return rc;
    }
    if ((rc = hc.copy_back({{out_count, w->o_count, 4}, {out_selected, w->o_sel, 8}}, (size_t)nq))) return rc;
    return hc.finish();
}

}  // extern "C"
