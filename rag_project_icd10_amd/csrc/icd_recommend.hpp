// icd_recommend.hpp - recommend search (icd_recommend_*, icd_index_recommend). Part of icd_search.hip's
// translation unit (fail(), HIP_TRY, the owned-handle and host-call helpers, launch_lds, the mask and band checks, the mask table's
// staging, icd_wide.hpp's launch_wide_sort_emit); included there, behind icd_wide.hpp, and nowhere else.
#pragma once

// A recommend workspace belongs to the index it was created for but keeps no pointer into it: handle and identity are compared,
// never followed. The example block E, its scores SE, the request block S, the candidate block, the threshold records, the
// request table (device and pinned host) and a host caller's vectors, bounds and outputs are allocated here, never in a call.
struct icd_recommend : OwnedHandle {
    static constexpr uint32_t MAGIC = 0x1CD0EC03u;
    static constexpr const char *NOUN = "recommend";
    int64_t max_requests = 0, max_examples = 0;
    int max_k = 0;
    RecommendLayout l{};
    float *v = nullptr;                                      // [max_examples][dim] a host caller's example vectors
    float *lo = nullptr, *hi = nullptr;                      // [max_requests] a host caller's bounds
    int *table = nullptr, *h_table = nullptr;                // rc_table_words: device, pinned host
    hipEvent_t ev_table = nullptr;                           // behind the table's copy: the next call waits for it before it refills h_table
    bool table_pending = false;
    float *E = nullptr;                                      // [block_examples][dim]
    uint32_t *SE = nullptr, *S = nullptr;                    // [block_examples][n_pad], [block][n_pad]
    u64 *C = nullptr;                                        // [block][max_k]
    WideRec *rec = nullptr;                                  // [block]
    double *o_adj = nullptr; float *o_raw = nullptr; long long *o_ids = nullptr; int *o_lv = nullptr;   // [block][max_k] a host caller's outputs
    int *o_count = nullptr; long long *o_sel = nullptr;      // [max_requests]
    int64_t last_vectors = 0;                                // vectors the last call's last block left in E (icd_recommend_read_vectors)
    std::mutex mu;
    ~icd_recommend() { if (ev_table) hipEventDestroy(ev_table); }
};

extern "C" {

int icd_recommend_create(icd_index *idx, int64_t max_requests, int64_t max_examples, int32_t max_k, icd_recommend **out) {
    static_assert(RC_MAX_EXAMPLES == ICD_RECOMMEND_MAX_EXAMPLES && RC_AVERAGE_VECTOR == ICD_RECOMMEND_AVERAGE_VECTOR &&
                  RC_BEST_SCORE == ICD_RECOMMEND_BEST_SCORE && RC_SUM_SCORES == ICD_RECOMMEND_SUM_SCORES,
                  "include/icd_search.h and recommend_plan.hpp disagree");
    if (!out) return fail(ICD_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!valid(idx)) return fail(ICD_ERR_STATE, "invalid handle");
    if (max_requests <= 0 || max_requests > RC_MAX_REQUESTS) return fail(ICD_ERR_INVALID, "max_requests=%lld: 1 .. %lld", (long long)max_requests, RC_MAX_REQUESTS);
    if (max_examples < max_requests || max_examples > max_requests * RC_MAX_EXAMPLES)
        return fail(ICD_ERR_INVALID, "max_examples=%lld: max_requests .. %d x max_requests", (long long)max_examples, RC_MAX_EXAMPLES);
    if (max_k < 1 || max_k > ICD_WIDE_MAX_K) return fail(ICD_ERR_INVALID, "max_k=%d: 1 .. %d", max_k, ICD_WIDE_MAX_K);
    if (idx->row_map) return fail(ICD_ERR_UNSUPPORTED, "a recommend search on a view is not supported: mask the parent");
    if (idx->n >= 0x80000000ll) return fail(ICD_ERR_UNSUPPORTED, "a recommend search needs fewer than 2^31 rows");
    const RecommendLayout l = rc_layout(max_requests, max_examples, max_k, idx->n, idx->dim);
    if (l.block < 1) return fail(ICD_ERR_UNSUPPORTED, "a recommend search of %lld rows does not fit one block of %zu bytes", (long long)idx->n, WS_BLOCK_BUDGET);
    HIP_TRY(hipSetDevice(idx->device));
    icd_recommend *w = new_handle<icd_recommend>(idx);
    if (!w) return fail(ICD_ERR_NOMEM, "host allocation failed");
    w->max_requests = max_requests; w->max_examples = max_examples; w->max_k = max_k; w->l = l;
#define RC_TRY(expr) HIP_TRY_OR(free_handle(w), expr)
    RC_TRY(w->alloc(&w->v, l.v_floats));
    RC_TRY(w->alloc(&w->lo, l.bounds)); RC_TRY(w->alloc(&w->hi, l.bounds));
    RC_TRY(w->alloc(&w->table, l.table));
    RC_TRY(hipHostMalloc(reinterpret_cast<void **>(&w->h_table), l.table * sizeof(int)));
    w->pinned.push_back(w->h_table);
    RC_TRY(hipEventCreateWithFlags(&w->ev_table, hipEventDisableTiming));
    RC_TRY(w->alloc(&w->E, l.e_floats)); RC_TRY(w->alloc(&w->SE, l.se_words));
    RC_TRY(w->alloc(&w->S, l.s_words)); RC_TRY(w->alloc(&w->C, l.c_keys)); RC_TRY(w->alloc(&w->rec, l.recs));
    RC_TRY(w->alloc(&w->o_adj, l.out_slots)); RC_TRY(w->alloc(&w->o_raw, l.out_slots)); RC_TRY(w->alloc(&w->o_ids, l.out_slots)); RC_TRY(w->alloc(&w->o_lv, l.out_slots));
    RC_TRY(w->alloc(&w->o_count, l.per_request)); RC_TRY(w->alloc(&w->o_sel, l.per_request));
#undef RC_TRY
    w->bytes = l.bytes;
    *out = w;
    return ICD_OK;
}

int icd_recommend_destroy(icd_recommend *ws) { return destroy_handle(ws); }

int icd_recommend_stats(icd_recommend *ws, int64_t *out_max_requests, int64_t *out_max_examples, int64_t *out_max_k, int64_t *out_bytes) {
    if (!valid_handle(ws)) return fail(ICD_ERR_STATE, "invalid recommend handle");
    if (out_max_requests) *out_max_requests = ws->max_requests;
    if (out_max_examples) *out_max_examples = ws->max_examples;
    if (out_max_k) *out_max_k = ws->max_k;
    if (out_bytes) *out_bytes = (int64_t)ws->bytes;
    return ICD_OK;
}

int icd_recommend_read_vectors(icd_recommend *ws, int64_t count, float *out) {
    if (!valid_handle(ws)) return fail(ICD_ERR_STATE, "invalid recommend handle");
    if (!out) return fail(ICD_ERR_INVALID, "out is NULL");
    std::lock_guard<std::mutex> guard(ws->mu);
    if (count < 0 || count > ws->last_vectors) return fail(ICD_ERR_INVALID, "count=%lld: the last block left %lld vectors", (long long)count, (long long)ws->last_vectors);
    if (count == 0) return ICD_OK;
    HIP_TRY(hipSetDevice(ws->at.device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, ws->E, (size_t)count * ws->at.dim * sizeof(float), hipMemcpyDeviceToHost));
    return ICD_OK;
}

int icd_index_recommend(icd_index *idx, icd_recommend *ws, icd_rowmask *const *masks, const int64_t *example_rows, const float *example_vectors,
                        const int64_t *example_off, const int32_t *n_positive, int64_t nr, int32_t strategy, int32_t k, int32_t first,
                        const float *lo, const float *hi, int32_t bounds_on_device, int32_t reweighted,
                        double *out_adj, float *out_raw, int64_t *out_ids, int32_t *out_levels, int32_t *out_count, int64_t *out_selected,
                        int32_t inputs_on_device, int32_t outputs_on_device, void *stream) {
    // every check comes before the first device call
    if (!valid(idx)) return fail(ICD_ERR_STATE, "invalid handle");
    if (!valid_handle(ws)) return fail(ICD_ERR_STATE, "invalid recommend handle");
    icd_recommend *w = ws;
    if (idx->row_map) return fail(ICD_ERR_UNSUPPORTED, "a recommend search on a view is not supported: mask the parent");
    int rc = check_owner(w->at, idx, "the recommend handle");
    if (rc) return rc;
    if (strategy != ICD_RECOMMEND_AVERAGE_VECTOR && strategy != ICD_RECOMMEND_BEST_SCORE && strategy != ICD_RECOMMEND_SUM_SCORES)
        return fail(ICD_ERR_INVALID, "strategy=%d: ICD_RECOMMEND_AVERAGE_VECTOR, _BEST_SCORE or _SUM_SCORES", strategy);
    if (k < 1 || k > ICD_WIDE_MAX_K) return fail(ICD_ERR_INVALID, "k=%d outside 1..%d", k, ICD_WIDE_MAX_K);
    if (first < 0) return fail(ICD_ERR_INVALID, "first=%d is negative", first);
    if ((long long)first + k > ICD_WIDE_MAX_K) return fail(ICD_ERR_INVALID, "first=%d + k=%d exceeds %d", first, k, ICD_WIDE_MAX_K);
    if (first + k > w->max_k) return fail(ICD_ERR_INVALID, "first=%d + k=%d exceeds the recommend handle's max_k=%d", first, k, w->max_k);
    if (nr < 0) return fail(ICD_ERR_INVALID, "nr=%lld", (long long)nr);
    if (nr > w->max_requests) return fail(ICD_ERR_INVALID, "nr=%lld exceeds the recommend handle's max_requests=%lld", (long long)nr, (long long)w->max_requests);
    if (reweighted && !out_adj) return fail(ICD_ERR_INVALID, "out_adj is NULL in a reweighted search");
    if (!out_raw || !out_ids || !out_levels || !out_count || !out_selected)
        return fail(ICD_ERR_INVALID, "out_raw, out_ids, out_levels, out_count or out_selected is NULL");
    const RangeBounds rb{lo, hi, nullptr, nullptr, bounds_on_device != 0};
    if ((lo || hi) && (rc = check_bands(rb, nr, "request"))) return rc;
    bool any_mask = false;
    if (masks && (rc = check_masks(idx, masks, nr, "masked recommend search", &any_mask))) return rc;
    if (nr == 0) return ICD_OK;
    if (!example_rows || !example_off || !n_positive) return fail(ICD_ERR_INVALID, "example_rows, example_off or n_positive is NULL");
    if (example_off[0] != 0) return fail(ICD_ERR_INVALID, "example_off[0]=%lld: offsets start at 0", (long long)example_off[0]);
    bool any_vector = false;
    for (int64_t r = 0; r < nr; ++r) {
        const int64_t cnt = example_off[r + 1] - example_off[r];
        if (cnt < 1 || cnt > ICD_RECOMMEND_MAX_EXAMPLES) return fail(ICD_ERR_INVALID, "request %lld holds %lld examples: 1 .. %d", (long long)r, (long long)cnt, ICD_RECOMMEND_MAX_EXAMPLES);
        if (example_off[r + 1] > w->max_examples) return fail(ICD_ERR_INVALID, "the call holds more examples than the recommend handle's max_examples=%lld", (long long)w->max_examples);
        if (n_positive[r] < 0 || n_positive[r] > cnt) return fail(ICD_ERR_INVALID, "n_positive[%lld]=%d of %lld examples", (long long)r, n_positive[r], (long long)cnt);
        if (strategy == ICD_RECOMMEND_AVERAGE_VECTOR && n_positive[r] < 1) return fail(ICD_ERR_INVALID, "request %lld: average_vector needs a positive example", (long long)r);
        for (int64_t e = example_off[r]; e < example_off[r + 1]; ++e) {
            if (example_rows[e] == -1) { any_vector = true; continue; }
            if (example_rows[e] < 0 || example_rows[e] >= idx->n) return fail(ICD_ERR_INVALID, "example_rows[%lld]=%lld outside [0, %lld) (-1: a vector)", (long long)e, (long long)example_rows[e], (long long)idx->n);
        }
    }
    const int64_t ne = example_off[nr];
    if (any_vector && !example_vectors) return fail(ICD_ERR_INVALID, "example_vectors is NULL and an example is a vector");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (stream_capturing(s)) return fail(ICD_ERR_INVALID, "a recommend search stages its request table on the host at call time: it cannot be captured into a graph");

    std::lock_guard<std::mutex> guard(w->mu);
    std::lock_guard<std::mutex> index_guard(idx->mu);   // (the mask table's pinned block is the index's)
    HIP_TRY(hipSetDevice(idx->device));
    // the request table: filled in the pinned block, one copy per call, an event behind it (stage_masks' rule)
    if (w->table_pending) { HIP_TRY(hipEventSynchronize(w->ev_table)); w->table_pending = false; }
    int *h_off = w->h_table, *h_npos = w->h_table + rc_table_npos(nr), *h_rows = w->h_table + rc_table_rows(nr);
    for (int64_t r = 0; r <= nr; ++r) h_off[r] = (int)example_off[r];
    for (int64_t r = 0; r < nr; ++r) h_npos[r] = n_positive[r];
    for (int64_t e = 0; e < ne; ++e) h_rows[e] = (int)example_rows[e];
    {
        const hipError_t ec = hipMemcpyAsync(w->table, w->h_table, rc_table_words(nr, ne) * sizeof(int), hipMemcpyHostToDevice, s);
        const hipError_t ee = hipEventRecord(w->ev_table, s);
        w->table_pending = ee == hipSuccess;
        if (ec != hipSuccess || ee != hipSuccess) {
            hipStreamSynchronize(s);
            w->table_pending = false;
            return fail(ICD_ERR_HIP, "request table: %s", hipGetErrorString(ec != hipSuccess ? ec : ee));
        }
    }
    const RecommendTable table{w->table, w->table + rc_table_npos(nr), w->table + rc_table_rows(nr)};
    const HostCall hc{s, inputs_on_device != 0, outputs_on_device != 0};
    const float *dv = nullptr;
    if (any_vector && (rc = hc.upload(example_vectors, w->v, (size_t)ne * idx->dim, &dv))) return rc;
    const float *dlo = lo, *dhi = hi;
    if ((lo || hi) && !bounds_on_device) {
        if (lo) { HIP_TRY(hipMemcpyAsync(w->lo, lo, (size_t)nr * sizeof(float), hipMemcpyHostToDevice, s)); dlo = w->lo; }
        if (hi) { HIP_TRY(hipMemcpyAsync(w->hi, hi, (size_t)nr * sizeof(float), hipMemcpyHostToDevice, s)); dhi = w->hi; }
    }
    if (any_mask && (rc = stage_masks(idx, masks, (int)nr, s))) return rc;
    const int width = first + k, tier = ws_tier(width);
    const bool average = strategy == ICD_RECOMMEND_AVERAGE_VECTOR;
    int *d_count = hc.target(out_count, w->o_count);
    long long *d_sel = hc.target(reinterpret_cast<long long *>(out_selected), w->o_sel);
    for (int64_t r0 = 0; r0 < nr;) {   // one block of whole requests at a time
        const int nb = (int)rc_cut(example_off, r0, nr, w->l.block, w->l.block_examples);
        if (nb < 1) return fail(ICD_ERR_STATE, "request %lld does not fit a block", (long long)r0);   // (rc_layout and the checks above make none)
        const int e0 = (int)example_off[r0];
        const int nv = average ? nb : (int)(example_off[r0 + nb] - e0);   // vectors of the block's E
        // step 1: the block's example vectors (or targets)
        RecommendExampleArgs x{};
        x.corpus = idx->corpus; x.vectors = dv; x.t = table; x.E = w->E; x.r0 = (int)r0; x.e0 = e0; x.dim = idx->dim; x.average = average ? 1 : 0;
        hipLaunchKernelGGL(recommend_examples_kernel, dim3((unsigned)nv), dim3(RC_EXAMPLE_THREADS), 0, s, x);
        HIP_TRY(hipGetLastError());
        w->last_vectors = nv;
        // step 2: their ordered scores on every row, as icd_index_search_wide launches the sweep - no mask, no bounds
        const RankOfPlan p = rk_plan(nv, idx->n, idx->num_cu);
        WideScoreArgs a{};
        a.corpus = idx->corpus; a.queries = w->E; a.mask = nullptr; a.lo = nullptr; a.hi = nullptr;
        a.S = w->SE; a.n_pad = w->l.n_pad; a.nq = nv; a.n = (int)idx->n; a.dim = idx->dim; a.chunks = p.chunks; a.rows_per_chunk = p.rows_per_chunk;
        HIP_TRY(launch_lds<wide_scores_kernel>(idx->device, rk_sweep_lds_bytes(), dim3((unsigned)p.grid), dim3(RK_THREADS), rk_sweep_lds_bytes(), s, a));
        // step 3: the fold - one ordered score per (request, row)
        RecommendCombineArgs c{};
        c.SE = w->SE; c.S = w->S; c.n_pad = w->l.n_pad; c.t = table; c.mask = any_mask ? idx->mask_dev + r0 : nullptr;
        c.lo = dlo ? dlo + r0 : nullptr; c.hi = dhi ? dhi + r0 : nullptr; c.r0 = (int)r0; c.e0 = e0; c.average = average ? 1 : 0;
        const dim3 cgrid((unsigned)rc_segments(w->l.n_pad), (unsigned)nb);
        if (strategy == ICD_RECOMMEND_SUM_SCORES) hipLaunchKernelGGL(recommend_combine_kernel<true>, cgrid, dim3(RC_COMBINE_THREADS), 0, s, c);
        else hipLaunchKernelGGL(recommend_combine_kernel<false>, cgrid, dim3(RC_COMBINE_THREADS), 0, s, c);
        HIP_TRY(hipGetLastError());
        // step 4: the wide search's select over S, unchanged: threshold, collect, sort and emit
        WideSelectArgs sel{};
        sel.S = w->S; sel.rec = w->rec; sel.C = w->C; sel.n_pad = w->l.n_pad; sel.width = width;
        hipLaunchKernelGGL(wide_threshold_kernel, dim3((unsigned)nb), dim3(WS_SELECT_THREADS), 0, s, sel);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(wide_collect_kernel, dim3((unsigned)nb), dim3(WS_SELECT_THREADS), 0, s, sel);
        HIP_TRY(hipGetLastError());
        const size_t o0 = hc.out_on_device ? (size_t)r0 * (size_t)k : 0;
        WideEmitArgs e{};
        e.C = w->C; e.rec = w->rec; e.levels = idx->levels;
        e.out_adj = reweighted ? hc.target(out_adj, w->o_adj) + o0 : nullptr;
        e.out_raw = hc.target(out_raw, w->o_raw) + o0;
        e.out_ids = hc.target(reinterpret_cast<long long *>(out_ids), w->o_ids) + o0;
        e.out_levels = hc.target(out_levels, w->o_lv) + o0;
        e.out_count = d_count + r0; e.out_selected = d_sel + r0;
        e.id_base = idx->id_base; e.width = width; e.first = first; e.k = k; e.reweighted = reweighted ? 1 : 0;
        HIP_TRY(launch_wide_sort_emit(idx->device, tier, (unsigned)nb, s, e));
        const size_t h0 = (size_t)r0 * (size_t)k;
        if ((rc = hc.copy_back({{reweighted ? out_adj + h0 : nullptr, w->o_adj, 8}, {out_raw + h0, w->o_raw, 4}, {out_ids + h0, w->o_ids, 8}, {out_levels + h0, w->o_lv, 4}},
                               (size_t)nb * (size_t)k))) return rc;
        r0 += nb;
    }
    if ((rc = hc.copy_back({{out_count, w->o_count, 4}, {out_selected, w->o_sel, 8}}, (size_t)nr))) return rc;
    return hc.finish();
}

}  // extern "C"
