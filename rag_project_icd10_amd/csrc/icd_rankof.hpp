// icd_rankof.hpp - rank-of search (icd_rankof_*, icd_index_rank_of). Part of icd_search.hip's translation unit
// (fail(), HIP_TRY, the owned-handle and host-call helpers, the mask checks and the mask table's staging); included there and
// nowhere else.
#pragma once

// A rank-of workspace belongs to the index it was created for but keeps no pointer into it: handle and identity are compared,
// never followed. A host caller's queries, the targets, their keys and every output are allocated here, never in a call.
struct icd_rankof : OwnedHandle {
    static constexpr uint32_t MAGIC = 0x1CD0AA4Fu;
    static constexpr const char *NOUN = "rank-of";
    int64_t max_nq = 0;
    float *q = nullptr;                                      // [max_nq][dim] a host caller's queries
    long long *targets = nullptr; u64 *tkey = nullptr;       // [max_nq][RK_MAX_TARGETS] the targets of a call and their keys, [nq][nt] used
    long long *o_rank = nullptr; double *o_adj = nullptr; float *o_raw = nullptr; int *o_lv = nullptr;   // [max_nq][RK_MAX_TARGETS] the outputs
    long long *o_sel = nullptr;                              // [max_nq]
    std::mutex mu;
};

extern "C" {

int icd_rankof_create(icd_index *idx, int64_t max_nq, icd_rankof **out) {
    static_assert(RK_MAX_TARGETS == ICD_RANKOF_MAX_TARGETS, "include/icd_search.h and rankof_plan.hpp disagree");
    if (!out) return fail(ICD_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!valid(idx)) return fail(ICD_ERR_STATE, "invalid handle");
    if (max_nq <= 0 || max_nq > 0x7FFFFFFFll / RK_MAX_TARGETS) return fail(ICD_ERR_INVALID, "max_nq=%lld", (long long)max_nq);
    if (idx->row_map) return fail(ICD_ERR_UNSUPPORTED, "a rank-of search on a view is not supported: mask the parent");
    if (idx->n >= 0x80000000ll) return fail(ICD_ERR_UNSUPPORTED, "a rank-of search needs fewer than 2^31 rows");
    HIP_TRY(hipSetDevice(idx->device));
    icd_rankof *w = new_handle<icd_rankof>(idx);
    if (!w) return fail(ICD_ERR_NOMEM, "host allocation failed");
    w->max_nq = max_nq;
    const RankOfLayout l = rk_layout(max_nq, idx->dim);
#define RK_TRY(expr) HIP_TRY_OR(free_handle(w), expr)
    RK_TRY(w->alloc(&w->q, l.q_floats));
    RK_TRY(w->alloc(&w->targets, l.slots)); RK_TRY(w->alloc(&w->tkey, l.slots));
    RK_TRY(w->alloc(&w->o_rank, l.slots)); RK_TRY(w->alloc(&w->o_adj, l.slots)); RK_TRY(w->alloc(&w->o_raw, l.slots)); RK_TRY(w->alloc(&w->o_lv, l.slots));
    RK_TRY(w->alloc(&w->o_sel, l.per_query));
#undef RK_TRY
    w->bytes = l.bytes;
    *out = w;
    return ICD_OK;
}

int icd_rankof_destroy(icd_rankof *ws) { return destroy_handle(ws); }

int icd_rankof_stats(icd_rankof *ws, int64_t *out_max_nq, int64_t *out_bytes) {
    if (!valid_handle(ws)) return fail(ICD_ERR_STATE, "invalid rank-of handle");
    if (out_max_nq) *out_max_nq = ws->max_nq;
    if (out_bytes) *out_bytes = (int64_t)ws->bytes;
    return ICD_OK;
}

int icd_index_rank_of(icd_index *idx, icd_rankof *ws, const float *queries, int64_t nq, int32_t queries_on_device,
                      const int64_t *targets, int32_t nt, icd_rowmask *const *masks, int64_t *out_rank, double *out_adj,
                      float *out_raw, int32_t *out_levels, int64_t *out_selected, void *stream) {
    // every check comes before the first device call
    if (!valid(idx)) return fail(ICD_ERR_STATE, "invalid handle");
    if (!valid_handle(ws)) return fail(ICD_ERR_STATE, "invalid rank-of handle");
    icd_rankof *w = ws;
    if (idx->row_map) return fail(ICD_ERR_UNSUPPORTED, "a rank-of search on a view is not supported: mask the parent");
    int rc = check_owner(w->at, idx, "the rank-of handle");
    if (rc) return rc;
    if (nt < 1 || nt > ICD_RANKOF_MAX_TARGETS) return fail(ICD_ERR_INVALID, "nt=%d: a rank-of search takes 1 .. %d targets per query", nt, ICD_RANKOF_MAX_TARGETS);
    if (nq < 0) return fail(ICD_ERR_INVALID, "nq=%lld", (long long)nq);
    if (nq > w->max_nq) return fail(ICD_ERR_INVALID, "nq=%lld exceeds the rank-of handle's max_nq=%lld", (long long)nq, (long long)w->max_nq);
    if (!out_rank) return fail(ICD_ERR_INVALID, "out_rank is NULL");
    bool any_mask = false;
    if (masks && (rc = check_masks(idx, masks, nq, "masked rank-of search", &any_mask))) return rc;
    if (nq == 0) return ICD_OK;
    if (!queries || !targets) return fail(ICD_ERR_INVALID, "queries or targets is NULL");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (stream_capturing(s)) return fail(ICD_ERR_INVALID, "a rank-of search returns host outputs and synchronises: it cannot be captured into a graph");
    std::lock_guard<std::mutex> guard(w->mu);
    std::lock_guard<std::mutex> index_guard(idx->mu);   // (the mask table's pinned block is the index's)
    HIP_TRY(hipSetDevice(idx->device));
    const HostCall hc{s, queries_on_device != 0, false};
    const float *dq = nullptr;
    if ((rc = hc.upload(queries, w->q, (size_t)nq * idx->dim, &dq))) return rc;
    const size_t slots = (size_t)nq * (size_t)nt;
    HIP_TRY(hipMemcpyAsync(w->targets, targets, slots * sizeof(long long), hipMemcpyHostToDevice, s));
    if (any_mask && (rc = stage_masks(idx, masks, (int)nq, s))) return rc;
    // step 1: the targets' scores and keys, the presets of the outputs
    RankOfTargetArgs t{};
    t.corpus = idx->corpus; t.queries = dq; t.targets = w->targets; t.levels = idx->levels; t.mask = any_mask ? idx->mask_dev : nullptr;
    t.tkey = w->tkey; t.rank = w->o_rank; t.adj = w->o_adj; t.raw = w->o_raw; t.out_levels = w->o_lv; t.selected = w->o_sel;
    t.n = idx->n; t.id_base = idx->id_base; t.dim = idx->dim; t.nq = (int)nq; t.nt = nt;
    hipLaunchKernelGGL(rankof_targets_kernel, dim3((unsigned)rk_target_blocks(nq, nt)), dim3(RK_TARGET_THREADS), 0, s, t);
    HIP_TRY(hipGetLastError());
    // step 2: the counting sweep
    const RankOfPlan p = rk_plan(nq, idx->n, idx->num_cu);
    RankOfSweepArgs a{};
    a.corpus = idx->corpus; a.queries = dq; a.mask = t.mask; a.tkey = w->tkey; a.rank = w->o_rank; a.selected = w->o_sel;
    a.nq = (int)nq; a.nt = nt; a.n = (int)idx->n; a.dim = idx->dim; a.chunks = p.chunks; a.rows_per_chunk = p.rows_per_chunk;
    hipLaunchKernelGGL(rankof_sweep_kernel, dim3((unsigned)p.grid), dim3(RK_THREADS), rk_sweep_lds_bytes(), s, a);
    HIP_TRY(hipGetLastError());
    if ((rc = hc.copy_back({{out_rank, w->o_rank, 8}, {out_adj, w->o_adj, 8}, {out_raw, w->o_raw, 4}, {out_levels, w->o_lv, 4}}, slots))) return rc;
    if ((rc = hc.copy_back({{out_selected, w->o_sel, 8}}, (size_t)nq))) return rc;
    return hc.finish();
}

}  // extern "C"
