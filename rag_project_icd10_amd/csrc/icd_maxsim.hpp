// icd_maxsim.hpp - the embedding-list search (icd_grouping_prepare_maxsim, icd_index_search_maxsim). Part of
// icd_search.hip's translation unit, behind icd_grouped.hpp whose handle, scoring pass and best-row pass it uses; included there
// and nowhere else.
#pragma once

extern "C" {

int icd_grouping_prepare_maxsim(icd_index *idx, icd_grouping *grouping, int64_t max_lists, int64_t max_vectors) {
    if (!valid(idx)) return fail(ICD_ERR_STATE, "invalid handle");
    if (!valid_handle(grouping)) return fail(ICD_ERR_STATE, "invalid grouping handle");
    if (const int rc = check_owner(grouping->at, idx, "the grouping")) return rc;
    if (max_lists < 1 || max_vectors < max_lists || max_vectors > 0x7FFFFFFFll / ICD_MAX_K)
        return fail(ICD_ERR_INVALID, "max_lists=%lld max_vectors=%lld: need 1 <= max_lists <= max_vectors", (long long)max_lists, (long long)max_vectors);
    std::lock_guard<std::mutex> guard(grouping->mu);
    icd_grouping *g = grouping;
    if (g->ms_lists > 0) {
        if (max_lists <= g->ms_lists && max_vectors <= g->ms_vectors) return ICD_OK;
        return fail(ICD_ERR_INVALID, "the grouping is prepared for %lld lists of %lld vectors: it is not prepared again for more",
                    (long long)g->ms_lists, (long long)g->ms_vectors);
    }
    HIP_TRY(hipSetDevice(idx->device));
    const size_t cells = (size_t)std::min<int64_t>(max_lists, g->qb) * g->G;   // a pass holds at most qb lists (of one vector each)
    const size_t nq = (size_t)max_vectors * idx->dim, ng = (size_t)max_lists * ICD_MAX_K, nm = (size_t)max_vectors * ICD_MAX_K;
    // the blocks join the handle's allocations only once all of them are there: a failure leaves nothing behind
    u64 *agg = nullptr; float *q = nullptr, *gs = nullptr, *ms = nullptr; int *gi = nullptr, *ml = nullptr; long long *mi = nullptr;
    hipError_t e = dmalloc(&agg, cells);
    if (e == hipSuccess) e = dmalloc(&q, nq);
    if (e == hipSuccess) e = dmalloc(&gs, ng);
    if (e == hipSuccess) e = dmalloc(&gi, ng);
    if (e == hipSuccess) e = dmalloc(&ms, nm);
    if (e == hipSuccess) e = dmalloc(&mi, nm);
    if (e == hipSuccess) e = dmalloc(&ml, nm);
    if (e != hipSuccess) {
        hipFree(agg); hipFree(q); hipFree(gs); hipFree(gi); hipFree(ms); hipFree(mi); hipFree(ml);
        return fail(ICD_ERR_HIP, "preparing a grouping for the embedding-list search: %s", hipGetErrorString(e));
    }
    for (void *p : {(void *)agg, (void *)q, (void *)gs, (void *)gi, (void *)ms, (void *)mi, (void *)ml}) g->allocs.push_back(p);
    g->ms_agg = agg; g->ms_q = q; g->ms_gscore = gs; g->ms_gid = gi; g->ms_mscore = ms; g->ms_mid = mi; g->ms_mlv = ml;
    g->bytes += cells * 8 + nq * 4 + ng * 8 + nm * 16;
    g->ms_lists = max_lists; g->ms_vectors = max_vectors;
    return ICD_OK;
}

int icd_index_search_maxsim(icd_index *idx, icd_grouping *grouping, const float *queries, const int64_t *list_off, int64_t nl, int32_t k,
                            int32_t scorer, int32_t queries_on_device, float *out_group_scores, int32_t *out_group_ids,
                            float *out_match_scores, int64_t *out_match_ids, int32_t *out_match_levels, int32_t out_on_device,
                            void *stream) {
    if (!valid(idx)) return fail(ICD_ERR_STATE, "invalid handle");
    if (!valid_handle(grouping)) return fail(ICD_ERR_STATE, "invalid grouping handle");
    icd_grouping *g = grouping;
    if (const int rc = check_owner(g->at, idx, "the grouping")) return rc;
    if (scorer != ICD_MAXSIM_SUM && scorer != ICD_MAXSIM_MEAN) return fail(ICD_ERR_INVALID, "scorer=%d: ICD_MAXSIM_SUM or ICD_MAXSIM_MEAN", scorer);
    if (k < 1 || k > ICD_MAX_K) return fail(ICD_ERR_INVALID, "k=%d: need 1 <= k <= %d", k, ICD_MAX_K);
    if (nl < 0) return fail(ICD_ERR_INVALID, "nl=%lld", (long long)nl);
    if (!out_group_scores || !out_group_ids) return fail(ICD_ERR_INVALID, "output pointer is NULL");
    if (nl == 0) return ICD_OK;
    if (!list_off || !queries) return fail(ICD_ERR_INVALID, "%s is NULL", list_off ? "queries" : "list_off");
    if (list_off[0] != 0) return fail(ICD_ERR_INVALID, "list_off[0]=%lld: the offsets start at 0", (long long)list_off[0]);
    for (int64_t l = 0; l < nl; ++l) {
        const int64_t t = list_off[l + 1] - list_off[l];
        if (t < 1 || t > ICD_MAXSIM_MAX_T)
            return fail(ICD_ERR_INVALID, "list %lld holds %lld vectors: need 1 .. %d (list_off is non-decreasing)", (long long)l, (long long)t, ICD_MAXSIM_MAX_T);
    }
    const int64_t nv = list_off[nl];
    std::lock_guard<std::mutex> guard(g->mu);
    if (g->ms_lists == 0) return fail(ICD_ERR_STATE, "the grouping was never prepared for the embedding-list search (icd_grouping_prepare_maxsim)");
    if (nl > g->ms_lists || nv > g->ms_vectors)
        return fail(ICD_ERR_INVALID, "%lld lists of %lld vectors exceed the grouping's preparation (%lld lists, %lld vectors)", (long long)nl,
                    (long long)nv, (long long)g->ms_lists, (long long)g->ms_vectors);
    std::vector<MaxsimPass> passes;
    if (!maxsim_plan(list_off, nl, g->qb, passes)) return fail(ICD_ERR_INVALID, "list_off: no plan");   // (checked above: not reached)
    HIP_TRY(hipSetDevice(idx->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const HostCall hc{s, queries_on_device != 0, out_on_device != 0};
    int rc = check_capture(s, !queries_on_device || !out_on_device, false, false);
    if (rc) return rc;
    const float *dq;
    if ((rc = hc.upload(queries, g->ms_q, (size_t)nv * idx->dim, &dq))) return rc;
    float *d_gs = hc.target(out_group_scores, g->ms_gscore);
    int *d_gi = hc.target(out_group_ids, g->ms_gid);
    float *d_ms = hc.target(out_match_scores, g->ms_mscore);
    long long *d_mi = hc.target(reinterpret_cast<long long *>(out_match_ids), g->ms_mid);
    int *d_ml = hc.target(out_match_levels, g->ms_mlv);

    for (const MaxsimPass &p : passes) {
        if ((rc = grouped_scores_pass(idx, g, dq + (size_t)p.v0 * idx->dim, p.nv, s))) return rc;
        if ((rc = grouped_best_pass(g, p.nv, s))) return rc;
        for (int i = 0; i < p.launches(); ++i) {
            MaxsimReduceArgs ra{};
            ra.best = g->best; ra.agg = g->ms_agg; ra.G = g->G; ra.mean = scorer == ICD_MAXSIM_MEAN ? 1 : 0; ra.lists = p.launch(i);
            hipLaunchKernelGGL(maxsim_reduce_kernel, dim3((unsigned)((g->G + 255) / 256), (unsigned)ra.lists.n), dim3(256), 0, s, ra);
            HIP_TRY(hipGetLastError());
            MaxsimFinishArgs fa{};
            fa.agg = g->ms_agg; fa.best = g->best; fa.dense_of = g->dense_of; fa.groups = g->group_of;
            fa.levels = idx->levels; fa.row_map = idx->row_map; fa.id_base = idx->id_base;
            fa.G = g->G; fa.k = k; fa.v_base = p.v0; fa.l_base = p.l0; fa.lists = ra.lists;
            fa.out_group_scores = d_gs; fa.out_group_ids = d_gi;
            fa.out_match_scores = d_ms; fa.out_match_ids = d_mi; fa.out_match_levels = d_ml;
            const dim3 grid((unsigned)((ra.lists.n + 3) / 4));
            if (k <= 16) hipLaunchKernelGGL((maxsim_finish_kernel<16, 2>), grid, dim3(256), 0, s, fa);
            else hipLaunchKernelGGL((maxsim_finish_kernel<128, 4>), grid, dim3(256), 0, s, fa);
            HIP_TRY(hipGetLastError());
        }
    }
    if ((rc = hc.copy_back({{out_group_scores, d_gs, 4}, {out_group_ids, d_gi, 4}}, (size_t)nl * k))) return rc;
    if ((rc = hc.copy_back({{out_match_scores, d_ms, 4}, {out_match_ids, d_mi, 8}, {out_match_levels, d_ml, 4}}, (size_t)nv * k))) return rc;
    return hc.finish();
}

}  // extern "C"
