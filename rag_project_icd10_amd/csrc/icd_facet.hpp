// icd_facet.hpp - facet counts over a batch of row masks (icd_rowmask_group_counts; facet_count_kernel.hpp).
// Part of icd_search.hip's translation unit (fail(), HIP_TRY, the owned-handle helpers, check_masks and stage_select of
// icd_range_mask.hpp, the grouping of icd_grouped.hpp); included there and nowhere else.
#pragma once

// One launch for the queries q0 .. q0 + nb of the staged mask table into `counts` ([nb][G], zeroed here on the stream).
static int facet_count_pass(icd_index *idx, icd_grouping *g, int64_t q0, int64_t nb, int *counts, hipStream_t s) {
    HIP_TRY(hipMemsetAsync(counts, 0, (size_t)nb * (size_t)g->G * sizeof(int), s));
    FacetCountArgs a{};
    a.masks = idx->mask_dev + q0; a.dense_of = g->dense_of; a.counts = counts;
    a.n = idx->n; a.mask_words = rowmask_tile_words(idx->n); a.segments = (int)ms_segments(idx->n); a.G = g->G;
    const dim3 grid((unsigned)(nb * a.segments));
    if (fc_lds_form(g->G)) hipLaunchKernelGGL(facet_count_kernel<true>, grid, dim3(MS_THREADS), 0, s, a);
    else hipLaunchKernelGGL(facet_count_kernel<false>, grid, dim3(MS_THREADS), 0, s, a);
    HIP_TRY(hipGetLastError());
    return ICD_OK;
}

extern "C" {

int icd_rowmask_group_counts(icd_index *idx, icd_grouping *grouping, icd_rowmask *const *masks, int64_t nq, int32_t *out_counts,
                             int32_t out_on_device, void *stream) {
    if (nq < 0) return fail(ICD_ERR_INVALID, "nq=%lld", (long long)nq);
    if (nq > 0 && !masks) return fail(ICD_ERR_INVALID, "masks is NULL");
    if (nq > 0 && !out_counts) return fail(ICD_ERR_INVALID, "out_counts is NULL");
    if (!valid(idx)) return fail(ICD_ERR_STATE, "invalid handle");
    if (!valid_handle(grouping)) return fail(ICD_ERR_STATE, "invalid grouping handle");
    bool any = false;
    if (const int rc = check_masks(idx, masks, nq, "facet count", &any)) return rc;
    icd_grouping *g = grouping;
    if (g->on_view) return fail(ICD_ERR_UNSUPPORTED, "facet counts with a grouping of a view are not supported: group and mask the parent");
    if (const int rc = check_owner(g->at, idx, "the grouping")) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (stream_capturing(s)) return fail(ICD_ERR_INVALID, "a facet count stages its mask table on the host at call time: it cannot be captured into a graph");
    if (nq == 0) return ICD_OK;
    const bool host = !out_on_device;
    // device outputs take every query's counts themselves; host outputs go through the grouping's `best` block, idle outside a search
    const long long segments = ms_segments(idx->n);
    const long long per_block = host ? fc_block_queries((long long)g->qb * g->G * (long long)sizeof(u64), g->G) : -1;
    const long long per = fc_pass_queries(nq, per_block, segments);
    if (fc_passes(nq, per) < 0) return fail(ICD_ERR_INVALID, "n=%lld: %lld segments of rows exceed 2^31 - 1 work-groups", (long long)idx->n, segments);
    std::lock_guard<std::mutex> guard_g(g->mu);
    std::lock_guard<std::mutex> guard(idx->mu);
    HIP_TRY(hipSetDevice(idx->device));
    if (const int rc = stage_select(idx, masks, nullptr, (int)nq, s)) return rc;
    for (int64_t q0 = 0; q0 < nq; q0 += per) {
        const int64_t nb = std::min<int64_t>(per, nq - q0);
        int *counts = host ? reinterpret_cast<int *>(g->best) : out_counts + (size_t)q0 * g->G;
        if (const int rc = facet_count_pass(idx, g, q0, nb, counts, s)) return rc;
        if (host) HIP_TRY(hipMemcpyAsync(out_counts + (size_t)q0 * g->G, counts, (size_t)nb * g->G * sizeof(int), hipMemcpyDeviceToHost, s));
    }
    if (host) HIP_TRY(hipStreamSynchronize(s));
    return ICD_OK;
}

}  // extern "C"
