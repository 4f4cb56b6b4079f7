// icd_text_match.hpp - keyword match filters (icd_sparse_match_rowmasks): the row masks of a batch of
// TEXT_MATCH predicates, built from a sparse index's postings by text_match_mask_kernel. The shared checks, the masks' block and
// its undo / publish are ProducedMasks' (icd_range_mask.hpp); here are the entry's own handle and input checks, what it stages
// and its launch. Part of icd_search.hip's translation unit; included there and nowhere else.
#pragma once

extern "C" {

// Behind the block's base pointers, for what arrives from the host: [nq + 1] offsets, [nq] min_match and the terms.
int icd_sparse_match_rowmasks(icd_index *idx, icd_sparse *sp, const int64_t *q_off, const uint32_t *q_terms, const int32_t *min_match,
                              int64_t nq, int32_t queries_on_device, icd_rowmask *const *base_masks, icd_rowmask **out_masks, void *stream) {
    int rc = produced_check_index(idx, nq, out_masks);
    if (rc) return rc;
    if (!valid_handle(sp)) return fail(ICD_ERR_STATE, "invalid sparse index handle");
    if ((rc = check_owner(sp->at, idx, "the sparse index"))) return rc;
    int64_t tiles = 0;
    bool any_base = false;
    if ((rc = produced_check_batch(idx, nq, base_masks, &tiles, &any_base))) return rc;
    if (nq == 0) return ICD_OK;
    if (!q_off || !min_match) return fail(ICD_ERR_INVALID, "q_off / min_match NULL");
    int64_t q_nnz = 0;
    if (!queries_on_device) {
        char msg[200];
        if (sparse_check_match_queries(q_off, q_terms, min_match, nq, sp->vocab, SP_MAX_TERMS, msg, sizeof msg)) return fail(ICD_ERR_INVALID, "%s", msg);
        q_nnz = q_off[nq];
    } else if (!q_terms) {
        return fail(ICD_ERR_INVALID, "q_terms NULL");
    }
    const size_t staged[3] = {queries_on_device ? 0 : ((size_t)nq + 1) * 8, queries_on_device ? 0 : (size_t)nq * 4, (size_t)q_nnz * 4};
    ProducedMasks pm;
    if ((rc = pm.begin("icd_sparse_match_rowmasks", idx, nq, base_masks, any_base, out_masks, staged, 3, stream))) return rc;

    TextMatchArgs a{};
    a.post_off = sp->post_off; a.post_row = sp->post_row; a.vocab = sp->vocab;
    a.q_off = reinterpret_cast<const long long *>(q_off); a.q_terms = q_terms; a.min_match = min_match;
    if (!queries_on_device) {
        long long *d_off = pm.region<long long>(pm.at.staged[0]);
        int *d_mm = pm.region<int>(pm.at.staged[1]);
        uint32_t *d_terms = pm.region<uint32_t>(pm.at.staged[2]);
        PM_TRY(pm, hipMemcpyAsync(d_off, q_off, staged[0], hipMemcpyHostToDevice, pm.s));
        PM_TRY(pm, hipMemcpyAsync(d_mm, min_match, staged[1], hipMemcpyHostToDevice, pm.s));
        if (q_nnz) PM_TRY(pm, hipMemcpyAsync(d_terms, q_terms, staged[2], hipMemcpyHostToDevice, pm.s));
        a.q_off = d_off; a.q_terms = d_terms; a.min_match = d_mm;
    }
    pm.fill(&a, idx, tiles);
    hipLaunchKernelGGL(text_match_mask_kernel, dim3((unsigned)(nq * tiles)), dim3(SP_THREADS), 0, pm.s, a);
    PM_TRY(pm, hipGetLastError());
    // what came from host memory was staged from pageable buffers: the call returns once the stream has taken them
    if (!queries_on_device || any_base) PM_TRY(pm, hipStreamSynchronize(pm.s));
    pm.publish();
    return ICD_OK;
}

}  // extern "C"
