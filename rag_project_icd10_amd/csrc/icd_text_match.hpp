// icd_text_match.hpp - keyword match filters (icd_sparse_match_rowmasks): the row masks of a batch of
// TEXT_MATCH predicates, built from a sparse index's postings by text_match_mask_kernel. Part of icd_search.hip's translation unit
// (fail(), HIP_TRY, the owned-handle and mask helpers, icd_sparse); included there and nowhere else.
#pragma once

extern "C" {

// ONE allocation holds what the call's nq masks and its kernel need: [nq][words] bitsets (tile words + the zero tail), [nq] row
// counters, and - for what arrives from the host - [nq] base pointers, [nq] min_match, [nq + 1] offsets and the terms. Every mask
// is an ordinary icd_rowmask that points into it; the block goes with the last of them (icd_rowmask_destroy).
int icd_sparse_match_rowmasks(icd_index *idx, icd_sparse *sp, const int64_t *q_off, const uint32_t *q_terms, const int32_t *min_match,
                              int64_t nq, int32_t queries_on_device, icd_rowmask *const *base_masks, icd_rowmask **out_masks, void *stream) {
    if (!out_masks) return fail(ICD_ERR_INVALID, "out_masks is NULL");
    if (nq < 0) return fail(ICD_ERR_INVALID, "nq=%lld", (long long)nq);
    for (int64_t q = 0; q < nq; ++q) out_masks[q] = nullptr;
    // every check comes before the first device call
    if (!valid(idx)) return fail(ICD_ERR_STATE, "invalid handle");
    if (idx->row_map) return fail(ICD_ERR_UNSUPPORTED, "row masks on a view are not supported: mask the parent");
    if (!valid_handle(sp)) return fail(ICD_ERR_STATE, "invalid sparse index handle");
    int rc = check_owner(sp->at, idx, "the sparse index");
    if (rc) return rc;
    if (nq * sp->tiles > 0x7FFFFFFFll) return fail(ICD_ERR_INVALID, "nq=%lld: %d tiles of rows times nq exceed 2^31 - 1 work-groups", (long long)nq, sp->tiles);
    bool any_base = false;
    if (base_masks)
        for (int64_t q = 0; q < nq; ++q) {   // (check_masks' rules without its bound on the table's length: no search table is filled here)
            const icd_rowmask *m = base_masks[q];
            if (!m) continue;
            any_base = true;
            if (!valid_handle(m)) return fail(ICD_ERR_STATE, "base_masks[%lld]: invalid row mask handle", (long long)q);
            if ((rc = check_owner(m->at, idx, "base_masks", (long long)q))) return rc;
        }
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
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (stream_capturing(s)) return fail(ICD_ERR_INVALID, "icd_sparse_match_rowmasks allocates: it cannot be captured into a graph");
    HIP_TRY(hipSetDevice(idx->device));

    const size_t words = (size_t)rowmask_tile_words(idx->n) + ROWMASK_TAIL_WORDS;   // (a multiple of 4: every bitset starts 16-byte aligned)
    const size_t b_bits = (size_t)nq * words * 4, b_cnt = (((size_t)nq * 4) + 15) / 16 * 16;
    const size_t b_base = any_base ? (size_t)nq * 8 : 0;
    const size_t b_off = queries_on_device ? 0 : ((size_t)nq + 1) * 8;
    const size_t b_mm = queries_on_device ? 0 : b_cnt, b_terms = queries_on_device ? 0 : (size_t)q_nnz * 4;
    std::vector<icd_rowmask *> made;
    std::vector<const uint32_t *> h_base;
    icd_rowmask::SharedBlock *blk = new (std::nothrow) icd_rowmask::SharedBlock();
    try {
        made.reserve((size_t)nq);
        if (any_base) h_base.resize((size_t)nq);
    } catch (const std::bad_alloc &) {
        delete blk;
        blk = nullptr;
    }
    if (!blk) return fail(ICD_ERR_NOMEM, "host allocation failed");
    char *dev = nullptr;
    // (undo: every handle made so far, then the block - the stream is drained first, a launch may be reading it)
    auto undo = [&]() {
        hipStreamSynchronize(s);
        for (icd_rowmask *m : made) free_handle(m);
        for (int64_t q = 0; q < nq; ++q) out_masks[q] = nullptr;
        hipFree(dev);
        delete blk;
    };
#define TM_TRY(expr) HIP_TRY_OR(undo(), expr)
    TM_TRY(hipMalloc(reinterpret_cast<void **>(&dev), b_bits + b_cnt + b_base + b_off + b_mm + b_terms));
    blk->dev = dev;
    uint32_t *d_bits = reinterpret_cast<uint32_t *>(dev);
    int *d_cnt = reinterpret_cast<int *>(dev + b_bits);
    const uint32_t **d_base = reinterpret_cast<const uint32_t **>(dev + b_bits + b_cnt);
    long long *d_off = reinterpret_cast<long long *>(dev + b_bits + b_cnt + b_base);
    int *d_mm = reinterpret_cast<int *>(dev + b_bits + b_cnt + b_base + b_off);
    uint32_t *d_terms = reinterpret_cast<uint32_t *>(dev + b_bits + b_cnt + b_base + b_off + b_mm);
    for (int64_t q = 0; q < nq; ++q) {
        icd_rowmask *m = new_handle<icd_rowmask>(idx);
        if (!m) { undo(); return fail(ICD_ERR_NOMEM, "host allocation failed"); }
        m->rows = -1; m->bytes = words * sizeof(uint32_t) + sizeof(int);
        m->bits = d_bits + (size_t)q * words; m->count_dev = d_cnt + q; m->block = blk;
        made.push_back(m);
    }
    TM_TRY(hipMemsetAsync(dev, 0, b_bits + b_cnt, s));   // (the tails, the words of tiles the kernel leaves alone, the counters)
    TextMatchArgs a{};
    a.post_off = sp->post_off; a.post_row = sp->post_row; a.vocab = sp->vocab;
    a.q_off = reinterpret_cast<const long long *>(q_off); a.q_terms = q_terms; a.min_match = min_match;
    if (!queries_on_device) {
        TM_TRY(hipMemcpyAsync(d_off, q_off, ((size_t)nq + 1) * 8, hipMemcpyHostToDevice, s));
        TM_TRY(hipMemcpyAsync(d_mm, min_match, (size_t)nq * 4, hipMemcpyHostToDevice, s));
        if (q_nnz) TM_TRY(hipMemcpyAsync(d_terms, q_terms, (size_t)q_nnz * 4, hipMemcpyHostToDevice, s));
        a.q_off = d_off; a.q_terms = d_terms; a.min_match = d_mm;
    }
    if (any_base) {
        for (int64_t q = 0; q < nq; ++q) h_base[(size_t)q] = base_masks[q] ? base_masks[q]->bits : nullptr;
        TM_TRY(hipMemcpyAsync(d_base, h_base.data(), (size_t)nq * 8, hipMemcpyHostToDevice, s));
        a.base = d_base;
    }
    a.bits = d_bits; a.stride = (long long)words; a.count = d_cnt;
    a.n = idx->n; a.mask_words = rowmask_tile_words(idx->n); a.tiles = sp->tiles;
    hipLaunchKernelGGL(text_match_mask_kernel, dim3((unsigned)(nq * sp->tiles)), dim3(SP_THREADS), 0, s, a);
    TM_TRY(hipGetLastError());
    // what came from host memory was staged from pageable buffers: the call returns once the stream has taken them
    if (!queries_on_device || any_base) TM_TRY(hipStreamSynchronize(s));
#undef TM_TRY
    blk->refs.store((int)nq);
    for (int64_t q = 0; q < nq; ++q) out_masks[q] = made[(size_t)q];
    return ICD_OK;
}

}  // extern "C"
