// icd_sparse.hpp - the sparse-vector search (icd_sparse_*) and its grouped form (icd_grouping_pair_sparse, icd_sparse_search_grouped).
// Part of icd_search.hip's translation unit (fail(), HIP_TRY, the owned-handle, mask and host-call helpers, the grouping); included
// there and nowhere else.
#pragma once
#include "sparse_pack.hpp"

// ---- sparse search (sparse_kernel.hpp) ------------------------------------------------------------------
// A sparse index belongs to the index it was created for but keeps no pointer into it: handle and identity are compared, never
// followed. Postings, the staging of a host caller's queries and outputs, the tiles' partial lists and the bands of a range
// search (max_nq BandQ on the device, and a pinned host block host bounds are packed in) are allocated
// here, never in a search.
struct icd_sparse : OwnedHandle {
    static constexpr uint32_t MAGIC = 0x1CD5BA25u;
    static constexpr const char *NOUN = "sparse index";
    int64_t vocab = 0, nnz = 0;
    int tiles = 0, max_nq = 0, max_k = 0;
    long long *post_off = nullptr; uint32_t *post_row = nullptr; float *post_val = nullptr;   // [vocab + 1], [nnz], [nnz]
    long long *q_off = nullptr; uint32_t *q_terms = nullptr; float *q_vals = nullptr;         // a host caller's queries: [max_nq + 1], [max_nq][64] each
    icd::u64 *part = nullptr;                                                                  // [tiles][max_nq][max_k] keys, best first
    double *o_adj = nullptr; float *o_raw = nullptr; long long *o_ids = nullptr; int *o_lv = nullptr;   // [max_nq][max_k] a host caller's outputs
    BandQ *band_dev = nullptr, *h_band = nullptr;                                              // [max_nq] each; h_band pinned host memory
    std::mutex mu;
};

static_assert(ICD_SPARSE_MAX_QUERY_TERMS == SP_MAX_TERMS, "ICD_SPARSE_MAX_QUERY_TERMS and sparse_kernel.hpp disagree");

extern "C" {

int icd_sparse_tile_rows(void) { return SP_TILE; }

int icd_sparse_pack(const int64_t *row_off, const uint32_t *terms, const float *vals, int64_t n, int64_t vocab, int64_t *post_off,
                    uint32_t *post_row, float *post_val) {
    char msg[200];
    if (sparse_pack_rows(row_off, terms, vals, n, vocab, post_off, post_row, post_val, msg, sizeof msg)) return fail(ICD_ERR_INVALID, "%s", msg);
    return ICD_OK;
}

int icd_sparse_create(icd_index *idx, const int64_t *row_off, const uint32_t *terms, const float *vals, int64_t vocab, int32_t max_nq,
                      int32_t max_k, icd_sparse **out) {
    if (!out) return fail(ICD_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!valid(idx)) return fail(ICD_ERR_STATE, "invalid handle");
    if (idx->row_map) return fail(ICD_ERR_UNSUPPORTED, "a sparse index on a view is not supported: build it on the parent and mask");
    if (idx->n > 0x7FFFFFFFll) return fail(ICD_ERR_UNSUPPORTED, "n=%lld: a sparse index addresses rows with 31 bits (n < 2^31)", (long long)idx->n);
    if (max_nq < 1 || max_k < 1 || max_k > ICD_MAX_K) return fail(ICD_ERR_INVALID, "max_nq=%d max_k=%d (max_k in 1 .. %d)", max_nq, max_k, ICD_MAX_K);
    const int64_t tiles = (idx->n + SP_TILE - 1) / SP_TILE;
    if (tiles * max_nq > 0x7FFFFFFFll) return fail(ICD_ERR_INVALID, "max_nq=%d: %lld tiles of rows times max_nq exceed 2^31 - 1 work-groups", max_nq, (long long)tiles);
    char msg[200];
    if (sparse_check_rows(row_off, terms, vals, idx->n, vocab, msg, sizeof msg)) return fail(ICD_ERR_INVALID, "%s", msg);   // (the one pass over the rows' rules)
    const int64_t nnz = row_off[idx->n];
    std::vector<int64_t> h_off;
    std::vector<uint32_t> h_row;
    std::vector<float> h_val;
    try {
        h_off.resize((size_t)vocab + 1); h_row.resize((size_t)nnz); h_val.resize((size_t)nnz);
    } catch (const std::bad_alloc &) {
        return fail(ICD_ERR_NOMEM, "host allocation failed");
    }
    sparse_pack_checked(row_off, terms, vals, idx->n, vocab, h_off.data(), h_row.data(), h_val.data());
    HIP_TRY(hipSetDevice(idx->device));
    icd_sparse *sp = new_handle<icd_sparse>(idx);
    if (!sp) return fail(ICD_ERR_NOMEM, "host allocation failed");
    sp->vocab = vocab; sp->nnz = nnz; sp->tiles = (int)tiles; sp->max_nq = max_nq; sp->max_k = max_k;
    const size_t nt = (size_t)max_nq * SP_MAX_TERMS, no = (size_t)max_nq * max_k, np_ = (size_t)tiles * no;
#define SP_TRY(expr) HIP_TRY_OR(free_handle(sp), expr)
    SP_TRY(sp->alloc(&sp->post_off, (size_t)vocab + 1)); SP_TRY(sp->alloc(&sp->post_row, (size_t)nnz)); SP_TRY(sp->alloc(&sp->post_val, (size_t)nnz));
    SP_TRY(sp->alloc(&sp->q_off, (size_t)max_nq + 1)); SP_TRY(sp->alloc(&sp->q_terms, nt)); SP_TRY(sp->alloc(&sp->q_vals, nt));
    SP_TRY(sp->alloc(&sp->part, np_));
    SP_TRY(sp->alloc(&sp->o_adj, no)); SP_TRY(sp->alloc(&sp->o_raw, no)); SP_TRY(sp->alloc(&sp->o_ids, no)); SP_TRY(sp->alloc(&sp->o_lv, no));
    SP_TRY(sp->alloc(&sp->band_dev, (size_t)max_nq));
    SP_TRY(hipHostMalloc(reinterpret_cast<void **>(&sp->h_band), (size_t)max_nq * sizeof(BandQ), hipHostMallocDefault));
    sp->pinned.push_back(sp->h_band);
    SP_TRY(hipMemcpy(sp->post_off, h_off.data(), ((size_t)vocab + 1) * 8, hipMemcpyHostToDevice));
    if (nnz) {
        SP_TRY(hipMemcpy(sp->post_row, h_row.data(), (size_t)nnz * 4, hipMemcpyHostToDevice));
        SP_TRY(hipMemcpy(sp->post_val, h_val.data(), (size_t)nnz * 4, hipMemcpyHostToDevice));
    }
#undef SP_TRY
    sp->bytes = ((size_t)vocab + 1) * 8 + (size_t)nnz * 8 + ((size_t)max_nq + 1) * 8 + nt * 8 + np_ * 8 + no * (8 + 4 + 8 + 4) +
                (size_t)max_nq * sizeof(BandQ);
    *out = sp;
    return ICD_OK;
}

int icd_sparse_destroy(icd_sparse *sp) { return destroy_handle(sp); }

int icd_sparse_stats(icd_sparse *sp, int64_t *out_vocab, int64_t *out_nnz, int64_t *out_bytes) {
    if (!valid_handle(sp)) return fail(ICD_ERR_STATE, "invalid sparse index handle");
    if (out_vocab) *out_vocab = sp->vocab;
    if (out_nnz) *out_nnz = sp->nnz;
    if (out_bytes) *out_bytes = (int64_t)sp->bytes;
    return ICD_OK;
}

}  // extern "C"

// A caller's queries (CSR; host or device memory) and what icd_sparse_search, icd_sparse_search_range and icd_sparse_search_grouped do
// with them on either side of their locks.
struct SparseQueries {
    const int64_t *off; const uint32_t *terms; const float *vals;
    int64_t nq; bool on_device;
    int64_t nnz = 0;   // of a host caller's queries, measured by check()

    // before the first device call: a host caller's CSR against the sparse index's vocabulary, a device caller's pointers against NULL
    int check(const icd_sparse *sp) {
        if (!off) return fail(ICD_ERR_INVALID, "q_off is NULL");
        if (!on_device) {
            char msg[200];
            if (sparse_check_csr(off, terms, vals, nq, sp->vocab, SP_MAX_TERMS, "query", msg, sizeof msg)) return fail(ICD_ERR_INVALID, "%s", msg);
            nnz = off[nq];
        } else if (!terms || !vals) {
            return fail(ICD_ERR_INVALID, "q_terms / q_vals NULL");
        }
        return ICD_OK;
    }

    // behind the caller's locks and check_capture: the postings, queries, masks and tiles of `a`. masks != nullptr (a table that holds a
    // mask): the call reads section 12's table of the index, so `table` takes the index's mutex here and the caller keeps it to its last
    // launch, as every masked dense search does (an unmasked call touches nothing of the index's workspace). A host caller's queries go
    // into the sparse index's staging.
    int stage(icd_index *idx, icd_sparse *sp, icd_rowmask *const *masks, std::unique_lock<std::mutex> &table, hipStream_t s, SparseArgs &a) {
        int rc;
        if (masks) {
            table.lock();
            if ((rc = stage_masks(idx, masks, (int)nq, s))) return rc;
        }
        a.post_off = sp->post_off; a.post_row = sp->post_row; a.post_val = sp->post_val; a.vocab = sp->vocab;
        a.q_off = reinterpret_cast<const long long *>(off); a.q_terms = terms; a.q_vals = vals;
        if (!on_device) {
            HIP_TRY(hipMemcpyAsync(sp->q_off, off, ((size_t)nq + 1) * 8, hipMemcpyHostToDevice, s));
            if (nnz) {
                HIP_TRY(hipMemcpyAsync(sp->q_terms, terms, (size_t)nnz * 4, hipMemcpyHostToDevice, s));
                HIP_TRY(hipMemcpyAsync(sp->q_vals, vals, (size_t)nnz * 4, hipMemcpyHostToDevice, s));
            }
            a.q_off = sp->q_off; a.q_terms = sp->q_terms; a.q_vals = sp->q_vals;
        }
        a.masks = masks ? idx->mask_dev : nullptr;
        a.mask_words = rowmask_tile_words(idx->n);
        a.tiles = sp->tiles;
        return ICD_OK;
    }
};

// icd_sparse_search and icd_sparse_search_range: rb = nullptr is the search without a band, through the BAND = false kernel.
static int sparse_search_lists(icd_index *idx, icd_sparse *sp, const int64_t *q_off, const uint32_t *q_terms, const float *q_vals, int64_t nq,
                               int32_t k, int32_t queries_on_device, icd_rowmask *const *masks, const RangeBounds *rb, int32_t reweighted,
                               double *out_adj, float *out_raw, int64_t *out_ids, int32_t *out_levels, int32_t out_on_device, void *stream) {
    // every check comes before the first device call
    if (!valid(idx)) return fail(ICD_ERR_STATE, "invalid handle");
    if (!valid_handle(sp)) return fail(ICD_ERR_STATE, "invalid sparse index handle");
    int rc = check_owner(sp->at, idx, "the sparse index");
    if (rc) return rc;
    if (idx->row_map) return fail(ICD_ERR_UNSUPPORTED, "a sparse search on a view is not supported");
    if (k < 1 || k > ICD_MAX_K) return fail(ICD_ERR_INVALID, "k=%d: a sparse search returns 1 .. %d hits per query", k, ICD_MAX_K);
    if (k > sp->max_k) return fail(ICD_ERR_INVALID, "k=%d exceeds the sparse index's max_k=%d", k, sp->max_k);
    if (nq < 0 || nq > sp->max_nq) return fail(ICD_ERR_INVALID, "nq=%lld exceeds the sparse index's max_nq=%d", (long long)nq, sp->max_nq);
    if (!out_raw || !out_ids || (reweighted && !out_adj)) return fail(ICD_ERR_INVALID, "output pointer is NULL");
    if (rb) {
        if ((rb->after_scores == nullptr) != (rb->after_ids == nullptr))
            return fail(ICD_ERR_INVALID, "after_scores and after_ids: both or neither (a cursor is a hit's score AND id)");
        if ((rc = check_bands(*rb, nq, "query"))) return rc;
    }
    bool any_mask = false;
    if (masks && (rc = check_masks(idx, masks, nq, "masked sparse search", &any_mask))) return rc;
    if (nq == 0) return ICD_OK;
    SparseQueries sq{q_off, q_terms, q_vals, nq, queries_on_device != 0};
    if ((rc = sq.check(sp))) return rc;
    std::lock_guard<std::mutex> guard(sp->mu);
    HIP_TRY(hipSetDevice(idx->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const HostCall hc{s, queries_on_device != 0, out_on_device != 0};
    const bool host_bands = rb && !rb->on_device;
    if ((rc = check_capture(s, !queries_on_device || !out_on_device, host_bands, any_mask))) return rc;
    std::unique_lock<std::mutex> table(idx->mu, std::defer_lock);
    SparseArgs a{};
    if ((rc = sq.stage(idx, sp, any_mask ? masks : nullptr, table, s, a))) return rc;
    a.nq = (int)nq; a.k = k; a.part = sp->part;
    if (rb) {   // the bounds -> BandQ (a sparse index has no views: row_map = nullptr), then the BAND = true form
        if (rb->on_device) {
            hipLaunchKernelGGL(band_pack_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s, rb->radius, rb->range_filter, rb->after_scores,
                               rb->after_ids, (int)nq, (const long long *)nullptr, (long long)idx->n, (long long)idx->id_base, sp->band_dev);
            HIP_TRY(hipGetLastError());
        } else {
            for (int64_t q = 0; q < nq; ++q)
                sp->h_band[q] = pack_band_host(*rb, q, rb->after_ids ? band_cut_plain(rb->after_ids[q], idx->id_base, idx->n) : 0);
            HIP_TRY(hipMemcpyAsync(sp->band_dev, sp->h_band, (size_t)nq * sizeof(BandQ), hipMemcpyHostToDevice, s));
        }
        hipLaunchKernelGGL(sparse_accumulate_select_kernel<true>, dim3((unsigned)(nq * sp->tiles)), dim3(SP_THREADS), 0, s, a, SparseBands<true>{sp->band_dev});
    } else {
        hipLaunchKernelGGL(sparse_accumulate_select_kernel<false>, dim3((unsigned)(nq * sp->tiles)), dim3(SP_THREADS), 0, s, a, SparseBands<false>{});
    }
    HIP_TRY(hipGetLastError());
    SparseMergeArgs m{};
    m.part = sp->part; m.tiles = sp->tiles; m.nq = (int)nq; m.k = k; m.reweighted = reweighted ? 1 : 0;
    m.id_base = idx->id_base; m.levels = idx->levels;
    m.out_adj = reweighted ? hc.target(out_adj, sp->o_adj) : nullptr; m.out_raw = hc.target(out_raw, sp->o_raw);
    m.out_ids = hc.target(reinterpret_cast<long long *>(out_ids), sp->o_ids); m.out_levels = hc.target(out_levels, sp->o_lv);
    hipLaunchKernelGGL(sparse_merge_kernel, dim3((unsigned)nq), dim3(SP_THREADS), 0, s, m);
    HIP_TRY(hipGetLastError());
    if ((rc = hc.copy_back({{reweighted ? out_adj : nullptr, m.out_adj, 8}, {out_raw, m.out_raw, 4}, {out_ids, m.out_ids, 8}, {out_levels, m.out_levels, 4}},
                           (size_t)nq * k)))
        return rc;
    return hc.finish(host_bands);   // (host bounds went through the pinned block: the next call may repack it)
}

extern "C" {

int icd_sparse_search(icd_index *idx, icd_sparse *sp, const int64_t *q_off, const uint32_t *q_terms, const float *q_vals, int64_t nq,
                      int32_t k, int32_t queries_on_device, icd_rowmask *const *masks, int32_t reweighted, double *out_adj, float *out_raw,
                      int64_t *out_ids, int32_t *out_levels, int32_t out_on_device, void *stream) {
    return sparse_search_lists(idx, sp, q_off, q_terms, q_vals, nq, k, queries_on_device, masks, nullptr, reweighted, out_adj, out_raw, out_ids,
                               out_levels, out_on_device, stream);
}

// (no bound at all IS icd_sparse_search: the same kernel instantiations, nothing packed)
int icd_sparse_search_range(icd_index *idx, icd_sparse *sp, const int64_t *q_off, const uint32_t *q_terms, const float *q_vals, int64_t nq,
                            int32_t k, int32_t queries_on_device, icd_rowmask *const *masks, const float *radius, const float *range_filter,
                            const float *after_scores, const int64_t *after_ids, int32_t bounds_on_device, int32_t reweighted, double *out_adj,
                            float *out_raw, int64_t *out_ids, int32_t *out_levels, int32_t out_on_device, void *stream) {
    const RangeBounds rb{radius, range_filter, after_scores, reinterpret_cast<const long long *>(after_ids), bounds_on_device != 0};
    const bool any = radius || range_filter || after_scores || after_ids;
    return sparse_search_lists(idx, sp, q_off, q_terms, q_vals, nq, k, queries_on_device, masks, any ? &rb : nullptr, reweighted, out_adj, out_raw,
                               out_ids, out_levels, out_on_device, stream);
}

// ---- grouped sparse search -------------------------------------------------------------------------------
// The one-time pairing of a grouping with a sparse index of the same index: builds the grouping's row -> position table (one
// launch over `order`, memory the grouping owns) so that no search allocates. Idempotent; a grouping that is never paired keeps
// the bytes icd_grouping_stats has always reported.
int icd_grouping_pair_sparse(icd_index *idx, icd_grouping *grouping, icd_sparse *sp) {
    if (!valid(idx)) return fail(ICD_ERR_STATE, "invalid handle");
    if (!valid_handle(grouping)) return fail(ICD_ERR_STATE, "invalid grouping handle");
    if (!valid_handle(sp)) return fail(ICD_ERR_STATE, "invalid sparse index handle");
    int rc = check_owner(grouping->at, idx, "the grouping");
    if (rc) return rc;
    if ((rc = check_owner(sp->at, idx, "the sparse index"))) return rc;
    std::lock_guard<std::mutex> guard(grouping->mu);
    if (grouping->pos_of) return ICD_OK;
    HIP_TRY(hipSetDevice(idx->device));
    const int n = (int)grouping->at.n;
    // a stream of its own (a NULL-stream launch or a device-wide wait would collide with a capture elsewhere on the device); the
    // table joins the handle's allocations only once it is built, so a failure leaves nothing behind
    int *pos = nullptr;
    hipStream_t st = nullptr;
    HIP_TRY(dmalloc(&pos, (size_t)n));
    hipError_t e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(grouping_invert_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, grouping->order, pos, n);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        hipStreamDestroy(st);
    }
    if (e != hipSuccess) {
        hipFree(pos);
        return fail(ICD_ERR_HIP, "pairing a grouping with a sparse index: %s", hipGetErrorString(e));
    }
    grouping->allocs.push_back(pos);
    grouping->pos_of = pos;
    grouping->bytes += (size_t)n * sizeof(int);
    return ICD_OK;
}

int icd_sparse_search_grouped(icd_index *idx, icd_sparse *sp, icd_grouping *grouping, const int64_t *q_off, const uint32_t *q_terms,
                              const float *q_vals, int64_t nq, int32_t k, int32_t group_size, int32_t queries_on_device,
                              icd_rowmask *const *masks, int32_t reweighted, double *out_adj, float *out_raw, int64_t *out_ids,
                              int32_t *out_levels, int32_t *out_groups, int32_t out_on_device, void *stream) {
    // every check comes before the first device call
    if (!valid(idx)) return fail(ICD_ERR_STATE, "invalid handle");
    if (!valid_handle(sp)) return fail(ICD_ERR_STATE, "invalid sparse index handle");
    if (!valid_handle(grouping)) return fail(ICD_ERR_STATE, "invalid grouping handle");
    icd_grouping *g = grouping;
    int rc = check_owner(sp->at, idx, "the sparse index");
    if (rc) return rc;
    if ((rc = check_owner(g->at, idx, "the grouping"))) return rc;
    if (idx->row_map) return fail(ICD_ERR_UNSUPPORTED, "a sparse search on a view is not supported");
    if (k < 1 || group_size < 1 || (int64_t)k * group_size > ICD_MAX_K)
        return fail(ICD_ERR_INVALID, "k=%d group_size=%d: need k >= 1, group_size >= 1 and k * group_size <= %d", k, group_size, ICD_MAX_K);
    if (nq < 0 || nq > sp->max_nq) return fail(ICD_ERR_INVALID, "nq=%lld exceeds the sparse index's max_nq=%d", (long long)nq, sp->max_nq);
    if (nq > g->max_nq) return fail(ICD_ERR_INVALID, "nq=%lld exceeds the grouping's max_nq=%d", (long long)nq, g->max_nq);
    if (!out_raw || !out_ids || (reweighted && !out_adj)) return fail(ICD_ERR_INVALID, "output pointer is NULL");
    bool any_mask = false;
    if (masks && (rc = check_masks(idx, masks, nq, "masked sparse search", &any_mask))) return rc;
    if (nq == 0) return ICD_OK;
    SparseQueries sq{q_off, q_terms, q_vals, nq, queries_on_device != 0};
    if ((rc = sq.check(sp))) return rc;
    // lock order: sparse index, grouping, index
    std::lock_guard<std::mutex> guard_sp(sp->mu);
    std::lock_guard<std::mutex> guard_g(g->mu);
    if (!g->pos_of) return fail(ICD_ERR_STATE, "the grouping was never paired with a sparse index (icd_grouping_pair_sparse)");
    HIP_TRY(hipSetDevice(idx->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const HostCall hc{s, queries_on_device != 0, out_on_device != 0};
    if ((rc = check_capture(s, !queries_on_device || !out_on_device, false, any_mask))) return rc;
    std::unique_lock<std::mutex> table(idx->mu, std::defer_lock);
    SparseStoreArgs a{};
    if ((rc = sq.stage(idx, sp, any_mask ? masks : nullptr, table, s, a.sp))) return rc;
    a.n = (int)idx->n; a.pos_of = g->pos_of; a.S = g->S; a.ldS = g->ldS;
    const GroupedOuts o{hc.target(out_adj, g->o_adj), hc.target(out_raw, g->o_raw), hc.target(reinterpret_cast<long long *>(out_ids), g->o_ids),
                        hc.target(out_levels, g->o_lv), hc.target(out_groups, g->o_grp)};
    for (int64_t q0 = 0; q0 < nq; q0 += g->qb) {   // passes of the grouping's query block
        const int nb = (int)std::min<int64_t>(g->qb, nq - q0);
        a.sp.nq = nb; a.q_base = (int)q0;
        hipLaunchKernelGGL(sparse_store_kernel, dim3((unsigned)((int64_t)nb * sp->tiles)), dim3(SP_THREADS), 0, s, a);
        HIP_TRY(hipGetLastError());
        if ((rc = grouped_reduce_pass(idx, g, nb, q0, k, group_size, reweighted != 0, o, s))) return rc;
    }
    if ((rc = hc.copy_back({{reweighted ? out_adj : nullptr, o.d_adj, 8}, {out_raw, o.d_raw, 4}, {out_ids, o.d_ids, 8}, {out_levels, o.d_lv, 4},
                            {out_groups, o.d_grp, 4}}, (size_t)nq * k * group_size)))
        return rc;
    return hc.finish();
}

}  // extern "C"
