// icd_filter.hpp - filter expressions on the device (icd_columns_*, icd_filter_program_check, icd_filter_rowmasks; DESIGN.md section
// 18): the row masks of a batch of filter programs over an index's int32 columns and a sparse index's postings, built by
// filter_mask_kernel. icd_filter_rowmasks' shared checks, its masks' block and the undo / publish are ProducedMasks'
// (icd_range_mask.hpp). Part of icd_search.hip's translation unit (fail(), HIP_TRY, the owned-handle helpers, icd_sparse); included
// there and nowhere else.
#pragma once

// The int32 columns of an index's rows: [ncols][n] on the device. Belongs to the index it was created for but keeps no pointer into
// it: handle and identity are compared, never followed.
struct icd_columns : OwnedHandle {
    static constexpr uint32_t MAGIC = 0x1CDC0175u;
    static constexpr const char *NOUN = "columns";
    int ncols = 0;
    int *cols = nullptr;   // [ncols][n]
};

static_assert(ICD_FILTER_RANGE == FOP_RANGE && ICD_FILTER_SET == FOP_SET && ICD_FILTER_TEXT == FOP_TEXT && ICD_FILTER_AND == FOP_AND &&
              ICD_FILTER_OR == FOP_OR && ICD_FILTER_NOT == FOP_NOT, "include/icd_search.h and filter_program.hpp disagree");

extern "C" {

int icd_columns_create(icd_index *idx, const int32_t *cols, int32_t ncols, icd_columns **out) {
    if (!out) return fail(ICD_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!valid(idx)) return fail(ICD_ERR_STATE, "invalid handle");
    if (idx->row_map) return fail(ICD_ERR_UNSUPPORTED, "columns on a view are not supported: filter the parent");
    if (idx->n > 0x7FFFFFFFll) return fail(ICD_ERR_UNSUPPORTED, "n=%lld: the filter kernel addresses rows with 31 bits (n < 2^31)", (long long)idx->n);
    if (!cols || ncols < 1 || ncols > ICD_FILTER_MAX_COLUMNS) return fail(ICD_ERR_INVALID, "cols NULL or ncols=%d (1 .. %d)", ncols, ICD_FILTER_MAX_COLUMNS);
    HIP_TRY(hipSetDevice(idx->device));
    icd_columns *c = new_handle<icd_columns>(idx);
    if (!c) return fail(ICD_ERR_NOMEM, "host allocation failed");
    const size_t count = (size_t)ncols * (size_t)idx->n;
    c->ncols = ncols; c->bytes = count * sizeof(int);
    HIP_TRY_OR(free_handle(c), c->alloc(&c->cols, count));
    HIP_TRY_OR(free_handle(c), hipMemcpy(c->cols, cols, count * sizeof(int), hipMemcpyHostToDevice));
    *out = c;
    return ICD_OK;
}

int icd_columns_destroy(icd_columns *columns) { return destroy_handle(columns); }

int icd_columns_stats(icd_columns *columns, int32_t *out_ncols, int64_t *out_rows, int64_t *out_bytes) {
    if (!valid_handle(columns)) return fail(ICD_ERR_STATE, "invalid columns handle");
    if (out_ncols) *out_ncols = columns->ncols;
    if (out_rows) *out_rows = columns->at.n;
    if (out_bytes) *out_bytes = (int64_t)columns->bytes;
    return ICD_OK;
}

int icd_filter_program_check(const int64_t *prog_off, const uint32_t *prog, int64_t nq, int32_t ncols, int64_t vocab, char *msg, int64_t msg_len) {
    char local[200];
    const bool own = !msg || msg_len < 1;
    if (filter_check_programs(prog_off, prog, nq, ncols, vocab, own ? local : msg, own ? sizeof local : (size_t)msg_len))
        return fail(ICD_ERR_INVALID, "%s", own ? local : msg);
    return ICD_OK;
}

// Behind the block's base pointers: [nq + 1] program offsets and the programs.
int icd_filter_rowmasks(icd_index *idx, icd_columns *columns, icd_sparse *sp, const int64_t *prog_off, const uint32_t *prog, int64_t nq,
                        icd_rowmask *const *base_masks, icd_rowmask **out_masks, void *stream) {
    int rc = produced_check_index(idx, nq, out_masks);
    if (rc) return rc;
    if (!valid_handle(columns)) return fail(ICD_ERR_STATE, "invalid columns handle");
    if ((rc = check_owner(columns->at, idx, "the columns"))) return rc;
    if (sp) {
        if (!valid_handle(sp)) return fail(ICD_ERR_STATE, "invalid sparse index handle");
        if ((rc = check_owner(sp->at, idx, "the sparse index"))) return rc;
    }
    int64_t tiles = 0;
    bool any_base = false;
    if ((rc = produced_check_batch(idx, nq, base_masks, &tiles, &any_base))) return rc;
    if (nq == 0) return ICD_OK;
    char msg[200];
    bool any_text = false;
    if (filter_check_programs(prog_off, prog, nq, columns->ncols, sp ? sp->vocab : 0, msg, sizeof msg, &any_text)) return fail(ICD_ERR_INVALID, "%s", msg);
    const size_t staged[2] = {((size_t)nq + 1) * 8, (size_t)prog_off[nq] * 4};   // (every program holds a word: the second is never empty)
    ProducedMasks pm;
    if ((rc = pm.begin("icd_filter_rowmasks", idx, nq, base_masks, any_base, out_masks, staged, 2, stream))) return rc;

    long long *d_off = pm.region<long long>(pm.at.staged[0]);
    uint32_t *d_prog = pm.region<uint32_t>(pm.at.staged[1]);
    PM_TRY(pm, hipMemcpyAsync(d_off, prog_off, staged[0], hipMemcpyHostToDevice, pm.s));
    PM_TRY(pm, hipMemcpyAsync(d_prog, prog, staged[1], hipMemcpyHostToDevice, pm.s));
    FilterMaskArgs a{};
    a.cols = columns->cols; a.prog_off = d_off; a.prog = d_prog;
    if (any_text) { a.post_off = sp->post_off; a.post_row = sp->post_row; }
    pm.fill(&a, idx, tiles);
    hipLaunchKernelGGL(filter_mask_kernel, dim3((unsigned)(nq * tiles)), dim3(SP_THREADS), 0, pm.s, a);
    PM_TRY(pm, hipGetLastError());
    PM_TRY(pm, hipStreamSynchronize(pm.s));   // the programs were staged from pageable host buffers: the call returns once the stream has taken them
    pm.publish();
    return ICD_OK;
}

}  // extern "C"
