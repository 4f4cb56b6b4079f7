// icd_filter.hpp - filter expressions on the device (icd_columns_*, icd_filter_program_check, icd_filter_rowmasks; DESIGN.md section
// 18): the row masks of a batch of filter programs over an index's int32 columns and a sparse index's postings, built by
// filter_mask_kernel. Part of icd_search.hip's translation unit (fail(), HIP_TRY, the owned-handle and mask helpers, icd_sparse);
// included there and nowhere else.
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

// ONE allocation holds what the call's nq masks and its kernel need: [nq][words] bitsets (tile words + the zero tail), [nq] row
// counters, [nq] base pointers (with a base mask), [nq + 1] program offsets and the programs. Every mask is an ordinary icd_rowmask
// that points into it; the block goes with the last of them (icd_rowmask_destroy).
int icd_filter_rowmasks(icd_index *idx, icd_columns *columns, icd_sparse *sp, const int64_t *prog_off, const uint32_t *prog, int64_t nq,
                        icd_rowmask *const *base_masks, icd_rowmask **out_masks, void *stream) {
    if (!out_masks) return fail(ICD_ERR_INVALID, "out_masks is NULL");
    if (nq < 0) return fail(ICD_ERR_INVALID, "nq=%lld", (long long)nq);
    for (int64_t q = 0; q < nq; ++q) out_masks[q] = nullptr;
    // every check comes before the first device call
    if (!valid(idx)) return fail(ICD_ERR_STATE, "invalid handle");
    if (idx->row_map) return fail(ICD_ERR_UNSUPPORTED, "row masks on a view are not supported: mask the parent");
    if (!valid_handle(columns)) return fail(ICD_ERR_STATE, "invalid columns handle");
    int rc = check_owner(columns->at, idx, "the columns");
    if (rc) return rc;
    if (sp) {
        if (!valid_handle(sp)) return fail(ICD_ERR_STATE, "invalid sparse index handle");
        if ((rc = check_owner(sp->at, idx, "the sparse index"))) return rc;
    }
    const int64_t tiles = (idx->n + SP_TILE - 1) / SP_TILE;
    if (nq * tiles > 0x7FFFFFFFll) return fail(ICD_ERR_INVALID, "nq=%lld: %lld tiles of rows times nq exceed 2^31 - 1 work-groups", (long long)nq, (long long)tiles);
    bool any_base = false;
    if (base_masks)
        for (int64_t q = 0; q < nq; ++q) {
            const icd_rowmask *m = base_masks[q];
            if (!m) continue;
            any_base = true;
            if (!valid_handle(m)) return fail(ICD_ERR_STATE, "base_masks[%lld]: invalid row mask handle", (long long)q);
            if ((rc = check_owner(m->at, idx, "base_masks", (long long)q))) return rc;
        }
    if (nq == 0) return ICD_OK;
    char msg[200];
    bool any_text = false;
    if (filter_check_programs(prog_off, prog, nq, columns->ncols, sp ? sp->vocab : 0, msg, sizeof msg, &any_text)) return fail(ICD_ERR_INVALID, "%s", msg);
    const int64_t p_words = prog_off[nq];
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (stream_capturing(s)) return fail(ICD_ERR_INVALID, "icd_filter_rowmasks allocates: it cannot be captured into a graph");
    HIP_TRY(hipSetDevice(idx->device));

    const size_t words = (size_t)rowmask_tile_words(idx->n) + ROWMASK_TAIL_WORDS;   // (a multiple of 4: every bitset starts 16-byte aligned)
    const size_t b_bits = (size_t)nq * words * 4, b_cnt = (((size_t)nq * 4) + 15) / 16 * 16;
    const size_t b_base = any_base ? (size_t)nq * 8 : 0, b_off = ((size_t)nq + 1) * 8, b_prog = (size_t)p_words * 4;
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
#define FM_TRY(expr) HIP_TRY_OR(undo(), expr)
    FM_TRY(hipMalloc(reinterpret_cast<void **>(&dev), b_bits + b_cnt + b_base + b_off + b_prog));
    blk->dev = dev;
    uint32_t *d_bits = reinterpret_cast<uint32_t *>(dev);
    int *d_cnt = reinterpret_cast<int *>(dev + b_bits);
    const uint32_t **d_base = reinterpret_cast<const uint32_t **>(dev + b_bits + b_cnt);
    long long *d_off = reinterpret_cast<long long *>(dev + b_bits + b_cnt + b_base);
    uint32_t *d_prog = reinterpret_cast<uint32_t *>(dev + b_bits + b_cnt + b_base + b_off);
    for (int64_t q = 0; q < nq; ++q) {
        icd_rowmask *m = new_handle<icd_rowmask>(idx);
        if (!m) { undo(); return fail(ICD_ERR_NOMEM, "host allocation failed"); }
        m->rows = -1; m->bytes = words * sizeof(uint32_t) + sizeof(int);
        m->bits = d_bits + (size_t)q * words; m->count_dev = d_cnt + q; m->block = blk;
        made.push_back(m);
    }
    FM_TRY(hipMemsetAsync(dev, 0, b_bits + b_cnt, s));   // (the tails, the words of tiles the kernel leaves alone, the counters)
    FM_TRY(hipMemcpyAsync(d_off, prog_off, ((size_t)nq + 1) * 8, hipMemcpyHostToDevice, s));
    FM_TRY(hipMemcpyAsync(d_prog, prog, (size_t)p_words * 4, hipMemcpyHostToDevice, s));   // (every program holds a word: p_words >= nq)
    FilterMaskArgs a{};
    a.cols = columns->cols; a.prog_off = d_off; a.prog = d_prog;
    if (any_text) { a.post_off = sp->post_off; a.post_row = sp->post_row; }
    if (any_base) {
        for (int64_t q = 0; q < nq; ++q) h_base[(size_t)q] = base_masks[q] ? base_masks[q]->bits : nullptr;
        FM_TRY(hipMemcpyAsync(d_base, h_base.data(), (size_t)nq * 8, hipMemcpyHostToDevice, s));
        a.base = d_base;
    }
    a.bits = d_bits; a.stride = (long long)words; a.count = d_cnt;
    a.n = idx->n; a.mask_words = rowmask_tile_words(idx->n); a.tiles = (int)tiles;
    hipLaunchKernelGGL(filter_mask_kernel, dim3((unsigned)(nq * tiles)), dim3(SP_THREADS), 0, s, a);
    FM_TRY(hipGetLastError());
    FM_TRY(hipStreamSynchronize(s));   // the programs were staged from pageable host buffers: the call returns once the stream has taken them
#undef FM_TRY
    blk->refs.store((int)nq);
    for (int64_t q = 0; q < nq; ++q) out_masks[q] = made[(size_t)q];
    return ICD_OK;
}

}  // extern "C"
