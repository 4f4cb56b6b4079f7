// icd_range_mask.hpp - range and masked search (DESIGN.md sections 11 and 12): the callers' bounds and their packing, the row-mask
// handle and its table, the block of a call's produced masks (ProducedMasks: sections 17.3 and 18.3), icd_index_search_range /
// icd_index_search_masked. Part of icd_search.hip's translation unit (fail(), HIP_TRY, the owned-handle and request helpers,
// run_search); included there and nowhere else.
#pragma once
#include "produced_mask_layout.hpp"

// The bounds of a banded search as the caller gave them: packed into BandQ inside run_search, under the handle's mutex.
struct RangeBounds {
    const float *radius, *range_filter, *after_scores;
    const long long *after_ids;
    bool on_device;
};

// The band checks, over `count` entries: host bounds hold no NaN and radius < range_filter (device
// bounds cannot be read without a synchronisation: an empty or inverted band there simply yields padding). `unit`: what an entry
// is called in the message ("query", "sub-search").
static int check_bands(const RangeBounds &rb, int64_t count, const char *unit) {
    if (rb.on_device) return ICD_OK;
    for (int64_t q = 0; q < count; ++q) {
        if (rb.radius && std::isnan(rb.radius[q])) return fail(ICD_ERR_INVALID, "radius[%lld] is NaN", (long long)q);
        if (rb.range_filter && std::isnan(rb.range_filter[q])) return fail(ICD_ERR_INVALID, "range_filter[%lld] is NaN", (long long)q);
        if (rb.after_scores && std::isnan(rb.after_scores[q])) return fail(ICD_ERR_INVALID, "after_scores[%lld] is NaN", (long long)q);
        if (rb.radius && rb.range_filter && !(rb.radius[q] < rb.range_filter[q]))
            return fail(ICD_ERR_INVALID, "%s %lld: radius=%g must be below range_filter=%g (hits have radius < score <= range_filter)", unit, (long long)q, (double)rb.radius[q], (double)rb.range_filter[q]);
    }
    return ICD_OK;
}

// ---- range search: the callers' bounds -> BandQ (topk_select.hpp) --------------------------------------
// The cursor names a hit by its GLOBAL id; the kernels compare keys of LOCAL rows. cut = the first local row whose id is larger
// than the cursor's: id - id_base + 1 clamped to [0, n], or on a view the upper bound in its strictly increasing row map - once
// per query, here, not per score.
__global__ void band_pack_kernel(const float *radius, const float *range_filter, const float *after_scores, const long long *after_ids,
                                 int nq, const long long *row_map, long long n, long long id_base, BandQ *out) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    BandQ b;
    b.lo = radius ? radius[q] : -INFINITY;
    b.hi = range_filter ? range_filter[q] : INFINITY;
    b.below = ~0ull;
    if (b.lo != b.lo || b.hi != b.hi) { b.lo = INFINITY; b.hi = -INFINITY; }   // (NaN bounds, unseen by the host: an empty band)
    if (after_scores) {
        const float as = after_scores[q];
        const long long id = after_ids[q];
        long long cut;
        if (row_map) {
            long long lo = 0, hi = n;   // first local row with row_map[row] > id
            while (lo < hi) { const long long mid = (lo + hi) >> 1; if (row_map[mid] > id) hi = mid; else lo = mid + 1; }
            cut = lo;
        } else {
            cut = id < id_base ? 0 : (id - id_base >= n ? n : id - id_base + 1);
        }
        b.below = as != as ? 0ull : band_below(order_f32(as), (uint32_t)cut);
    }
    out[q] = b;
}

static uint32_t host_order_f32(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

// One query's host bounds -> BandQ, for an index without a row map (row_map == nullptr in band_pack_kernel's terms): the dense
// range search off a view and the sparse range search (icd_sparse.hpp) share it.
static long long band_cut_plain(long long id, long long id_base, long long n) {
    return id < id_base ? 0 : (id - id_base >= n ? n : id - id_base + 1);
}
static BandQ pack_band_host(const RangeBounds &rb, int64_t q, long long cut) {   // cut: read only with a cursor
    BandQ b;
    b.lo = rb.radius ? rb.radius[q] : -INFINITY;
    b.hi = rb.range_filter ? rb.range_filter[q] : INFINITY;
    b.below = rb.after_scores ? band_below(host_order_f32(rb.after_scores[q]), (uint32_t)cut) : ~0ull;
    return b;
}

// Host bounds were validated by check_bands; device bounds are packed as they are.
static int pack_bands(icd_index *x, const RangeBounds &rb, int nq, hipStream_t s, BandArgs *out) {
    out->q = x->band_dev;
    if (rb.on_device) {
        hipLaunchKernelGGL(band_pack_kernel, dim3((nq + 255) / 256), dim3(256), 0, s, rb.radius, rb.range_filter, rb.after_scores,
                           rb.after_ids, nq, x->row_map, (long long)x->n, (long long)x->id_base, x->band_dev);
        HIP_TRY(hipGetLastError());
        return ICD_OK;
    }
    for (int q = 0; q < nq; ++q) {
        long long cut = 0;
        if (rb.after_scores) {
            const long long id = rb.after_ids[q];
            if (x->row_map) cut = std::upper_bound(x->h_row_map.begin(), x->h_row_map.end(), id) - x->h_row_map.begin();
            else cut = band_cut_plain(id, x->id_base, x->n);
        }
        const BandQ b = pack_band_host(rb, q, cut);
        x->h_band[q] = b;
        if (q < 4) out->inl[q] = b;
    }
    x->band_pending = nq;
    return ICD_OK;
}

// ---- row masks (icd_rowmask_create) ---------------------------------------------------------------------
struct icd_rowmask : OwnedHandle {
    static constexpr uint32_t MAGIC = 0x1CD3A5C1u;
    static constexpr const char *NOUN = "row mask";
    int64_t rows = 0;           // -1: counted on the device (count_dev), read back by the first icd_rowmask_stats
    uint32_t *bits = nullptr;   // [rowmask_tile_words(n) + ROWMASK_TAIL_WORDS]
    // a produced mask (ProducedMasks below; DESIGN.md sections 17 and 18): bits and count_dev point into ONE allocation the masks
    // of that call share; the last of them to be destroyed frees it
    struct SharedBlock { void *dev = nullptr; std::atomic<int> refs{0}; };
    SharedBlock *block = nullptr;
    const int *count_dev = nullptr;
};

// The mask table of a call, over `count` entries against an index: no table on a view, every entry NULL or a live mask of THIS
// index. *any: the table holds a mask at all (an all-NULL table is no table). `noun`: the search's name in the message.
static int check_masks(const icd_index *idx, icd_rowmask *const *masks, int64_t count, const char *noun, bool *any) {
    if (idx->row_map) return fail(ICD_ERR_UNSUPPORTED, "a %s on a view is not supported: mask the parent", noun);
    if (count > idx->max_nq) return fail(ICD_ERR_INVALID, "nq=%lld exceeds max_nq=%d", (long long)count, idx->max_nq);   // (before the table is read)
    for (int64_t q = 0; q < count; ++q) {
        const icd_rowmask *m = masks[q];
        if (!m) continue;
        *any = true;
        if (!valid_handle(m)) return fail(ICD_ERR_STATE, "masks[%lld]: invalid row mask handle", (long long)q);
        if (const int rc = check_owner(m->at, idx, "masks", (long long)q)) return rc;
    }
    return ICD_OK;
}

// the [query] -> bitset table of a masked search: filled in the pinned block under the handle's mutex, one copy per call. An
// event recorded right behind the copy guards the block: the next masked call waits for it before it refills the block, so
// neither a device-in / device-out call (which only enqueues) nor an error return further down leaves a copy reading a block
// that is being rewritten. (A view has no table: check_masks refused the call.)
static int stage_masks(icd_index *x, icd_rowmask *const *masks, int nq, hipStream_t s) {
    if (x->mask_copy_pending) { HIP_TRY(hipEventSynchronize(x->ev_mask)); x->mask_copy_pending = false; }
    for (int q = 0; q < nq; ++q) x->h_mask[q] = (masks && masks[q]) ? masks[q]->bits : x->mask_ones;   // (masks == nullptr: a boosted search without a table)
    const hipError_t ec = hipMemcpyAsync(x->mask_dev, x->h_mask, (size_t)nq * sizeof(uint32_t *), hipMemcpyHostToDevice, s);
    const hipError_t ee = hipEventRecord(x->ev_mask, s);   // (also behind a copy that failed to enqueue: whatever did get queued is covered)
    x->mask_copy_pending = ee == hipSuccess;
    if (ec != hipSuccess || ee != hipSuccess) {
        hipStreamSynchronize(s);
        x->mask_copy_pending = false;
        return fail(ICD_ERR_HIP, "mask table: %s", hipGetErrorString(ec != hipSuccess ? ec : ee));
    }
    return ICD_OK;
}

// ---- produced masks: what icd_sparse_match_rowmasks and icd_filter_rowmasks share (DESIGN.md sections 17.3 and 18.3) ------------
// Their common checks, in the two places they hold in both entries: the entry's own handle checks stand between them (handle-state
// errors win over ownership errors). The base table follows check_masks' rules without its bound on the table's length.
static int produced_check_index(icd_index *idx, int64_t nq, icd_rowmask **out_masks) {
    if (!out_masks) return fail(ICD_ERR_INVALID, "out_masks is NULL");
    if (nq < 0) return fail(ICD_ERR_INVALID, "nq=%lld", (long long)nq);
    for (int64_t q = 0; q < nq; ++q) out_masks[q] = nullptr;
    if (!valid(idx)) return fail(ICD_ERR_STATE, "invalid handle");
    if (idx->row_map) return fail(ICD_ERR_UNSUPPORTED, "row masks on a view are not supported: mask the parent");
    return ICD_OK;
}
static int produced_check_batch(const icd_index *idx, int64_t nq, icd_rowmask *const *base_masks, int64_t *tiles, bool *any_base) {
    *tiles = (idx->n + SP_TILE - 1) / SP_TILE;
    if (nq * *tiles > 0x7FFFFFFFll) return fail(ICD_ERR_INVALID, "nq=%lld: %lld tiles of rows times nq exceed 2^31 - 1 work-groups", (long long)nq, (long long)*tiles);
    *any_base = false;
    for (int64_t q = 0; base_masks && q < nq; ++q) {
        const icd_rowmask *m = base_masks[q];
        if (!m) continue;
        *any_base = true;
        if (!valid_handle(m)) return fail(ICD_ERR_STATE, "base_masks[%lld]: invalid row mask handle", (long long)q);
        if (const int rc = check_owner(m->at, idx, "base_masks", (long long)q)) return rc;
    }
    return ICD_OK;
}

// The block of a call's nq masks (produced_mask_layout.hpp): ONE allocation of bitsets, row counters, base pointers and whatever
// the entry stages behind them. Every mask is an ordinary icd_rowmask that points into it; the block goes with the last of them
// (icd_rowmask_destroy). begin() refuses a capturing stream in the entry's name, allocates, makes the handles, clears bitsets and
// counters (the tails, the words of tiles the kernel leaves alone) and stages the base table; an entry then stages its regions
// and launches under PM_TRY, and publish() hands the masks out. Until then undo() takes everything back.
#define PM_TRY(pm, expr) HIP_TRY_OR((pm).undo(), expr)
struct ProducedMasks {
    hipStream_t s = nullptr;
    int64_t nq = 0;
    icd_rowmask **out = nullptr;
    ProducedMaskLayout at{};
    char *dev = nullptr;
    icd_rowmask::SharedBlock *blk = nullptr;
    std::vector<icd_rowmask *> made;
    std::vector<const uint32_t *> h_base;   // (with a base mask; pageable: alive until the entry's synchronisation)

    template <typename T>
    T *region(size_t offset) const { return reinterpret_cast<T *>(dev + offset); }

    // (the stream is drained first, a launch may be reading the block)
    void undo() {
        hipStreamSynchronize(s);
        for (icd_rowmask *m : made) free_handle(m);
        for (int64_t q = 0; q < nq; ++q) out[q] = nullptr;
        hipFree(dev);
        delete blk;
    }

    int begin(const char *entry, const icd_index *idx, int64_t nq_, icd_rowmask *const *base_masks, bool any_base, icd_rowmask **out_masks,
              const size_t *staged_bytes, int n_staged, void *stream) {
        s = reinterpret_cast<hipStream_t>(stream); nq = nq_; out = out_masks;
        if (stream_capturing(s)) return fail(ICD_ERR_INVALID, "%s allocates: it cannot be captured into a graph", entry);
        HIP_TRY(hipSetDevice(idx->device));
        at = produced_mask_layout(nq, idx->n, any_base, staged_bytes, n_staged);
        blk = new (std::nothrow) icd_rowmask::SharedBlock();
        try {
            made.reserve((size_t)nq);
            if (any_base) h_base.resize((size_t)nq);
        } catch (const std::bad_alloc &) {
            delete blk;
            blk = nullptr;
        }
        if (!blk) return fail(ICD_ERR_NOMEM, "host allocation failed");
        PM_TRY(*this, hipMalloc(reinterpret_cast<void **>(&dev), at.total));
        blk->dev = dev;
        for (int64_t q = 0; q < nq; ++q) {
            icd_rowmask *m = new_handle<icd_rowmask>(idx);
            if (!m) { undo(); return fail(ICD_ERR_NOMEM, "host allocation failed"); }
            m->rows = -1; m->bytes = at.words * sizeof(uint32_t) + sizeof(int);
            m->bits = region<uint32_t>(at.bits) + (size_t)q * at.words; m->count_dev = region<int>(at.counters) + q; m->block = blk;
            made.push_back(m);
        }
        PM_TRY(*this, hipMemsetAsync(dev, 0, at.zeroed, s));
        if (any_base) {
            for (int64_t q = 0; q < nq; ++q) h_base[(size_t)q] = base_masks[q] ? base_masks[q]->bits : nullptr;
            PM_TRY(*this, hipMemcpyAsync(region<void>(at.base), h_base.data(), (size_t)nq * 8, hipMemcpyHostToDevice, s));
        }
        return ICD_OK;
    }

    // the fields TextMatchArgs and FilterMaskArgs name alike
    template <typename Args>
    void fill(Args *a, const icd_index *idx, int64_t tiles) const {
        a->base = h_base.empty() ? nullptr : region<const uint32_t *>(at.base);
        a->bits = region<uint32_t>(at.bits); a->stride = (long long)at.words; a->count = region<int>(at.counters);
        a->n = idx->n; a->mask_words = rowmask_tile_words(idx->n); a->tiles = (int)tiles;
    }

    void publish() {
        blk->refs.store((int)nq);
        for (int64_t q = 0; q < nq; ++q) out[q] = made[(size_t)q];
    }
};

// ---- row masks --------------------------------------------------------------------------------------------------------------
// A row list that already sits on the device -> bitset: one memset in front, then one vector atomicOr per row. The list is
// checked here as well (inside [0, n), strictly increasing): a bad entry sets *err and writes nothing.
extern "C" {   // (the symbol this kernel has always had)
__global__ void rowmask_build_kernel(const long long *rows, long long n_rows, long long n, uint32_t *bits, int *err) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows) return;
    const long long r = rows[i];
    if (r < 0 || r >= n || (i > 0 && rows[i - 1] >= r)) { atomicOr(err, 1); return; }
    atomicOr(bits + (r >> 5), 1u << (r & 31));
}
}  // extern "C"


// The banded entry points behind their own checks: masks = nullptr is the range search, `noun` names the caller in messages;
// boost (icd_boost.hpp): the boosted search's table, its entries already checked.
// (The checks that need neither the handle nor the device come first.)
static int search_banded(icd_index *idx, icd_rowmask *const *masks, const char *noun, const float *queries, int64_t nq, int32_t k,
                         int32_t queries_on_device, const RangeBounds &rb, int32_t reweighted, double *out_adj, float *out_raw,
                         int64_t *out_ids, int32_t *out_levels, int32_t out_on_device, void *stream, const BoostRequest *boost = nullptr) {
    if (k < 1 || k > ICD_MAX_K) return fail(ICD_ERR_INVALID, "k=%d: a %s search returns 1 .. %d hits per query", k, noun, ICD_MAX_K);
    if ((rb.after_scores == nullptr) != (rb.after_ids == nullptr)) return fail(ICD_ERR_INVALID, "after_scores and after_ids: both or neither (a cursor is a hit's score AND id)");
    if (nq < 0) return fail(ICD_ERR_INVALID, "nq=%lld", (long long)nq);
    if (!out_raw || !out_ids || (reweighted && !out_adj)) return fail(ICD_ERR_INVALID, "output pointer is NULL");
    if (const int rc = check_bands(rb, nq, "query")) return rc;
    return run_search(idx, SearchRequest{queries, nq, k, queries_on_device != 0, out_on_device != 0, ICD_MODE_EXACT,
                                         outs_for(reweighted != 0, out_adj, out_raw, out_ids, out_levels), &rb, masks,
                                         reinterpret_cast<hipStream_t>(stream), nullptr, boost});
}

extern "C" {

int icd_index_search_range(icd_index *idx, const float *queries, int64_t nq, int32_t k, int32_t queries_on_device,
                           const float *radius, const float *range_filter, const float *after_scores, const int64_t *after_ids,
                           int32_t bounds_on_device, int32_t reweighted, double *out_adj, float *out_raw, int64_t *out_ids,
                           int32_t *out_levels, int32_t out_on_device, void *stream) {
    const RangeBounds rb{radius, range_filter, after_scores, reinterpret_cast<const long long *>(after_ids), bounds_on_device != 0};
    return search_banded(idx, nullptr, "range", queries, nq, k, queries_on_device, rb, reweighted, out_adj, out_raw, out_ids, out_levels,
                         out_on_device, stream);
}

int icd_rowmask_pack(const int64_t *rows, int64_t n_rows, int64_t n, uint32_t *out_words, int64_t out_count) {
    if (n <= 0 || n_rows < 0 || (n_rows > 0 && !rows) || !out_words) return fail(ICD_ERR_INVALID, "rows / out_words NULL, n=%lld or n_rows=%lld", (long long)n, (long long)n_rows);
    if (out_count < rowmask_tile_words(n)) return fail(ICD_ERR_INVALID, "out_count=%lld: %lld rows need %lld words", (long long)out_count, (long long)n, rowmask_tile_words(n));
    for (int64_t i = 0; i < n_rows; ++i) {   // (checked before anything is written)
        if (rows[i] < 0 || rows[i] >= n) return fail(ICD_ERR_INVALID, "rows[%lld]=%lld outside the index's [0, %lld)", (long long)i, (long long)rows[i], (long long)n);
        if (i > 0 && rows[i] <= rows[i - 1]) return fail(ICD_ERR_INVALID, "rows[%lld]=%lld: row ids must be strictly increasing", (long long)i, (long long)rows[i]);
    }
    memset(out_words, 0, (size_t)out_count * sizeof(uint32_t));
    for (int64_t i = 0; i < n_rows; ++i) out_words[rows[i] >> 5] |= 1u << (rows[i] & 31);
    return ICD_OK;
}

int icd_rowmask_create(icd_index *idx, const int64_t *rows, int64_t n_rows, int32_t rows_on_device, icd_rowmask **out) {
    if (!out) return fail(ICD_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!valid(idx)) return fail(ICD_ERR_STATE, "invalid handle");
    if (n_rows < 0 || (n_rows > 0 && !rows)) return fail(ICD_ERR_INVALID, "rows NULL or n_rows=%lld", (long long)n_rows);
    if (n_rows > idx->n) return fail(ICD_ERR_INVALID, "n_rows=%lld exceeds the index's %lld rows", (long long)n_rows, (long long)idx->n);
    if (idx->row_map) return fail(ICD_ERR_UNSUPPORTED, "row masks on a view are not supported: mask the parent");
    HIP_TRY(hipSetDevice(idx->device));
    const size_t words = (size_t)rowmask_tile_words(idx->n) + ROWMASK_TAIL_WORDS;
    std::vector<uint32_t> packed;
    if (!rows_on_device) {   // a host list: checked and packed here, one upload
        packed.resize(words);
        const int rcp = icd_rowmask_pack(rows, n_rows, idx->n, packed.data(), (int64_t)words);
        if (rcp) return rcp;
    }
    icd_rowmask *m = new_handle<icd_rowmask>(idx);
    if (!m) return fail(ICD_ERR_NOMEM, "host allocation failed");
    m->rows = n_rows; m->bytes = words * sizeof(uint32_t);
    int *derr = nullptr;
    int herr = 0;
    hipError_t e = m->alloc(&m->bits, words);
    if (e == hipSuccess && !rows_on_device) e = hipMemcpy(m->bits, packed.data(), words * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess && rows_on_device) {
        e = hipMemset(m->bits, 0, words * sizeof(uint32_t));
        if (e == hipSuccess && n_rows > 0) {
            e = dmalloc(&derr, 1);
            if (e == hipSuccess) e = hipMemset(derr, 0, sizeof(int));
            if (e == hipSuccess) {
                hipLaunchKernelGGL(rowmask_build_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, 0,
                                   reinterpret_cast<const long long *>(rows), (long long)n_rows, (long long)idx->n, m->bits, derr);
                e = hipGetLastError();
            }
            if (e == hipSuccess) e = hipMemcpy(&herr, derr, sizeof(int), hipMemcpyDeviceToHost);
            hipFree(derr);
        }
    }
    if (e != hipSuccess || herr) {
        free_handle(m);
        if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? ICD_ERR_NOMEM : ICD_ERR_HIP, "row mask: %s", hipGetErrorString(e));
        return fail(ICD_ERR_INVALID, "rows: row ids must be strictly increasing and inside the index's [0, %lld)", (long long)idx->n);
    }
    *out = m;
    return ICD_OK;
}

int icd_rowmask_destroy(icd_rowmask *m) {
    icd_rowmask::SharedBlock *b = valid_handle(m) ? m->block : nullptr;
    const int rc = destroy_handle(m);   // (synchronises the mask's device first)
    if (b && b->refs.fetch_sub(1) == 1) { hipFree(b->dev); delete b; }
    return rc;
}

int icd_rowmask_stats(icd_rowmask *m, int64_t *out_rows, int64_t *out_bytes) {
    if (!valid_handle(m)) return fail(ICD_ERR_STATE, "invalid row mask handle");
    if (m->rows < 0 && out_rows) {   // a produced mask: its kernel counted the rows; wait for it, once
        int cnt = 0;
        HIP_TRY(hipSetDevice(m->at.device));
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(&cnt, m->count_dev, sizeof(int), hipMemcpyDeviceToHost));
        m->rows = cnt;
    }
    if (out_rows) *out_rows = m->rows;
    if (out_bytes) *out_bytes = (int64_t)m->bytes;
    return ICD_OK;
}

int icd_rowmask_read(icd_rowmask *m, uint32_t *out_words, int64_t out_count) {
    if (!valid_handle(m)) return fail(ICD_ERR_STATE, "invalid row mask handle");
    const int64_t words = rowmask_tile_words(m->at.n);
    if (!out_words || out_count < words) return fail(ICD_ERR_INVALID, "out_words NULL or out_count=%lld: %lld rows need %lld words", (long long)out_count, (long long)m->at.n, (long long)words);
    HIP_TRY(hipSetDevice(m->at.device));
    HIP_TRY(hipDeviceSynchronize());   // (whatever stream the mask was built on)
    HIP_TRY(hipMemcpy(out_words, m->bits, (size_t)words * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return ICD_OK;
}

// ---- the ordered select over a batch of masks (mask_select_kernel.hpp) ---------------------------------------
// Its mask table keeps the NULL entries (the kernels count and walk "every row" without a bitset) and travels with the offsets:
// both through pinned blocks behind stage_masks' event, under the handle's mutex.
static int stage_select(icd_index *x, icd_rowmask *const *masks, const int64_t *offsets, int nq, hipStream_t s) {
    if (x->mask_copy_pending) { HIP_TRY(hipEventSynchronize(x->ev_mask)); x->mask_copy_pending = false; }
    for (int q = 0; q < nq; ++q) {
        x->h_mask[q] = masks[q] ? masks[q]->bits : nullptr;
        x->h_sel_off[q] = offsets ? (long long)offsets[q] : 0ll;
    }
    const hipError_t em = hipMemcpyAsync(x->mask_dev, x->h_mask, (size_t)nq * sizeof(uint32_t *), hipMemcpyHostToDevice, s);
    const hipError_t eo = hipMemcpyAsync(x->sel_off, x->h_sel_off, (size_t)nq * sizeof(long long), hipMemcpyHostToDevice, s);
    const hipError_t ee = hipEventRecord(x->ev_mask, s);   // (also behind a copy that failed to enqueue, as in stage_masks)
    x->mask_copy_pending = ee == hipSuccess;
    if (em != hipSuccess || eo != hipSuccess || ee != hipSuccess) {
        hipStreamSynchronize(s);
        x->mask_copy_pending = false;
        return fail(ICD_ERR_HIP, "select table: %s", hipGetErrorString(em != hipSuccess ? em : eo != hipSuccess ? eo : ee));
    }
    return ICD_OK;
}

int icd_rowmask_select(icd_index *idx, icd_rowmask *const *masks, int64_t nq, const int64_t *offsets, int32_t limit, int64_t *out_ids,
                       int64_t *out_total, int32_t *out_taken, int32_t out_on_device, void *stream) {
    static_assert(ICD_SELECT_MAX_LIMIT == MS_MAX_LIMIT, "include/icd_search.h and mask_select_plan.hpp disagree");
    if (limit < 1 || limit > ICD_SELECT_MAX_LIMIT) return fail(ICD_ERR_INVALID, "limit=%d: a select returns 1 .. %d rows per query", limit, ICD_SELECT_MAX_LIMIT);
    if (nq < 0) return fail(ICD_ERR_INVALID, "nq=%lld", (long long)nq);
    if (!out_total) return fail(ICD_ERR_INVALID, "out_total is NULL");
    if (out_ids && !out_taken) return fail(ICD_ERR_INVALID, "out_taken is NULL (out_ids without it cannot be read)");
    if (nq > 0 && !masks) return fail(ICD_ERR_INVALID, "masks is NULL");
    if (!valid(idx)) return fail(ICD_ERR_STATE, "invalid handle");
    bool any = false;
    if (const int rc = check_masks(idx, masks, nq, "row select", &any)) return rc;
    for (int64_t q = 0; offsets && q < nq; ++q)
        if (offsets[q] < 0) return fail(ICD_ERR_INVALID, "offsets[%lld]=%lld is negative", (long long)q, (long long)offsets[q]);
    const long long segments = ms_segments(idx->n);
    if (nq * segments > 0x7FFFFFFFll) return fail(ICD_ERR_INVALID, "nq=%lld: %lld segments of rows times nq exceed 2^31 - 1 work-groups", (long long)nq, segments);
    const size_t slots = (size_t)nq * (size_t)limit;
    if (!out_on_device && out_ids && slots > idx->sel_out_cap)
        return fail(ICD_ERR_INVALID, "nq=%lld x limit=%d: host outputs hold up to %lld ids per call (device outputs have no such bound)", (long long)nq, limit, (long long)idx->sel_out_cap);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (stream_capturing(s)) return fail(ICD_ERR_INVALID, "a row select stages its mask table on the host at call time: it cannot be captured into a graph");
    if (nq == 0) return ICD_OK;
    std::lock_guard<std::mutex> guard(idx->mu);
    HIP_TRY(hipSetDevice(idx->device));
    if (const int rc = stage_select(idx, masks, offsets, (int)nq, s)) return rc;
    const bool host = !out_on_device;
    MaskSelectArgs a{};
    a.masks = idx->mask_dev; a.offsets = idx->sel_off; a.counts = idx->sel_counts;
    a.ids = reinterpret_cast<long long *>(out_ids && host ? reinterpret_cast<int64_t *>(idx->sel_ids) : out_ids);
    a.total = host ? idx->sel_total : reinterpret_cast<long long *>(out_total);
    a.taken = out_taken && host ? idx->sel_taken : out_taken;
    a.n = idx->n; a.mask_words = rowmask_tile_words(idx->n); a.segments = (int)segments; a.limit = limit;
    const dim3 grid((unsigned)(nq * segments));
    hipLaunchKernelGGL(mask_count_kernel, grid, dim3(MS_THREADS), 0, s, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(mask_select_kernel, grid, dim3(MS_THREADS), 0, s, a);
    HIP_TRY(hipGetLastError());
    if (!host) return ICD_OK;
    if (out_ids) HIP_TRY(hipMemcpyAsync(out_ids, idx->sel_ids, slots * sizeof(long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out_total, idx->sel_total, (size_t)nq * sizeof(long long), hipMemcpyDeviceToHost, s));
    if (out_taken) HIP_TRY(hipMemcpyAsync(out_taken, idx->sel_taken, (size_t)nq * sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return ICD_OK;
}

// A NULL table or an all-NULL table is the range search (which the all-NULL table equals bit for bit), under its name.
int icd_index_search_masked(icd_index *idx, icd_rowmask *const *masks, const float *queries, int64_t nq, int32_t k, int32_t queries_on_device,
                            const float *radius, const float *range_filter, const float *after_scores, const int64_t *after_ids,
                            int32_t bounds_on_device, int32_t reweighted, double *out_adj, float *out_raw, int64_t *out_ids,
                            int32_t *out_levels, int32_t out_on_device, void *stream) {
    bool any = false;
    if (masks) {
        if (!valid(idx)) return fail(ICD_ERR_STATE, "invalid handle");
        if (const int rc = check_masks(idx, masks, nq, "masked search", &any)) return rc;
    }
    const RangeBounds rb{radius, range_filter, after_scores, reinterpret_cast<const long long *>(after_ids), bounds_on_device != 0};
    return search_banded(idx, any ? masks : nullptr, any ? "masked" : "range", queries, nq, k, queries_on_device, rb, reweighted, out_adj,
                         out_raw, out_ids, out_levels, out_on_device, stream);
}

}  // extern "C"
