// icd_hybrid.hpp - the hybrid search (icd_fusion_*, icd_index_search_hybrid), the fuse of caller-provided lists (icd_fusion_fuse_lists)
// and their grouped forms. Part of icd_search.hip's translation unit (fail(), HIP_TRY, the owned-handle, request and host-call
// helpers, run_search, the grouping); included there and nowhere else.
#pragma once

// ---- hybrid search (hybrid_fuse.hpp) -----------------------------------------------------------------
// A fusion belongs to the index it was created for but keeps no pointer into it: handle and identity are compared, never
// followed. Its workspace - the staging of the sub-lists, the staging of host callers - is allocated here, never in a search.
struct icd_fusion : OwnedHandle {
    static constexpr uint32_t MAGIC = 0x1CDF05EDu;
    static constexpr const char *NOUN = "fusion";
    int64_t max_total = 0;
    float *st_scores = nullptr; long long *st_ids = nullptr;   // [max_total][ICD_MAX_K] the sub-lists of a call, [nq * R][max limit] used
    float *qdev = nullptr;                                     // [max_total][dim] a host caller's vectors
    double *o_adj = nullptr, *o_fused = nullptr; long long *o_ids = nullptr; int *o_lv = nullptr; uint32_t *o_bits = nullptr;   // [FUSION_HOST_CHUNK][ICD_MAX_K] a host caller's outputs, FUSION_HOST_CHUNK queries at a time
    int limits[ICD_MAX_REQUESTS] = {};                         // of the current call (copied: the caller's arrays are not read again)
    double weights[ICD_MAX_REQUESTS] = {};
    std::mutex mu;
};

namespace {
// a HOST caller's outputs leave the device in pieces of this many queries (one fuse launch and its copies per piece, in stream
// order through one staging block of 256 x 128 slots = 1 MB): the staging does not grow with max_total, and a device caller,
// who never uses it, does not pay for it
constexpr int FUSION_HOST_CHUNK = 256;
}  // namespace

// Step 2 of a hybrid search: ONE launch of hybrid_fuse_kernel over the [nq * R][lmax] sub-lists at st_scores / st_ids (device memory;
// the fusion's staging, or a caller's lists: icd_fusion_fuse_lists), limits and weights taken from the fusion, where the caller
// has put them. Host outputs leave through the fusion's staging, FUSION_HOST_CHUNK queries at a time.
static int fuse_lists_step(icd_index *idx, icd_fusion *f, const float *st_scores, const long long *st_ids, int64_t nq, int32_t R, int lmax,
                           int32_t ranker, double rrf_c, int32_t norm, int32_t k, int32_t reweighted, double *out_adj, double *out_fused,
                           int64_t *out_ids, int32_t *out_levels, uint32_t *out_reqbits, const HostCall &hc, hipStream_t s,
                           icd_grouping *grp = nullptr, int group_size = 1, int32_t *out_groups = nullptr) {
    int rc;
    // grouped (grp != nullptr): hybrid_fuse_grouped_kernel, k groups of group_size members, k * group_size slots per query, the
    // hits' group ids as one more output (a host caller's through the grouping's staging)
    const int kk = grp ? k * group_size : k;
    HybridGroupedArgs ga{};
    HybridArgs &a = ga.h;
    a.st_scores = st_scores; a.st_ids = st_ids;
    a.R = R; a.lmax = lmax; a.k = k;
    a.slots = 2;
    while (a.slots < R * lmax) a.slots <<= 1;
    for (int r = 0; r < HY_MAX_R; ++r) { a.limits[r] = f->limits[r]; a.weights[r] = f->weights[r]; }
    a.rrf_c = rrf_c; a.ranker = ranker; a.norm = norm; a.reweighted = reweighted ? 1 : 0;
    a.n = idx->n; a.id_base = idx->id_base; a.row_map = idx->row_map; a.levels = idx->levels;
    a.out_adj = out_adj; a.out_fused = out_fused; a.out_ids = reinterpret_cast<long long *>(out_ids); a.out_levels = out_levels; a.out_reqbits = out_reqbits;
    if (grp) { ga.dense_of = grp->dense_of; ga.group_of = grp->group_of; ga.s = group_size; ga.out_groups = out_groups; }
    auto launch = [&](int64_t nb) {
        if (grp) hipLaunchKernelGGL(hybrid_fuse_grouped_kernel, dim3((unsigned)nb), dim3(HY_THREADS), 0, s, ga);
        else hipLaunchKernelGGL(hybrid_fuse_kernel, dim3((unsigned)nb), dim3(HY_THREADS), 0, s, a);
        return hipGetLastError();
    };
    if (hc.out_on_device) {
        HIP_TRY(launch(nq));
    } else {
        // host outputs: FUSION_HOST_CHUNK queries per launch into the staging, copied out behind it (stream order keeps the
        // next piece's launch behind this piece's copies)
        a.out_adj = reweighted ? f->o_adj : nullptr; a.out_fused = f->o_fused; a.out_ids = f->o_ids;
        a.out_levels = out_levels ? f->o_lv : nullptr; a.out_reqbits = out_reqbits ? f->o_bits : nullptr;
        if (grp) ga.out_groups = out_groups ? grp->o_grp : nullptr;   // (a piece is at most FUSION_HOST_CHUNK <= nq <= the grouping's max_nq queries)
        for (int64_t q0 = 0; q0 < nq; q0 += FUSION_HOST_CHUNK) {
            const int64_t nb = std::min<int64_t>(FUSION_HOST_CHUNK, nq - q0);
            a.st_scores = st_scores + (size_t)q0 * R * lmax;
            a.st_ids = st_ids + (size_t)q0 * R * lmax;
            HIP_TRY(launch(nb));
            const size_t at = (size_t)q0 * kk;
            if ((rc = hc.copy_back({{reweighted ? out_adj + at : nullptr, a.out_adj, 8}, {out_fused + at, a.out_fused, 8}, {out_ids + at, a.out_ids, 8},
                                    {out_levels ? out_levels + at : nullptr, a.out_levels, 4}, {out_reqbits ? out_reqbits + at : nullptr, a.out_reqbits, 4},
                                    {out_groups ? out_groups + at : nullptr, ga.out_groups, 4}},
                                   (size_t)nb * kk)))
                return rc;
        }
    }
    return ICD_OK;
}

// The ranker's rules, the same for every fuse entry point: rrf_c in (0, 16384); R weights in [0, 1] and one of the three norms.
static int check_fuse_ranker(int32_t R, int32_t ranker, double rrf_c, const double *weights, int32_t norm) {
    if (ranker == ICD_RANKER_RRF) {
        if (!(rrf_c > 0.0 && rrf_c < 16384.0)) return fail(ICD_ERR_INVALID, "rrf_c=%g: need 0 < c < 16384", rrf_c);
    } else if (ranker == ICD_RANKER_WEIGHTED) {
        if (!weights) return fail(ICD_ERR_INVALID, "weights is NULL");
        for (int r = 0; r < R; ++r)
            if (!(weights[r] >= 0.0 && weights[r] <= 1.0)) return fail(ICD_ERR_INVALID, "weights[%d]=%g: a weight lies in [0, 1]", r, weights[r]);
        if (norm != ICD_NORM_NONE && norm != ICD_NORM_COSINE && norm != ICD_NORM_ATAN) return fail(ICD_ERR_INVALID, "norm=%d", norm);
    } else {
        return fail(ICD_ERR_INVALID, "ranker=%d", ranker);
    }
    return ICD_OK;
}

// limits and weights of the current call into the fusion, where fuse_lists_step reads them (under the fusion's mutex)
static void stage_fuse_params(icd_fusion *f, int32_t R, const int32_t *limits, int32_t ranker, const double *weights) {
    for (int r = 0; r < ICD_MAX_REQUESTS; ++r) {
        f->limits[r] = r < R ? limits[r] : 0;
        f->weights[r] = (r < R && ranker == ICD_RANKER_WEIGHTED) ? weights[r] : 0.0;
    }
}

extern "C" {

int icd_fusion_create(icd_index *idx, int64_t max_total, icd_fusion **out) {
    if (!out) return fail(ICD_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!valid(idx)) return fail(ICD_ERR_STATE, "invalid handle");
    if (max_total <= 0 || max_total > 0x7FFFFFFFll / ICD_MAX_K) return fail(ICD_ERR_INVALID, "max_total=%lld", (long long)max_total);
    if (idx->n >= 0x7FFFFFFFll) return fail(ICD_ERR_UNSUPPORTED, "n=%lld: a fusion addresses rows with 31 bits", (long long)idx->n);
    HIP_TRY(hipSetDevice(idx->device));
    icd_fusion *f = new_handle<icd_fusion>(idx);
    if (!f) return fail(ICD_ERR_NOMEM, "host allocation failed");
    f->max_total = max_total;
    const size_t no = (size_t)max_total * ICD_MAX_K;
#define FU_TRY(expr) HIP_TRY_OR(free_handle(f), expr)
    FU_TRY(f->alloc(&f->st_scores, no)); FU_TRY(f->alloc(&f->st_ids, no));
    FU_TRY(f->alloc(&f->qdev, (size_t)max_total * idx->dim));
    const size_t nh = (size_t)std::min<int64_t>(max_total, FUSION_HOST_CHUNK) * ICD_MAX_K;
    FU_TRY(f->alloc(&f->o_adj, nh)); FU_TRY(f->alloc(&f->o_fused, nh)); FU_TRY(f->alloc(&f->o_ids, nh)); FU_TRY(f->alloc(&f->o_lv, nh)); FU_TRY(f->alloc(&f->o_bits, nh));
#undef FU_TRY
    f->bytes = no * (4 + 8) + (size_t)max_total * idx->dim * 4 + nh * (8 + 8 + 8 + 4 + 4);
    *out = f;
    return ICD_OK;
}

int icd_fusion_destroy(icd_fusion *fusion) { return destroy_handle(fusion); }

int icd_fusion_stats(icd_fusion *fusion, int64_t *out_max_total, int64_t *out_bytes) {
    if (!valid_handle(fusion)) return fail(ICD_ERR_STATE, "invalid fusion handle");
    if (out_max_total) *out_max_total = fusion->max_total;
    if (out_bytes) *out_bytes = (int64_t)fusion->bytes;
    return ICD_OK;
}

int icd_index_search_hybrid(icd_index *idx, icd_fusion *fusion, const float *queries, int64_t nq, int32_t R, int32_t queries_on_device,
                            const int32_t *limits, icd_rowmask *const *masks, const float *radius, const float *range_filter,
                            int32_t bounds_on_device, int32_t mode, int32_t ranker, double rrf_c, const double *weights, int32_t norm,
                            int32_t k, int32_t reweighted, double *out_adj, double *out_fused, int64_t *out_ids, int32_t *out_levels,
                            uint32_t *out_reqbits, int32_t out_on_device, void *stream) {
    // every check comes before the first device call
    if (!valid(idx)) return fail(ICD_ERR_STATE, "invalid handle");
    if (!valid_handle(fusion)) return fail(ICD_ERR_STATE, "invalid fusion handle");
    icd_fusion *f = fusion;
    int rc = check_owner(f->at, idx, "the fusion");
    if (rc) return rc;
    if (R < 1 || R > ICD_MAX_REQUESTS) return fail(ICD_ERR_INVALID, "R=%d: a hybrid search takes 1 .. %d requests per query", R, ICD_MAX_REQUESTS);
    if (k < 1 || k > ICD_MAX_K) return fail(ICD_ERR_INVALID, "k=%d: a hybrid search returns 1 .. %d hits per query", k, ICD_MAX_K);
    if (!limits) return fail(ICD_ERR_INVALID, "limits is NULL");
    int lmax = 0;
    for (int r = 0; r < R; ++r) {
        if (limits[r] < 1 || limits[r] > ICD_MAX_K) return fail(ICD_ERR_INVALID, "limits[%d]=%d: a request returns 1 .. %d hits", r, limits[r], ICD_MAX_K);
        lmax = std::max(lmax, (int)limits[r]);
    }
    if (lmax > idx->max_k) return fail(ICD_ERR_INVALID, "limit %d exceeds the index's max_k=%d", lmax, idx->max_k);
    if (nq < 0) return fail(ICD_ERR_INVALID, "nq=%lld", (long long)nq);
    const int64_t total = nq * R;
    if (total > f->max_total) return fail(ICD_ERR_INVALID, "nq * R = %lld exceeds the fusion's max_total=%lld", (long long)total, (long long)f->max_total);
    if (total > idx->max_nq) return fail(ICD_ERR_INVALID, "nq * R = %lld exceeds the index's max_nq=%d", (long long)total, idx->max_nq);
    if (mode != ICD_MODE_AUTO && mode != ICD_MODE_EXACT) return fail(ICD_ERR_INVALID, "mode=%d", mode);
    if ((rc = check_fuse_ranker(R, ranker, rrf_c, weights, norm))) return rc;
    if (!out_fused || !out_ids || (reweighted && !out_adj)) return fail(ICD_ERR_INVALID, "output pointer is NULL");
    const bool banded = radius || range_filter;
    const RangeBounds rb{radius, range_filter, nullptr, nullptr, bounds_on_device != 0};
    if ((rc = check_bands(rb, total, "sub-search"))) return rc;
    bool any_mask = false;
    if (masks && (rc = check_masks(idx, masks, total, "masked hybrid search", &any_mask))) return rc;
    if (nq == 0) return ICD_OK;
    if (!queries) return fail(ICD_ERR_INVALID, "queries is NULL");
    std::lock_guard<std::mutex> guard(f->mu);
    HIP_TRY(hipSetDevice(idx->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const HostCall hc{s, queries_on_device != 0, out_on_device != 0};
    bool capturing;
    if ((rc = check_capture(s, !queries_on_device || !out_on_device, banded && !bounds_on_device, masks != nullptr, &capturing))) return rc;
    stage_fuse_params(f, R, limits, ranker, weights);
    const float *dq;
    if ((rc = hc.upload(queries, f->qdev, (size_t)total * idx->dim, &dq))) return rc;
    // step 1 (its capture checks are the ones made above): ONE sub-search over the nq * R vectors at k = the largest limit, into the staging: the plain search in the caller's
    // mode when there is neither a mask table nor a band, else the banded EXACT search (with the table when it holds a mask)
    const bool plain = !masks && !banded;
    rc = run_search(idx, SearchRequest{dq, total, lmax, true, true, plain ? mode : ICD_MODE_EXACT,
                                       outs_for(false, nullptr, f->st_scores, reinterpret_cast<int64_t *>(f->st_ids), nullptr),
                                       plain ? nullptr : &rb, any_mask ? masks : nullptr, s, &capturing});
    if (rc) return rc;
    // step 2: the fuse
    if ((rc = fuse_lists_step(idx, f, f->st_scores, f->st_ids, nq, R, lmax, ranker, rrf_c, norm, k, reweighted, out_adj, out_fused, out_ids,
                              out_levels, out_reqbits, hc, s)))
        return rc;
    return hc.finish();
}

}  // extern "C"

// ---- grouped hybrid search (rules H1 - H6) -----------------------------------------------------------------
// the checks the two grouped entry points share (section 13's and section 10's), before the first device call; *lmax_groups: max L_r
static int check_grouped_fuse(icd_index *idx, icd_fusion *f, icd_grouping *g, int64_t nq, int32_t R, const int32_t *limits, int32_t ranker,
                              double rrf_c, const double *weights, int32_t norm, int32_t k, int32_t group_size, int32_t reweighted,
                              const double *out_adj, const double *out_fused, const int64_t *out_ids, int *lmax_groups) {
    if (!valid(idx)) return fail(ICD_ERR_STATE, "invalid handle");
    if (!valid_handle(f)) return fail(ICD_ERR_STATE, "invalid fusion handle");
    if (!valid_handle(g)) return fail(ICD_ERR_STATE, "invalid grouping handle");
    int rc = check_owner(f->at, idx, "the fusion");
    if (rc) return rc;
    if ((rc = check_owner(g->at, idx, "the grouping"))) return rc;
    if (R < 1 || R > ICD_MAX_REQUESTS) return fail(ICD_ERR_INVALID, "R=%d: a hybrid search takes 1 .. %d requests per query", R, ICD_MAX_REQUESTS);
    if (k < 1 || group_size < 1 || (int64_t)k * group_size > ICD_MAX_K)
        return fail(ICD_ERR_INVALID, "k=%d group_size=%d: need k >= 1, group_size >= 1 and k * group_size <= %d", k, group_size, ICD_MAX_K);
    if (!limits) return fail(ICD_ERR_INVALID, "limits is NULL");
    int lmax = 0;
    for (int r = 0; r < R; ++r) {
        if (limits[r] < 1 || (int64_t)limits[r] * group_size > ICD_MAX_K)
            return fail(ICD_ERR_INVALID, "limits[%d]=%d group_size=%d: a request returns 1 .. %d / group_size groups", r, limits[r], group_size, ICD_MAX_K);
        lmax = std::max(lmax, (int)limits[r]);
    }
    *lmax_groups = lmax;
    if (nq < 0) return fail(ICD_ERR_INVALID, "nq=%lld", (long long)nq);
    if (nq * R > f->max_total) return fail(ICD_ERR_INVALID, "nq * R = %lld exceeds the fusion's max_total=%lld", (long long)(nq * R), (long long)f->max_total);
    if (nq * R > g->max_nq) return fail(ICD_ERR_INVALID, "nq * R = %lld exceeds the grouping's max_nq=%d", (long long)(nq * R), g->max_nq);
    if ((rc = check_fuse_ranker(R, ranker, rrf_c, weights, norm))) return rc;
    if (!out_fused || !out_ids || (reweighted && !out_adj)) return fail(ICD_ERR_INVALID, "output pointer is NULL");
    return ICD_OK;
}

extern "C" {

int icd_fusion_fuse_lists(icd_index *idx, icd_fusion *fusion, const float *scores, const int64_t *ids, int64_t nq, int32_t R, int32_t lmax,
                          const int32_t *limits, int32_t ranker, double rrf_c, const double *weights, int32_t norm, int32_t k,
                          int32_t reweighted, double *out_adj, double *out_fused, int64_t *out_ids, int32_t *out_levels,
                          uint32_t *out_reqbits, int32_t out_on_device, void *stream) {
    // the checks of icd_index_search_hybrid that concern its step 2, before the first device call
    if (!valid(idx)) return fail(ICD_ERR_STATE, "invalid handle");
    if (!valid_handle(fusion)) return fail(ICD_ERR_STATE, "invalid fusion handle");
    icd_fusion *f = fusion;
    int rc = check_owner(f->at, idx, "the fusion");
    if (rc) return rc;
    if (R < 1 || R > ICD_MAX_REQUESTS) return fail(ICD_ERR_INVALID, "R=%d: a hybrid search takes 1 .. %d requests per query", R, ICD_MAX_REQUESTS);
    if (k < 1 || k > ICD_MAX_K) return fail(ICD_ERR_INVALID, "k=%d: a hybrid search returns 1 .. %d hits per query", k, ICD_MAX_K);
    if (lmax < 1 || lmax > ICD_MAX_K) return fail(ICD_ERR_INVALID, "lmax=%d: a list holds 1 .. %d hits", lmax, ICD_MAX_K);
    if (!limits) return fail(ICD_ERR_INVALID, "limits is NULL");
    for (int r = 0; r < R; ++r)
        if (limits[r] < 1 || limits[r] > lmax) return fail(ICD_ERR_INVALID, "limits[%d]=%d: a request returns 1 .. lmax=%d hits", r, limits[r], lmax);
    if (nq < 0) return fail(ICD_ERR_INVALID, "nq=%lld", (long long)nq);
    if (nq * R > f->max_total) return fail(ICD_ERR_INVALID, "nq * R = %lld exceeds the fusion's max_total=%lld", (long long)(nq * R), (long long)f->max_total);
    if ((rc = check_fuse_ranker(R, ranker, rrf_c, weights, norm))) return rc;
    if (!out_fused || !out_ids || (reweighted && !out_adj)) return fail(ICD_ERR_INVALID, "output pointer is NULL");
    if (nq == 0) return ICD_OK;
    if (!scores || !ids) return fail(ICD_ERR_INVALID, "scores / ids NULL");
    std::lock_guard<std::mutex> guard(f->mu);
    HIP_TRY(hipSetDevice(idx->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const HostCall hc{s, true, out_on_device != 0};
    if ((rc = check_capture(s, !out_on_device, false, false))) return rc;
    stage_fuse_params(f, R, limits, ranker, weights);
    if ((rc = fuse_lists_step(idx, f, scores, reinterpret_cast<const long long *>(ids), nq, R, lmax, ranker, rrf_c, norm, k, reweighted, out_adj,
                              out_fused, out_ids, out_levels, out_reqbits, hc, s)))
        return rc;
    return hc.finish();
}

int icd_fusion_fuse_lists_grouped(icd_index *idx, icd_fusion *fusion, icd_grouping *grouping, const float *scores, const int64_t *ids, int64_t nq,
                                  int32_t R, int32_t lmax, const int32_t *limits, int32_t ranker, double rrf_c, const double *weights, int32_t norm,
                                  int32_t k, int32_t group_size, int32_t reweighted, double *out_adj, double *out_fused, int64_t *out_ids,
                                  int32_t *out_levels, uint32_t *out_reqbits, int32_t *out_groups, int32_t out_on_device, void *stream) {
    int lg = 0;
    int rc = check_grouped_fuse(idx, fusion, grouping, nq, R, limits, ranker, rrf_c, weights, norm, k, group_size, reweighted, out_adj, out_fused, out_ids, &lg);
    if (rc) return rc;
    if (lmax < 1 || lmax > ICD_MAX_K) return fail(ICD_ERR_INVALID, "lmax=%d: a list holds 1 .. %d hits", lmax, ICD_MAX_K);
    if (nq == 0) return ICD_OK;
    if (!scores || !ids) return fail(ICD_ERR_INVALID, "scores / ids NULL");
    // lock order: fusion, grouping, index
    std::lock_guard<std::mutex> guard(fusion->mu);
    std::lock_guard<std::mutex> guard_g(grouping->mu);
    HIP_TRY(hipSetDevice(idx->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const HostCall hc{s, true, out_on_device != 0};
    if ((rc = check_capture(s, !out_on_device, false, false))) return rc;
    stage_fuse_params(fusion, R, limits, ranker, weights);
    if ((rc = fuse_lists_step(idx, fusion, scores, reinterpret_cast<const long long *>(ids), nq, R, lmax, ranker, rrf_c, norm, k, reweighted, out_adj,
                              out_fused, out_ids, out_levels, out_reqbits, hc, s, grouping, group_size, out_groups)))
        return rc;
    return hc.finish();
}

int icd_index_search_hybrid_grouped(icd_index *idx, icd_fusion *fusion, icd_grouping *grouping, const float *queries, int64_t nq, int32_t R,
                                    int32_t queries_on_device, const int32_t *limits, icd_rowmask *const *masks, const float *radius,
                                    const float *range_filter, int32_t ranker, double rrf_c, const double *weights, int32_t norm, int32_t k,
                                    int32_t group_size, int32_t reweighted, double *out_adj, double *out_fused, int64_t *out_ids,
                                    int32_t *out_levels, uint32_t *out_reqbits, int32_t *out_groups, int32_t out_on_device, void *stream) {
    int lg = 0;
    int rc = check_grouped_fuse(idx, fusion, grouping, nq, R, limits, ranker, rrf_c, weights, norm, k, group_size, reweighted, out_adj, out_fused, out_ids, &lg);
    if (rc) return rc;
    if (masks || radius || range_filter)
        return fail(ICD_ERR_INVALID, "row masks and radius / range_filter cannot be combined with grouping (filter with a view and its grouping)");
    if (nq == 0) return ICD_OK;
    if (!queries) return fail(ICD_ERR_INVALID, "queries is NULL");
    icd_fusion *f = fusion;
    std::lock_guard<std::mutex> guard(f->mu);
    std::lock_guard<std::mutex> guard_g(grouping->mu);
    HIP_TRY(hipSetDevice(idx->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const HostCall hc{s, queries_on_device != 0, out_on_device != 0};
    if ((rc = check_capture(s, !queries_on_device || !out_on_device, false, false))) return rc;
    stage_fuse_params(f, R, limits, ranker, weights);
    const int64_t total = nq * R;
    const float *dq;
    if ((rc = hc.upload(queries, f->qdev, (size_t)total * idx->dim, &dq))) return rc;
    // step 1: ONE grouped sub-search over the nq * R vectors at max L_r groups of group_size members, raw form, into the staging
    if ((rc = grouped_search_device(idx, grouping, dq, total, lg, group_size, false, GroupedOuts{nullptr, f->st_scores, f->st_ids, nullptr, nullptr}, s)))
        return rc;
    // step 2: the grouped fuse; list r is cut in front of its (L_r + 1)-th group
    if ((rc = fuse_lists_step(idx, f, f->st_scores, f->st_ids, nq, R, lg * group_size, ranker, rrf_c, norm, k, reweighted, out_adj, out_fused, out_ids,
                              out_levels, out_reqbits, hc, s, grouping, group_size, out_groups)))
        return rc;
    return hc.finish();
}

}  // extern "C"
