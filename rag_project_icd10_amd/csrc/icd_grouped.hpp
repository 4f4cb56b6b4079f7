// icd_grouped.hpp - the grouping search (icd_grouping_*, icd_index_search_grouped). Part of icd_search.hip's translation unit (fail(),
// HIP_TRY, the owned-handle and host-call helpers); included there and nowhere else.
#pragma once

// ---- grouping search (group_topk.hpp) ----------------------------------------------------------------
// A grouping belongs to the index it was created for (n rows, the same device) but keeps no pointer into it: the handle is
// compared, never followed, outside a search that is given both. Its workspace - the score block S, the per-group keys, the
// staging of host callers - is allocated here, never inside a search.
struct icd_grouping : OwnedHandle {
    static constexpr uint32_t MAGIC = 0x1CD96B0Fu;
    static constexpr const char *NOUN = "grouping";
    int G = 0, largest = 0, max_nq = 0, qb = 0;
    bool on_view = false;   // created for a view: its rows are the view's, not the parent's (no mask addresses them)
    long long ldS = 0;
    int *group_of = nullptr, *dense_of = nullptr, *order = nullptr, *gpos = nullptr, *seg = nullptr;
    int *pos_of = nullptr;   // [n] the inverse of `order`; built by icd_grouping_pair_sparse, absent before
    float *S = nullptr;
    u64 *best = nullptr;
    float *qdev = nullptr;
    double *o_adj = nullptr; float *o_raw = nullptr; long long *o_ids = nullptr; int *o_lv = nullptr, *o_grp = nullptr;
    // the group scorers (icd_grouping_prepare_scorers; group_aggregate_plan.hpp), absent before: the plan, and a host caller's
    // group scores and ids [max_nq][ICD_MAX_K]
    bool scorers = false;
    int npacks = 0, nlong = 0;
    GaPack *packs = nullptr; int *long_groups = nullptr;
    float *o_gscore = nullptr; int *o_gid = nullptr;
    // the embedding-list search (icd_grouping_prepare_maxsim; icd_maxsim.hpp), absent before: the lists' aggregates
    // [min(ms_lists, qb)][G], and a host caller's vectors [ms_vectors][dim], group outputs [ms_lists][ICD_MAX_K] and match outputs
    // [ms_vectors][ICD_MAX_K]
    int64_t ms_lists = 0, ms_vectors = 0;
    u64 *ms_agg = nullptr; float *ms_q = nullptr;
    float *ms_gscore = nullptr; int *ms_gid = nullptr;
    float *ms_mscore = nullptr; long long *ms_mid = nullptr; int *ms_mlv = nullptr;
    std::mutex mu;
};

namespace {
constexpr int GROUP_QUERY_BLOCK = 512;   // queries scored per pass: S = 512 x 40 576 x 4 B = 83 MB stays in the 256-MiB Infinity Cache next to the 124-MB corpus
}  // namespace

// where a grouped search writes: the reweighted form fills all five, the raw form all but d_adj
// (d_gscore / d_gid: the winning groups' own scores and ids of the scored entry point, null everywhere else)
struct GroupedOuts { double *d_adj; float *d_raw; long long *d_ids; int *d_lv, *d_grp; float *d_gscore; int *d_gid; };

// Steps 2 and 3 of a grouped search for ONE pass of nb <= g->qb queries whose scores of all rows sit in g->S (queries q0 .. of
// the call): group_best_kernel, group_finish_kernel. Whoever filled S - the dense scoring pass or the sparse store - calls this.
// Step 2 for the scorers SUM / AVG (group_aggregate_kernel.hpp) in group_best_kernel's place: the packs' launch and the long
// groups' launch write every cell of g->best between them, so nothing is zeroed in front. The grouping is prepared (checked by
// the entry point).
static int grouped_aggregate_pass(icd_grouping *g, int nb, int group_size, int scorer, hipStream_t s) {
    GroupAggArgs aa{};
    aa.S = g->S; aa.ldS = g->ldS; aa.order = g->order; aa.gpos = g->gpos; aa.seg = g->seg;
    aa.packs = g->packs; aa.long_groups = g->long_groups; aa.npacks = g->npacks; aa.nlong = g->nlong;
    aa.nq = nb; aa.G = g->G; aa.s = group_size; aa.avg = scorer == ICD_GROUP_SCORER_AVG ? 1 : 0; aa.best = g->best;
    if (g->npacks > 0) {
        hipLaunchKernelGGL(group_aggregate_pack_kernel, dim3((unsigned)ga_pack_blocks(g->npacks, nb)), dim3(64 * GA_WAVES), 0, s, aa);
        HIP_TRY(hipGetLastError());
    }
    if (g->nlong > 0) {
        const dim3 grid((unsigned)ga_long_blocks(g->nlong, nb));
        if (group_size <= 16) hipLaunchKernelGGL((group_aggregate_long_kernel<16, 2>), grid, dim3(64 * GA_WAVES), 0, s, aa);
        else hipLaunchKernelGGL((group_aggregate_long_kernel<128, 4>), grid, dim3(64 * GA_WAVES), 0, s, aa);
        HIP_TRY(hipGetLastError());
    }
    return ICD_OK;
}

// Step 1 for nb <= g->qb query vectors at dq: their scores of all rows -> g->S
static int grouped_scores_pass(icd_index *idx, icd_grouping *g, const float *dq, int nb, hipStream_t s) {
    GroupScoreArgs sa{};
    sa.corpus = idx->corpus; sa.queries = dq; sa.order = g->order;
    sa.nq = nb; sa.n = (int)g->at.n; sa.dim = idx->dim; sa.mtiles = (nb + GROUP_TILE - 1) / GROUP_TILE;
    sa.S = g->S; sa.ldS = g->ldS;
    hipLaunchKernelGGL(group_scores_kernel, dim3((unsigned)((int)(g->ldS / GROUP_TILE) * sa.mtiles)), dim3(256), 0, s, sa);
    HIP_TRY(hipGetLastError());
    return ICD_OK;
}

// Step 2 for the scorer MAX: g->best zeroed, then group_best_kernel over g->S
static int grouped_best_pass(icd_grouping *g, int nb, hipStream_t s) {
    const int n = (int)g->at.n;
    HIP_TRY(hipMemsetAsync(g->best, 0, (size_t)nb * g->G * sizeof(u64), s));
    GroupBestArgs ba{};
    ba.S = g->S; ba.ldS = g->ldS; ba.order = g->order; ba.gpos = g->gpos; ba.seg = g->seg;
    ba.nq = nb; ba.n = n; ba.G = g->G; ba.best = g->best;
    ba.R = nb >= 64 ? 1024 : 128;
    ba.nranges = (n + ba.R - 1) / ba.R;
    constexpr int QW = 4;
    const long long waves = (long long)((nb + QW - 1) / QW) * ba.nranges;
    hipLaunchKernelGGL(group_best_kernel<QW>, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, ba);
    HIP_TRY(hipGetLastError());
    return ICD_OK;
}

static int grouped_reduce_pass(icd_index *idx, icd_grouping *g, int nb, int64_t q0, int k, int group_size, bool reweighted, const GroupedOuts &o,
                               hipStream_t s, int scorer = ICD_GROUP_SCORER_MAX) {
    if (scorer != ICD_GROUP_SCORER_MAX) {
        if (const int rc = grouped_aggregate_pass(g, nb, group_size, scorer, s)) return rc;
    } else if (const int rc = grouped_best_pass(g, nb, s)) return rc;

    GroupFinishArgs fa{};
    fa.best = g->best; fa.S = g->S; fa.ldS = g->ldS; fa.order = g->order; fa.seg = g->seg; fa.dense_of = g->dense_of;
    fa.nq = nb; fa.G = g->G; fa.k = k; fa.s = group_size; fa.q_base = (int)q0;
    fa.fin.k = k * group_size; fa.fin.levels = idx->levels; fa.fin.id_base = idx->id_base; fa.fin.row_map = idx->row_map; fa.fin.groups = g->group_of;
    if (reweighted) {
        fa.fin.out_adj = o.d_adj; fa.fin.out_adj_raw = o.d_raw; fa.fin.out_adj_ids = o.d_ids; fa.fin.out_adj_levels = o.d_lv; fa.fin.out_adj_groups = o.d_grp;
    } else {
        fa.fin.out_scores = o.d_raw; fa.fin.out_ids = o.d_ids; fa.fin.out_levels = o.d_lv; fa.fin.out_groups = o.d_grp;
    }
    fa.out_group_scores = o.d_gscore; fa.out_group_ids = o.d_gid;
    const bool gs = o.d_gscore || o.d_gid;   // (the instantiations without them are the kernels every other caller launches)
    const dim3 grid((unsigned)((nb + 3) / 4));
    if (k <= 16 && group_size <= 16) {
        if (gs) hipLaunchKernelGGL((group_finish_kernel<16, 2, true>), grid, dim3(256), 0, s, fa);
        else hipLaunchKernelGGL((group_finish_kernel<16, 2>), grid, dim3(256), 0, s, fa);
    } else {
        if (gs) hipLaunchKernelGGL((group_finish_kernel<128, 4, true>), grid, dim3(256), 0, s, fa);
        else hipLaunchKernelGGL((group_finish_kernel<128, 4>), grid, dim3(256), 0, s, fa);
    }
    HIP_TRY(hipGetLastError());
    return ICD_OK;
}

// icd_index_search_grouped's body for device queries and device outputs: per pass of the grouping's query block the scoring pass
// and the reduction. The hybrid grouped search runs it on the fusion's staged vectors. The caller holds the grouping's lock.
static int grouped_search_device(icd_index *idx, icd_grouping *g, const float *dq, int64_t nq, int k, int group_size, bool reweighted,
                                 const GroupedOuts &o, hipStream_t s, int scorer = ICD_GROUP_SCORER_MAX) {
    for (int64_t q0 = 0; q0 < nq; q0 += g->qb) {
        const int nb = (int)std::min<int64_t>(g->qb, nq - q0);
        if (const int rc = grouped_scores_pass(idx, g, dq + (size_t)q0 * idx->dim, nb, s)) return rc;
        if (const int rc = grouped_reduce_pass(idx, g, nb, q0, k, group_size, reweighted, o, s, scorer)) return rc;
    }
    return ICD_OK;
}

// The one body of icd_index_search_grouped (scorer MAX, no group outputs) and icd_index_search_grouped_scored. Every check comes
// before the first device call.
static int grouped_search_entry(icd_index *idx, icd_grouping *grouping, const float *queries, int64_t nq, int32_t k, int32_t group_size,
                                int32_t queries_on_device, int32_t reweighted, int32_t scorer, double *out_adj, float *out_raw, int64_t *out_ids,
                                int32_t *out_levels, int32_t *out_groups, float *out_group_scores, int32_t *out_group_ids, int32_t out_on_device,
                                void *stream) {
    if (!valid(idx)) return fail(ICD_ERR_STATE, "invalid handle");
    if (!valid_handle(grouping)) return fail(ICD_ERR_STATE, "invalid grouping handle");
    icd_grouping *g = grouping;
    if (const int rc = check_owner(g->at, idx, "the grouping")) return rc;
    if (scorer != ICD_GROUP_SCORER_MAX && scorer != ICD_GROUP_SCORER_SUM && scorer != ICD_GROUP_SCORER_AVG)
        return fail(ICD_ERR_INVALID, "scorer=%d: ICD_GROUP_SCORER_MAX, _SUM or _AVG", scorer);
    if (k < 1 || group_size < 1 || (int64_t)k * group_size > ICD_MAX_K)
        return fail(ICD_ERR_INVALID, "k=%d group_size=%d: need k >= 1, group_size >= 1 and k * group_size <= %d", k, group_size, ICD_MAX_K);
    if (nq < 0 || nq > g->max_nq) return fail(ICD_ERR_INVALID, "nq=%lld exceeds the grouping's max_nq=%d", (long long)nq, g->max_nq);
    if (!out_ids || !out_raw || (reweighted && !out_adj)) return fail(ICD_ERR_INVALID, "output pointer is NULL");
    if (nq == 0) return ICD_OK;
    if (!queries) return fail(ICD_ERR_INVALID, "queries is NULL");
    std::lock_guard<std::mutex> guard(g->mu);
    const bool scored = scorer != ICD_GROUP_SCORER_MAX || out_group_scores || out_group_ids;
    if (scored && !g->scorers) return fail(ICD_ERR_STATE, "the grouping was never prepared for the group scorers (icd_grouping_prepare_scorers)");
    HIP_TRY(hipSetDevice(idx->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const HostCall hc{s, queries_on_device != 0, out_on_device != 0};
    int rc = check_capture(s, !queries_on_device || !out_on_device, false, false);
    if (rc) return rc;
    const float *dq;
    if ((rc = hc.upload(queries, g->qdev, (size_t)nq * idx->dim, &dq))) return rc;
    double *d_adj = hc.target(out_adj, g->o_adj); float *d_raw = hc.target(out_raw, g->o_raw);
    long long *d_ids = hc.target(reinterpret_cast<long long *>(out_ids), g->o_ids);
    int *d_lv = hc.target(out_levels, g->o_lv), *d_grp = hc.target(out_groups, g->o_grp);
    float *d_gs = hc.target(out_group_scores, g->o_gscore);
    int *d_gi = hc.target(out_group_ids, g->o_gid);
    const int ks = k * group_size;
    if ((rc = grouped_search_device(idx, g, dq, nq, k, group_size, reweighted != 0, GroupedOuts{d_adj, d_raw, d_ids, d_lv, d_grp, d_gs, d_gi}, s, scorer)))
        return rc;
    if ((rc = hc.copy_back({{out_adj, d_adj, 8}, {out_raw, d_raw, 4}, {out_ids, d_ids, 8}, {out_levels, d_lv, 4}, {out_groups, d_grp, 4}}, (size_t)nq * ks)))
        return rc;
    if ((rc = hc.copy_back({{out_group_scores, d_gs, 4}, {out_group_ids, d_gi, 4}}, (size_t)nq * k))) return rc;
    return hc.finish();
}

extern "C" {

int icd_grouping_create(icd_index *idx, const int32_t *group_of, int64_t n, int32_t on_device, int32_t max_nq, icd_grouping **out) {
    if (!out) return fail(ICD_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!valid(idx)) return fail(ICD_ERR_STATE, "invalid handle");
    if (!group_of) return fail(ICD_ERR_INVALID, "group_of is NULL");
    if (n != idx->n) return fail(ICD_ERR_INVALID, "group_of holds %lld ids, the index %lld rows", (long long)n, (long long)idx->n);
    if (n >= 0x7FFFFFFFll) return fail(ICD_ERR_UNSUPPORTED, "n=%lld: a grouping addresses rows with 31 bits", (long long)n);
    if (max_nq <= 0) return fail(ICD_ERR_INVALID, "max_nq=%d", max_nq);
    HIP_TRY(hipSetDevice(idx->device));
    std::vector<int> ids((size_t)n);
    if (on_device) HIP_TRY(hipMemcpy(ids.data(), group_of, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    else memcpy(ids.data(), group_of, (size_t)n * sizeof(int));
    for (int64_t i = 0; i < n; ++i)
        if (ids[i] < 0) return fail(ICD_ERR_INVALID, "group_of[%lld]=%d: group ids are non-negative (-1 marks padding in the outputs)", (long long)i, ids[i]);
    // rows in (group, row) order; dense group numbers in the order of the caller's ids
    std::vector<int> order((size_t)n), gpos((size_t)n), dense((size_t)n), seg;
    for (int64_t i = 0; i < n; ++i) order[i] = (int)i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return ids[a] < ids[b]; });
    int largest = 0;
    for (int64_t p = 0; p < n; ++p) {
        if (p == 0 || ids[order[p]] != ids[order[p - 1]]) {
            if (!seg.empty()) largest = std::max(largest, (int)p - seg.back());
            seg.push_back((int)p);
        }
        gpos[p] = (int)seg.size() - 1;
        dense[order[p]] = gpos[p];
    }
    largest = std::max(largest, (int)n - seg.back());
    const int G = (int)seg.size();
    seg.push_back((int)n);

    icd_grouping *g = new_handle<icd_grouping>(idx);
    if (!g) return fail(ICD_ERR_NOMEM, "host allocation failed");
    g->G = G; g->largest = largest; g->max_nq = max_nq; g->on_view = idx->row_map != nullptr;
    g->qb = std::min(GROUP_QUERY_BLOCK, (max_nq + GROUP_TILE - 1) / GROUP_TILE * GROUP_TILE);
    g->ldS = ((long long)n + GROUP_TILE - 1) / GROUP_TILE * GROUP_TILE;
    const size_t no = (size_t)max_nq * ICD_MAX_K;
#define GR_TRY(expr) HIP_TRY_OR(free_handle(g), expr)
    GR_TRY(g->alloc(&g->group_of, (size_t)n)); GR_TRY(g->alloc(&g->dense_of, (size_t)n)); GR_TRY(g->alloc(&g->order, (size_t)n));
    GR_TRY(g->alloc(&g->gpos, (size_t)n)); GR_TRY(g->alloc(&g->seg, (size_t)G + 1));
    GR_TRY(g->alloc(&g->S, (size_t)g->qb * g->ldS)); GR_TRY(g->alloc(&g->best, (size_t)g->qb * G));
    GR_TRY(g->alloc(&g->qdev, (size_t)max_nq * idx->dim));
    GR_TRY(g->alloc(&g->o_adj, no)); GR_TRY(g->alloc(&g->o_raw, no)); GR_TRY(g->alloc(&g->o_ids, no)); GR_TRY(g->alloc(&g->o_lv, no)); GR_TRY(g->alloc(&g->o_grp, no));
    GR_TRY(hipMemcpy(g->group_of, ids.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice));
    GR_TRY(hipMemcpy(g->dense_of, dense.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice));
    GR_TRY(hipMemcpy(g->order, order.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice));
    GR_TRY(hipMemcpy(g->gpos, gpos.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice));
    GR_TRY(hipMemcpy(g->seg, seg.data(), ((size_t)G + 1) * sizeof(int), hipMemcpyHostToDevice));
#undef GR_TRY
    g->bytes = (size_t)n * 20 + ((size_t)G + 1) * 4 + (size_t)g->qb * g->ldS * 4 + (size_t)g->qb * G * 8 + (size_t)max_nq * idx->dim * 4 + no * 28;
    *out = g;
    return ICD_OK;
}

int icd_grouping_destroy(icd_grouping *grouping) { return destroy_handle(grouping); }

int icd_grouping_stats(icd_grouping *grouping, int64_t *out_groups, int64_t *out_largest, int64_t *out_bytes) {
    if (!valid_handle(grouping)) return fail(ICD_ERR_STATE, "invalid grouping handle");
    if (out_groups) *out_groups = grouping->G;
    if (out_largest) *out_largest = grouping->largest;
    if (out_bytes) *out_bytes = (int64_t)grouping->bytes;
    return ICD_OK;
}

int icd_index_search_grouped(icd_index *idx, icd_grouping *grouping, const float *queries, int64_t nq, int32_t k, int32_t group_size,
                             int32_t queries_on_device, int32_t reweighted, double *out_adj, float *out_raw, int64_t *out_ids,
                             int32_t *out_levels, int32_t *out_groups, int32_t out_on_device, void *stream) {
    return grouped_search_entry(idx, grouping, queries, nq, k, group_size, queries_on_device, reweighted, ICD_GROUP_SCORER_MAX, out_adj, out_raw,
                                out_ids, out_levels, out_groups, nullptr, nullptr, out_on_device, stream);
}

int icd_index_search_grouped_scored(icd_index *idx, icd_grouping *grouping, const float *queries, int64_t nq, int32_t k, int32_t group_size,
                                    int32_t queries_on_device, int32_t reweighted, int32_t scorer, double *out_adj, float *out_raw,
                                    int64_t *out_ids, int32_t *out_levels, int32_t *out_groups, float *out_group_scores,
                                    int32_t *out_group_ids, int32_t out_on_device, void *stream) {
    return grouped_search_entry(idx, grouping, queries, nq, k, group_size, queries_on_device, reweighted, scorer, out_adj, out_raw, out_ids,
                                out_levels, out_groups, out_group_scores, out_group_ids, out_on_device, stream);
}

int icd_grouping_prepare_scorers(icd_index *idx, icd_grouping *grouping) {
    if (!valid(idx)) return fail(ICD_ERR_STATE, "invalid handle");
    if (!valid_handle(grouping)) return fail(ICD_ERR_STATE, "invalid grouping handle");
    if (const int rc = check_owner(grouping->at, idx, "the grouping")) return rc;
    std::lock_guard<std::mutex> guard(grouping->mu);
    icd_grouping *g = grouping;
    if (g->scorers) return ICD_OK;
    HIP_TRY(hipSetDevice(idx->device));
    // the plan is made from the grouping's own seg table (the host copy was not kept); synchronous copies on the NULL stream, as in
    // icd_grouping_create - so this call, like create, stays outside a capture
    std::vector<int> seg((size_t)g->G + 1);
    HIP_TRY(hipMemcpy(seg.data(), g->seg, seg.size() * sizeof(int), hipMemcpyDeviceToHost));
    const GaPlan plan = ga_plan(seg.data(), g->G);
    const size_t no = (size_t)g->max_nq * ICD_MAX_K;
    // the blocks join the handle's allocations only once all of them are there and filled: a failure leaves nothing behind
    GaPack *packs = nullptr; int *lg = nullptr; float *ogs = nullptr; int *ogi = nullptr;
    hipError_t e = dmalloc(&packs, std::max<size_t>(plan.packs.size(), 1));
    if (e == hipSuccess) e = dmalloc(&lg, std::max<size_t>(plan.long_groups.size(), 1));
    if (e == hipSuccess) e = dmalloc(&ogs, no);
    if (e == hipSuccess) e = dmalloc(&ogi, no);
    if (e == hipSuccess && !plan.packs.empty()) e = hipMemcpy(packs, plan.packs.data(), plan.packs.size() * sizeof(GaPack), hipMemcpyHostToDevice);
    if (e == hipSuccess && !plan.long_groups.empty())
        e = hipMemcpy(lg, plan.long_groups.data(), plan.long_groups.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        hipFree(packs); hipFree(lg); hipFree(ogs); hipFree(ogi);
        return fail(ICD_ERR_HIP, "preparing a grouping for the group scorers: %s", hipGetErrorString(e));
    }
    for (void *p : {(void *)packs, (void *)lg, (void *)ogs, (void *)ogi}) g->allocs.push_back(p);
    g->packs = packs; g->long_groups = lg; g->o_gscore = ogs; g->o_gid = ogi;
    g->npacks = (int)plan.packs.size(); g->nlong = (int)plan.long_groups.size();
    g->bytes += plan.bytes() + no * 8;
    g->scorers = true;
    return ICD_OK;
}

}  // extern "C"
