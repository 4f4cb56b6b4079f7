// icd_utility.hpp - the stateless utility entry points (no index, no handle): one launch each behind their argument checks. Part of
// icd_search.hip's translation unit (fail(), HIP_TRY, launch_lds); included there and nowhere else.
#pragma once

extern "C" {

int icd_merge_topk(int32_t device, const float *scores, const int64_t *ids, const int32_t *levels, int32_t G,
                   int64_t nq, int32_t k, double *out_adj, float *out_raw, int64_t *out_ids,
                   int32_t *out_levels, void *stream) {
    if (!scores || !ids || !levels) return fail(ICD_ERR_INVALID, "input pointer is NULL");
    if (G <= 0 || k <= 0 || k > ICD_MAX_K || (int64_t)G * k > 1024) return fail(ICD_ERR_INVALID, "G=%d k=%d: need G*k <= 1024", G, k);
    if (nq < 0 || nq > 0x7FFFFFFF) return fail(ICD_ERR_INVALID, "nq=%lld", (long long)nq);
    if (nq == 0) return ICD_OK;
    HIP_TRY(hipSetDevice(device));
    MergeArgs a{};
    a.scores = scores; a.ids = reinterpret_cast<const long long *>(ids); a.levels = levels;
    a.G = G; a.nq = (int)nq; a.k = k;
    a.out_adj = out_adj; a.out_raw = out_raw; a.out_ids = reinterpret_cast<long long *>(out_ids); a.out_levels = out_levels;
    const size_t lds = 4 * (1024 * 16 + 128 * 24);
    HIP_TRY(launch_lds<merge_topk_kernel>(device, lds, dim3(((int)nq + 3) / 4), dim3(256), lds, reinterpret_cast<hipStream_t>(stream), a));
    return ICD_OK;
}

// the two entry points share their checks and arguments; qp_width is the width of a query's row of q_params
static int hier_rescore_launch(int qp_width, int32_t device, const double *adj, const int64_t *ids, int64_t nq, int32_t k, int64_t id_base,
                               int64_t n_rows, const uint8_t *row_tags, const double *q_params, const double *weights,
                               int32_t *out_order, double *out_enhanced, double *out_score, double *out_vs, double *out_hb,
                               double *out_boost, void *stream) {
    if (!adj || !ids || !row_tags || !q_params || !weights) return fail(ICD_ERR_INVALID, "input pointer is NULL");
    if (!out_order || !out_enhanced || !out_score || !out_vs || !out_hb || !out_boost) return fail(ICD_ERR_INVALID, "output pointer is NULL");
    if (k <= 0 || k > HIER_MAX_K) return fail(ICD_ERR_INVALID, "k=%d (1..%d)", k, HIER_MAX_K);
    if (nq < 0 || nq > 0x7FFFFFFF || n_rows < 0) return fail(ICD_ERR_INVALID, "nq=%lld n_rows=%lld", (long long)nq, (long long)n_rows);
    if (nq == 0) return ICD_OK;
    HIP_TRY(hipSetDevice(device));
    HierArgs a{};
    a.adj = adj; a.ids = reinterpret_cast<const long long *>(ids); a.nq = (int)nq; a.k = k; a.id_base = id_base; a.n_rows = n_rows;
    a.row_tags = row_tags; a.q_params = q_params;
    a.w_hb = weights[0]; a.w_em = weights[1]; a.w_sc = weights[2]; a.w_ca = weights[3]; a.w_cr = weights[4];
    a.sc_value = weights[5]; a.level_term = weights[6];
    a.out_order = out_order; a.out_enhanced = out_enhanced; a.out_score = out_score; a.out_vs = out_vs; a.out_hb = out_hb;
    a.out_boost = out_boost;
    if (qp_width == HIER_QP_ENT)
        hipLaunchKernelGGL(hier_rescore_kernel<HIER_QP_ENT>, dim3(((int)nq + 3) / 4), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
    else
        hipLaunchKernelGGL(hier_rescore_kernel<HIER_QP>, dim3(((int)nq + 3) / 4), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
    HIP_TRY(hipGetLastError());
    return ICD_OK;
}

int icd_hier_rescore(int32_t device, const double *adj, const int64_t *ids, int64_t nq, int32_t k, int64_t id_base,
                     int64_t n_rows, const uint8_t *row_tags, const double *q_params, const double *weights,
                     int32_t *out_order, double *out_enhanced, double *out_score, double *out_vs, double *out_hb,
                     double *out_boost, void *stream) {
    return hier_rescore_launch(HIER_QP, device, adj, ids, nq, k, id_base, n_rows, row_tags, q_params, weights, out_order,
                               out_enhanced, out_score, out_vs, out_hb, out_boost, stream);
}

int icd_hier_rescore_entities(int32_t device, const double *adj, const int64_t *ids, int64_t nq, int32_t k, int64_t id_base,
                              int64_t n_rows, const uint8_t *row_tags, const double *q_params, const double *weights,
                              int32_t *out_order, double *out_enhanced, double *out_score, double *out_vs, double *out_hb,
                              double *out_boost, void *stream) {
    return hier_rescore_launch(HIER_QP_ENT, device, adj, ids, nq, k, id_base, n_rows, row_tags, q_params, weights, out_order,
                               out_enhanced, out_score, out_vs, out_hb, out_boost, stream);
}

int icd_pack_winners(int32_t device, const int32_t *order, const int64_t *ids, const float *raw, const double *adj, const double *enhanced,
                     const double *vs, const double *hb, const double *boost, int64_t nq, int32_t k, int32_t kk, double *out, void *stream) {
    if (!order || !ids || !raw || !adj || !enhanced || !vs || !hb || !boost || !out) return fail(ICD_ERR_INVALID, "pointer is NULL");
    if (k <= 0 || kk <= 0 || kk > k || nq < 0 || nq > 0x7FFFFFFF) return fail(ICD_ERR_INVALID, "nq=%lld k=%d kk=%d", (long long)nq, k, kk);
    if (nq == 0) return ICD_OK;
    HIP_TRY(hipSetDevice(device));
    PackWinnersArgs a{};
    a.order = order; a.ids = reinterpret_cast<const long long *>(ids); a.raw = raw; a.adj = adj; a.enh = enhanced; a.vs = vs; a.hb = hb; a.boost = boost;
    a.nq = (int)nq; a.k = k; a.kk = kk; a.out = out;
    const long long per = (long long)nq * kk;
    hipLaunchKernelGGL(pack_winners_kernel, dim3((unsigned)((per + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
    HIP_TRY(hipGetLastError());
    return ICD_OK;
}

int icd_score_stats(int32_t device, const double *scores, const int32_t *order, int64_t nq, int32_t k, int32_t use,
                    double *out, void *stream) {
    if (!scores || !out) return fail(ICD_ERR_INVALID, "pointer is NULL");
    if (k <= 0 || k > STATS_MAX_K || use <= 0) return fail(ICD_ERR_INVALID, "k=%d (1..%d) use=%d", k, STATS_MAX_K, use);
    if (nq < 0 || nq > 0x7FFFFFFF) return fail(ICD_ERR_INVALID, "nq=%lld", (long long)nq);
    if (nq == 0) return ICD_OK;
    HIP_TRY(hipSetDevice(device));
    StatsArgs a{};
    a.scores = scores; a.order = order; a.nq = (int)nq; a.k = k; a.use = use; a.out = out;
    hipLaunchKernelGGL(score_stats_kernel, dim3(((int)nq + 63) / 64), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), a);
    HIP_TRY(hipGetLastError());
    return ICD_OK;
}

int icd_cosine_rows(int32_t device, const float *x, const float *y, int64_t y_stride, int64_t nq, int32_t dim,
                    double *out, void *stream) {
    if (!x || !y || !out) return fail(ICD_ERR_INVALID, "pointer is NULL");
    if (dim <= 0 || (y_stride != 0 && y_stride != dim)) return fail(ICD_ERR_INVALID, "dim=%d y_stride=%lld (0 or dim)", dim, (long long)y_stride);
    if (nq < 0 || nq > 0x7FFFFFFF) return fail(ICD_ERR_INVALID, "nq=%lld", (long long)nq);
    if (nq == 0) return ICD_OK;
    HIP_TRY(hipSetDevice(device));
    CosArgs a{};
    a.x = x; a.y = y; a.y_stride = y_stride; a.nq = (int)nq; a.dim = dim; a.out = out;
    hipLaunchKernelGGL(cosine_rows_kernel, dim3(((int)nq + 3) / 4), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
    HIP_TRY(hipGetLastError());
    return ICD_OK;
}

int icd_term_first_match(int32_t device, const int32_t *key_cp, const int32_t *key_off, int32_t n_keys, const int32_t *term_cp,
                         const int32_t *term_off, int32_t n_terms, int32_t *out_first, void *stream_) {
    if (!key_cp || !key_off || !term_cp || !term_off || !out_first) return fail(ICD_ERR_INVALID, "pointer is NULL");
    if (n_keys < 0 || n_terms < 0) return fail(ICD_ERR_INVALID, "n_keys=%d n_terms=%d", n_keys, n_terms);
    if (n_terms == 0) return ICD_OK;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    HIP_TRY(hipSetDevice(device));
    // the terms' lengths decide whether the kernel can take them: read the offsets (n_terms + 1 ints) on the stream
    std::vector<int32_t> off((size_t)n_terms + 1);
    HIP_TRY(hipMemcpyAsync(off.data(), term_off, off.size() * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (off[0] < 0) return fail(ICD_ERR_INVALID, "term_off[0]=%d", off[0]);
    for (int32_t t = 0; t < n_terms; ++t) {
        const int32_t len = off[t + 1] - off[t];
        if (len < 0) return fail(ICD_ERR_INVALID, "term %d: term_off decreases", t);
        if (len > ICD_TERM_MAX_LEN) return fail(ICD_ERR_UNSUPPORTED, "term %d has %d code points (at most %d)", t, len, ICD_TERM_MAX_LEN);
    }
    static_assert(ICD_TERM_MAX_LEN == TERM_MAX_LEN, "ICD_TERM_MAX_LEN and term_lookup.hpp disagree");
    TermArgs a{};
    a.key_cp = key_cp; a.key_off = key_off; a.n_keys = n_keys; a.term_cp = term_cp; a.term_off = term_off; a.n_terms = n_terms;
    a.out_first = out_first;
    hipLaunchKernelGGL(term_first_match_kernel, dim3((unsigned)n_terms), dim3(TERM_BLOCK), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return ICD_OK;
}

int icd_packed_attention(int32_t device, const float *qkv, int64_t ld, const int32_t *starts, int32_t nseq, int32_t heads,
                         int32_t head_dim, int32_t max_len, float *out, int64_t out_ld, void *stream) {
    if (!qkv || !starts || !out) return fail(ICD_ERR_INVALID, "pointer is NULL");
    if (head_dim != ATT_HEAD_DIM) return fail(ICD_ERR_UNSUPPORTED, "head_dim=%d (this kernel is written for %d)", head_dim, ATT_HEAD_DIM);
    if (max_len < 1 || max_len > ATT_MAX_SEQ) return fail(ICD_ERR_UNSUPPORTED, "max_len=%d (1..%d tokens per sequence)", max_len, ATT_MAX_SEQ);
    if (nseq < 0 || heads <= 0 || (int64_t)nseq * heads > 0x7FFFFFF0LL) return fail(ICD_ERR_INVALID, "nseq=%d heads=%d", nseq, heads);
    const int64_t hidden = (int64_t)heads * head_dim;
    if (ld < 3 * hidden || out_ld < hidden || ld % 4 != 0) return fail(ICD_ERR_INVALID, "ld=%lld out_ld=%lld for hidden=%lld", (long long)ld, (long long)out_ld, (long long)hidden);
    if (nseq == 0) return ICD_OK;
    HIP_TRY(hipSetDevice(device));
    PackedAttnArgs a{};
    a.qkv = qkv; a.out = out; a.starts = starts; a.nseq = nseq; a.heads = heads; a.ld = ld; a.out_ld = out_ld; a.hidden = (int)hidden;
    a.scale = 0.125f;   // 1 / sqrt(64), exact
    const int tasks = nseq * heads;
    hipLaunchKernelGGL(packed_attention_kernel, dim3((tasks + 3) / 4), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
    HIP_TRY(hipGetLastError());
    return ICD_OK;
}

int icd_split_bf16x3(int32_t device, const float *x, int64_t rows, int32_t cols, int64_t ld, int32_t act, void *out, void *stream) {
    if (!x || !out) return fail(ICD_ERR_INVALID, "pointer is NULL");
    if (rows < 0 || cols < SPLIT_TAIL || cols % 8 != 0 || ld < cols || ld % 4 != 0) return fail(ICD_ERR_INVALID, "rows=%lld cols=%d ld=%lld (cols a multiple of 8, ld >= cols and a multiple of 4)", (long long)rows, cols, (long long)ld);
    if (act != 0 && act != 1) return fail(ICD_ERR_INVALID, "act=%d (0 none, 1 erf-GELU)", act);
    if ((reinterpret_cast<uintptr_t>(x) & 15) != 0 || (reinterpret_cast<uintptr_t>(out) & 15) != 0) return fail(ICD_ERR_INVALID, "x and out must be 16-byte aligned");
    if (rows == 0) return ICD_OK;
    HIP_TRY(hipSetDevice(device));
    SplitArgs a{};
    a.x = x; a.out = static_cast<unsigned short *>(out); a.rows = rows; a.cols = cols; a.act = act; a.ld = ld;
    const long long total = rows * (long long)(cols / 8);
    const int blocks = (int)std::min<long long>((total + 255) / 256, 8192);
    hipLaunchKernelGGL(split_bf16x3_kernel, dim3(blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
    HIP_TRY(hipGetLastError());
    return ICD_OK;
}

int icd_unpack_query_slices(int32_t device, const void *gathered, int32_t world, int64_t nq, int32_t k, double *out_adj,
                                  float *out_raw, int64_t *out_ids, int32_t *out_levels, void *stream) {
    if (!gathered || !out_adj || !out_raw || !out_ids || !out_levels) return fail(ICD_ERR_INVALID, "pointer is NULL");
    if (world < 1 || nq < 0 || k <= 0) return fail(ICD_ERR_INVALID, "world=%d nq=%lld k=%d", world, (long long)nq, k);
    HIP_TRY(hipSetDevice(device));
    const size_t width = ((size_t)nq + world - 1) / world, per = width * k;
    const char *rb = static_cast<const char *>(gathered);
    if (icd_internal_unpack_query_slices(rb, rb + per * world * 8, rb + per * world * 16, rb + per * world * 20, world, nq, k,
                                         (long long)width, out_adj, out_raw, out_ids, out_levels, stream))
        return fail(ICD_ERR_HIP, "the unpack launch failed");
    return ICD_OK;
}

}  // extern "C"
