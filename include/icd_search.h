/*
 * icd_search.h — C ABI of libicdsearch.so: exact inner-product (FLAT / IP) top-k search over a dense
 * fp32 corpus on one MI355X (gfx950), with the ICD level reweight of the reference fused in.
 *
 * This is the drop-in boundary for the reference's vector-engine calls. The reference has no FFI of
 * its own (pure Python); each entry point below names the reference call it
 * replaces (paths relative to the reference repository root):
 *
 *   icd_index_create            <- MilvusClient.create_collection + insert + load_collection
 *                                  services/milvus_service.py:163-206 (schema, FLAT/IP index),
 *                                  :208-269 (insert_records), :137-161 (load to memory)
 *   icd_index_search            <- MilvusClient.search(data=[q], limit=top_k)
 *                                  services/milvus_service.py:280-285
 *   icd_index_search_reweighted <- the same call plus the per-hit level weight and stable re-sort
 *                                  services/milvus_service.py:290-295,314,550-558
 *   icd_index_stats             <- get_collection_stats / get_memory_usage
 *                                  services/milvus_service.py:322-341,498-522
 *   icd_index_destroy           <- release_collection / disconnect
 *                                  services/milvus_service.py:400-424,452-496
 *   icd_merge_topk              <- no counterpart (the reference is single-process); merges the
 *                                  per-shard partial top-k lists of a row-sharded corpus after the
 *                                  RCCL all-gather.
 *   icd_group_*                 <- no counterpart: one process per GPU, an RCCL communicator owned by the group; the
 *                                  row-sharded search (local top-k -> ncclAllGather -> merge + reweight) and the
 *                                  query-sharded one (SURVEY.md section 8b "suggested C ABI", 8e) in one call, on one stream.
 *
 * Conventions
 *   - All matrices are dense row-major (exactly numpy's C order): corpus [n][dim], queries [nq][dim],
 *     outputs [nq][k].
 *   - Pointers are borrowed for the duration of the call. `*_on_device` says whether a pointer is a
 *     HIP device pointer (1) or host memory (0). Outputs are caller-allocated.
 *   - `stream` is a hipStream_t (NULL = the default stream). Calls with device inputs AND device
 *     outputs only enqueue work (no allocation, no synchronisation: graph-capturable); calls that
 *     touch host buffers synchronise the stream before returning.
 *   - Result order: best first by (score descending, row id ascending). Scores are the canonical
 *     fp32 fmaf chain over d = 0..dim-1, bit-identical to oracle/icd_oracle.c.
 *     Slots beyond the number of valid hits (n < k, NaN scores) hold id = -1, score = -inf.
 *   - Row ids are `id_base + row index` (id_base != 0 for a shard of a larger corpus).
 *   - Every function returns ICD_OK (0) or a negative icd_status; icd_last_error() gives the text.
 *   - Threads: calls on one handle are serialised by the library (a mutex guards the handle's host-side state: plans,
 *     adaptive counters, profiling ring), so concurrent callers cannot corrupt it. The handle's DEVICE workspace is
 *     reused by every search: enqueue the searches of one handle on ONE stream (or order the streams yourself); two
 *     searches of one handle executing concurrently on different streams is a data race on the device. Different
 *     handles are independent.
 */
#ifndef ICD_SEARCH_H
#define ICD_SEARCH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ICD_ABI_VERSION 6   /* 6: icd_encoder_encode_many; icd_index_create_view (an addition); the process-wide icd_debug_set_* switches became per-index options (icd_index_create flags, icd_index_set_option); ICD_ENCODER_MAX_TOKENS 512, ICD_ENCODER_MAX_SEQS 64 (round 6). 5: icd_unpack_query_slices, icd_debug_set_stream_one, icd_debug_set_pacing, icd_debug_set_exact_narrow, icd_debug_set_host_one, icd_split_bf16x3, icd_encoder_create / _encode / _destroy, icd_pack_winners (round 5). 4: icd_debug_set_family_order, icd_debug_set_center, icd_stats.centered / mean_share appended, icd_group_prepare / icd_group_connect (round 4). 3: icd_stats.sparse_fallback_armed appended, icd_debug_set_create_probe, icd_packed_attention (round 3). 2: + icd_hier_rescore, icd_score_stats, icd_cosine_rows, icd_debug_set_permute (round 2), the group entry points (round 3) */
#define ICD_MAX_K 128

typedef struct icd_index icd_index;

typedef enum icd_status {
    ICD_OK = 0,
    ICD_ERR_INVALID = -1,     /* bad argument */
    ICD_ERR_HIP = -2,         /* a HIP runtime call failed */
    ICD_ERR_NOMEM = -3,       /* device or host allocation failed */
    ICD_ERR_UNSUPPORTED = -4, /* shape / device not supported (not gfx950, dim, k) */
    ICD_ERR_STATE = -5        /* handle destroyed or not initialised */
} icd_status;

typedef enum icd_mode {
    ICD_MODE_AUTO = 0,  /* fp16-MFMA coarse pass + exact fp32 rescoring, certified per query;
                           uncertified queries re-run on the exact kernel. Results identical to EXACT. */
    ICD_MODE_EXACT = 1  /* fp32-MFMA kernel only */
} icd_mode;

typedef struct icd_stats {
    int64_t n;                  /* rows in this index / shard */
    int32_t dim;
    int32_t device;
    int64_t id_base;
    int64_t bytes_corpus_f32;   /* HBM bytes held */
    int64_t bytes_corpus_f16;
    int64_t bytes_workspace;
    int32_t max_nq;
    int32_t max_k;
    int32_t fast_path;          /* 1 if the fp16 coarse path is usable for this index */
    float   rmax;               /* max row L2 norm */
    /* counters of the most recent search (valid after the stream is synchronised) */
    int64_t last_nq;
    int64_t last_fallback;      /* queries that took the exact fallback in AUTO mode */
    int32_t last_chunks;        /* candidate lists per query (P) of the last call's scoring pass */
    int32_t last_mode;
    int64_t last_second_pass;   /* queries the first coarse pass could not certify and the second one took (AUTO mode) */
    int32_t last_second_pass_lists; /* candidate lists per query of that second pass (0: it was not part of the call) */
    int32_t second_pass_armed;  /* 1: the next large search carries the second pass's launches (armed for the first searches of
                                   an index and after any search that flagged more than the streaming kernel takes cheaply;
                                   dropped after a few consecutive searches that flagged fewer) */
    int32_t wide_mode;          /* 1: large batches are planned with the second pass's list count from the start (the
                                   previous large batch needed the second pass for most of its queries) */
    int32_t sparse_fallback_armed; /* 1: the exact re-search behind the last AUTO search carried the streaming kernel's two
                                   launches (few flagged queries: ~0.05 ms); 0: they were left out after a long run of
                                   searches with nothing flagged, and the fp32-MFMA kernel takes any count (~0.4 ms, once:
                                   the run restarts and the required length doubles). Results are exact either way. */
    int32_t centered;           /* 1: the fp16 image of the corpus holds the rows minus their column mean (the rows share a large
                                   common component, as sentence embeddings do: the coarse pass ranks by q.(c - mu), the same
                                   order as q.c, with an fp16 error relative to the centred rows). Results are exact either way. */
    float   mean_share;         /* |mu|^2 / mean |row|^2: the mean pairwise cosine of unit rows (centred when >= 0.25) */
} icd_stats;

/* per-kernel device time of the most recent search, measured with hipEvents on the search stream.
 * Only recorded while profiling is enabled (icd_index_set_profiling). */
typedef struct icd_profile {
    float ms_prep;      /* query fp32->fp16 + norms */
    float ms_coarse;    /* fp16 MFMA + fused top-k' (dominant kernel) */
    float ms_finalize;  /* merge + certify + exact rescoring + reweight */
    float ms_exact;     /* fp32 MFMA kernel (EXACT mode, or the AUTO fallback) */
    float ms_exact_finalize;
    float ms_total;     /* first event to last event */
} icd_profile;

int icd_abi_version(void);

/* Text of the most recent error on this thread (never NULL). */
const char *icd_last_error(void);

/* Number of HIP devices visible, or a negative icd_status. */
int icd_device_count(void);

/*
 * Build an index over `n` rows of `dim` floats. `levels` (int32[n], ICD hierarchy level of each row:
 * 1, 2 or 3) may be NULL (all rows level 1 -> weight 1.2, the reference default level,
 * services/milvus_service.py:247). The corpus is copied to HBM; the caller's buffer is not retained.
 * max_nq: largest query batch a single search call will receive (workspace is sized for it).
 * max_k:  largest k (<= ICD_MAX_K).
 * flags:  ICD_CREATE_CORPUS_ON_DEVICE - `corpus` (and `levels`) are device pointers; the rest are A/B and test options of
 *         THIS index (results are identical with or without them): ICD_CREATE_ROW_ORDER keeps the fp16 corpus copy in row
 *         order instead of the golden-ratio permutation (only the share of certified queries changes); ICD_CREATE_NO_PROBE
 *         skips the corpus-shape probe (with it, an index whose max_nq allows batches of >= 2 048 queries searches 2 048
 *         evenly spaced rows of its own corpus once and starts large batches on the wide partition, icd_stats.wide_mode, when
 *         most of them could not be certified from the narrow plan's lists - a corpus of tight families of near-identical
 *         rows; later searches keep deciding from their own counters); ICD_CREATE_NO_CENTER keeps the fp16 image uncentred
 *         whatever the rows look like (icd_stats.centered).
 */
enum { ICD_CREATE_CORPUS_ON_DEVICE = 1, ICD_CREATE_ROW_ORDER = 2, ICD_CREATE_NO_PROBE = 4, ICD_CREATE_NO_CENTER = 8 };
int icd_index_create(const float *corpus, int64_t n, int32_t dim, const int32_t *levels,
                     int64_t id_base, int32_t device, int32_t max_nq, int32_t max_k,
                     int32_t flags, icd_index **out);

int icd_index_destroy(icd_index *idx);

/*
 * A view: an ordinary index over rows rows[0 .. n_rows) of `parent` (a Milvus `filter` expression's selection). The row ids are
 * the parent's row indices, strictly increasing, inside [0, parent n); anything else is ICD_ERR_INVALID, and so is n_rows = 0.
 * `rows` is a device pointer when rows_on_device is set. The view is built on the parent's device from the parent's fp32 rows
 * and levels (a gather kernel: nothing is uploaded), then exactly like icd_index_create with ICD_CREATE_CORPUS_ON_DEVICE: its
 * own fp16 image, centring decision and probe, sized by max_nq / max_k; `flags` takes the same A/B bits. Every search entry
 * point, icd_index_stats and icd_index_set_option work on it unchanged; its hits carry the PARENT's global ids (id_base + row),
 * mapped where the outputs are written, so the (score desc, id asc) order and the stable re-sort are those of the parent's
 * ranking restricted to the rows. With fewer than k rows the lists are padded (score -inf, id -1, level 0). The view keeps no
 * pointer into the parent: either may be destroyed first. icd_index_lookup_levels and icd_group_create / _prepare on a view
 * return ICD_ERR_UNSUPPORTED.
 */
int icd_index_create_view(icd_index *parent, const int64_t *rows, int64_t n_rows, int32_t rows_on_device,
                          int32_t max_nq, int32_t max_k, int32_t flags, icd_index **out);

/*
 * Grouping search: Milvus's `group_by_field` / `group_size` (MilvusClient.search(..., group_by_field=, group_size=,
 * strict_group_size=False); the reference passes neither, services/milvus_service.py:280-285). For every query the k best GROUPS -
 * a group ranks by its best row - and of each its min(group_size, members) best rows, EXACT: every row is scored with the
 * canonical chain and reduced per group, so a group is never short because a candidate list was.
 *
 * icd_grouping_create: group_of int32[n] (n = the index's rows; host, or device with on_device = 1), any non-negative ids. The
 * rows are ordered by (group, row) on the host and uploaded with the workspace of the searches (sized for batches of up to
 * max_nq queries; nothing is allocated later). One grouping per field; any number of them per index, each with its own
 * workspace. On a view (icd_index_create_view) group_of has one id per row OF THE VIEW. A grouping keeps no pointer into its
 * index: either may be destroyed first; a search checks that the two belong together. n >= 2^31 rows: ICD_ERR_UNSUPPORTED.
 * The row-sharded path (icd_group_*) has no grouping search.
 *
 * icd_index_search_grouped: outputs [nq][k * group_size], k >= 1, group_size >= 1, k * group_size <= ICD_MAX_K (else
 * ICD_ERR_INVALID, before any device call).
 *   reweighted = 0  group-rank-major: the best group's rows best first, then the second group's, ... back to back (a group
 *                   with fewer than group_size rows takes fewer slots); out_raw the canonical scores, out_ids, out_levels,
 *                   out_groups (the caller's id of the hit's group). out_adj is not written.
 *   reweighted = 1  that list through icd_index_search_reweighted's step: out_adj = (double)raw * w[level] and ONE stable
 *                   descending re-sort of the query's hits; raw, ids, levels and groups travel with the hit.
 * Unused slots at the end of a query's list: score -inf, id -1, level 0, group -1. out_levels / out_groups may be NULL.
 * Queries and outputs are host or device pointers as in icd_index_search; device-in / device-out calls only enqueue on
 * `stream` (graph-capturable). Searches of one grouping share its workspace: one stream at a time, as for an index.
 */
typedef struct icd_grouping icd_grouping;
int icd_grouping_create(icd_index *idx, const int32_t *group_of, int64_t n, int32_t on_device, int32_t max_nq, icd_grouping **out);
int icd_grouping_destroy(icd_grouping *grouping);
/* distinct groups, rows of the largest one, device bytes held (any pointer may be NULL) */
int icd_grouping_stats(icd_grouping *grouping, int64_t *out_groups, int64_t *out_largest, int64_t *out_bytes);
int icd_index_search_grouped(icd_index *idx, icd_grouping *grouping, const float *queries, int64_t nq, int32_t k, int32_t group_size,
                             int32_t queries_on_device, int32_t reweighted, double *out_adj, float *out_raw, int64_t *out_ids,
                             int32_t *out_levels, int32_t *out_groups, int32_t out_on_device, void *stream);

/*
 * Group scorers: Milvus's group scorer max / sum / avg of its grouping search. A group ranks by the sum, or
 * the mean, of its group_size best rows instead of by its single best row - nearest-neighbour voting per group, exact over every
 * row. The sum-ranked best groups are not among the max-ranked ones in general, so no step behind icd_index_search_grouped can
 * answer this: every group of every query is reduced by its own top-group_size selection.
 *
 * For a query, a grouping, k, s = group_size and a scorer:
 *   1. Scores, keys and "a NaN score is no hit" are icd_index_search_grouped's. A group's members rank by (score desc, row asc);
 *      x_1 ... x_m are the scores of its m = min(s, hits in the group) best members, best first.
 *   2. ICD_GROUP_SCORER_MAX: a = x_1. ICD_GROUP_SCORER_SUM: a = x_1, then a = a + x_i for i = 2 ... m IN THAT ORDER, each ONE IEEE
 *      fp32 add (nothing contracted, nothing reassociated: the order is part of the contract, the worst-first sum differs in the
 *      last bit for a third of all triples). ICD_GROUP_SCORER_AVG: the SUM value, then ONE IEEE fp32 divide by (float)m.
 *   3. A group with no hit, or whose aggregate is NaN (+inf + -inf), is no hit. Every other aggregate ranks the way a row's score
 *      does, +inf and -inf included: -inf is an ordinary lowest score, as a best row at -inf is in icd_index_search_grouped.
 *   4. Groups rank by (aggregate desc, row of the group's best member asc). The answer is the min(k, groups that are hits) best
 *      groups, of each its m best rows; layout, padding and the reweighted = 1 step are icd_index_search_grouped's. out_raw holds
 *      the hit's own canonical score: the aggregate never replaces it and never enters the level reweight.
 *   5. out_group_scores f32 [nq][k] (the aggregate; padding -inf) and out_group_ids i32 [nq][k] (the caller's group id; padding -1)
 *      are in group-rank order in BOTH output modes (behind the reweight's re-sort the hits no longer say which group was first).
 *      Either may be NULL.
 *   6. MAX through this entry point is icd_index_search_grouped byte for byte (the same launches); SUM and AVG at s = 1 are MAX; one
 *      group of all rows at s = m returns icd_index_search's rows at k = m; views and id_base as in icd_index_search_grouped.
 *
 * icd_grouping_prepare_scorers: once per grouping, outside any search and outside any stream capture (it allocates and copies
 * synchronously, as icd_grouping_create does): builds the plan that cuts the grouping's positions into per-wave work along group
 * boundaries, and a host caller's staging of the two group outputs. Idempotent. Its bytes are counted in icd_grouping_stats from
 * then on. A search with scorer SUM or AVG, or with either group output, on a grouping that was never prepared is ICD_ERR_STATE;
 * nothing is allocated in a search, so device-in / device-out scored searches stay graph-capturable.
 *
 * icd_index_search_grouped_scored: icd_index_search_grouped's arguments, checks and limits (k * group_size <= ICD_MAX_K), plus the
 * scorer and the two group outputs. ICD_ERR_INVALID before any device call, with no output byte written: an unknown scorer, and
 * whatever icd_index_search_grouped refuses (a grouping of another index among it). One scorer per call.
 * Not offered: sparse grouped and hybrid grouped search with a scorer, the row-sharded path (icd_group_*), per-query scorers in
 * one batch, k * group_size > 128, a sum weighted by rank.
 */
#define ICD_GROUP_SCORER_MAX 0
#define ICD_GROUP_SCORER_SUM 1
#define ICD_GROUP_SCORER_AVG 2
int icd_grouping_prepare_scorers(icd_index *idx, icd_grouping *grouping);
int icd_index_search_grouped_scored(icd_index *idx, icd_grouping *grouping, const float *queries, int64_t nq, int32_t k, int32_t group_size,
                                    int32_t queries_on_device, int32_t reweighted, int32_t scorer, double *out_adj, float *out_raw,
                                    int64_t *out_ids, int32_t *out_levels, int32_t *out_groups, float *out_group_scores,
                                    int32_t *out_group_ids, int32_t out_on_device, void *stream);

/*
 * Embedding-list search: Milvus's embedding lists under the MAX_SIM metric. A query is a LIST of vectors -
 * the segments of one clinical text - and a group of rows scores the sum, over the list's vectors, of its best row's inner
 * product: which category, parent code or code covers all segments best, and which row answers which segment. The group that is
 * best in sum is in general not among any single vector's best groups, so no finished hit list can answer this: every row is
 * scored for every vector and reduced per group (the two kernels of icd_index_search_grouped), then per list.
 *
 * A batch of nl lists: list_off is a HOST int64 array of nl + 1 entries, non-decreasing from 0; list L owns the vectors
 * list_off[L] .. list_off[L + 1] (T_L of them) of queries[list_off[nl]][dim] (host, or device with queries_on_device = 1).
 *   1. Scores, keys and "a NaN score is no hit" are icd_index_search_grouped's. For a vector t and a group g, b(t, g) is the key of
 *      g's best row under t by (score desc, row asc), or none.
 *   2. ICD_MAXSIM_SUM: over the vectors of L that have a hit in g, IN LIST ORDER, a = x_first, then a = a + x_t, each ONE IEEE fp32
 *      add (nothing contracted, nothing reassociated: the order is part of the contract). ICD_MAXSIM_MEAN: that sum, then ONE IEEE
 *      fp32 divide by (float)hits, the number of vectors that have a hit in g.
 *   3. A group is no hit when no vector of L hits it or when its aggregate is NaN (+inf + -inf); +inf and -inf aggregates rank as
 *      ordinary scores.
 *   4. Groups rank by (aggregate desc, row of b(t1, g) asc), t1 the first vector of L that hits g. The answer is the
 *      min(k, groups that are hits) best groups.
 *   5. Outputs, host or (out_on_device = 1) device; any may be NULL except the first two:
 *        out_group_scores f32 [nl][k]   the aggregate; padding -inf
 *        out_group_ids    i32 [nl][k]   the caller's group id; padding -1
 *        out_match_scores f32, out_match_ids i64, out_match_levels i32, each [list_off[nl]][k]: for vector t of list L, slot j
 *        holds b(t, j-th group of L) - the canonical raw score, the id through row_map / id_base as everywhere, the level.
 *        Padding -inf / -1 / 0, also where t has no hit in that group. No level reweight touches the aggregate.
 *   6. Lists of one vector each give icd_index_search_grouped_scored(scorer MAX, group_size 1)'s group scores, group ids and hits
 *      byte for byte; the list [v, v] gives the groups of [v] with aggregates x + x; MEAN at T = 1 is SUM; views and id_base as
 *      in icd_index_search_grouped.
 *   7. 1 <= T_L <= ICD_MAXSIM_MAX_T, 1 <= k <= ICD_MAX_K, nl <= max_lists and list_off[nl] <= max_vectors of the preparation.
 *      A violation, an unknown scorer or a grouping of another index is ICD_ERR_INVALID before any device call, with no output
 *      byte written; a grouping that was never prepared is ICD_ERR_STATE. nl = 0 does nothing.
 *
 * icd_grouping_prepare_maxsim: once per grouping, outside any search and outside any stream capture (it allocates): the block of
 * the lists' aggregates and the staging of host callers for up to max_lists lists of max_vectors vectors in all. Idempotent: a
 * repeated call within those sizes returns at once, a larger one is ICD_ERR_INVALID. Its bytes are counted in icd_grouping_stats.
 * Nothing is allocated in a search (the list offsets travel in the launch arguments), so device-in / device-out calls are
 * graph-capturable; with host buffers a capturing stream is ICD_ERR_INVALID.
 * Not offered: per-list row masks (filter through a view, as for the grouping search), bands, per-vector weights, group_size > 1,
 * sparse lists, the row-sharded path (icd_group_*).
 */
#define ICD_MAXSIM_SUM 1
#define ICD_MAXSIM_MEAN 2
#define ICD_MAXSIM_MAX_T 64
int icd_grouping_prepare_maxsim(icd_index *idx, icd_grouping *grouping, int64_t max_lists, int64_t max_vectors);
int icd_index_search_maxsim(icd_index *idx, icd_grouping *grouping, const float *queries, const int64_t *list_off, int64_t nl, int32_t k,
                            int32_t scorer, int32_t queries_on_device, float *out_group_scores, int32_t *out_group_ids,
                            float *out_match_scores, int64_t *out_match_ids, int32_t *out_match_levels, int32_t out_on_device,
                            void *stream);

/* Raw top-k by inner product. out_scores float[nq][k], out_ids int64[nq][k]. */
int icd_index_search(icd_index *idx, const float *queries, int64_t nq, int32_t k,
                     int32_t queries_on_device, int32_t mode,
                     float *out_scores, int64_t *out_ids, int32_t out_on_device, void *stream);

/*
 * Raw top-k, then adj = (double)score * w[level] and a stable descending re-sort of the k hits
 * (the order MilvusService.search returns). All four outputs are [nq][k] in the re-sorted order:
 * out_adj (double), out_raw (float, the inner product), out_ids, out_levels. Any of out_raw /
 * out_levels may be NULL.
 */
int icd_index_search_reweighted(icd_index *idx, const float *queries, int64_t nq, int32_t k,
                                int32_t queries_on_device, int32_t mode,
                                double *out_adj, float *out_raw, int64_t *out_ids, int32_t *out_levels,
                                int32_t out_on_device, void *stream);

/*
 * Range search, offset and iterator pages (Milvus's search_params {"radius", "range_filter"}, `offset`, search_iterator; the
 * reference passes none of them, services/milvus_service.py:280-285): for every query the min(k, rows in the band) best rows
 * STRICTLY INSIDE A BAND of the (score desc, id asc) ranking, exact, best first. A row is in the band iff
 *     radius[q] < score                      (radius NULL: no floor)
 *     score <= range_filter[q]               (range_filter NULL: no ceiling; Milvus's rule for IP: radius < distance <= range_filter)
 *     (score, id) ranks strictly behind the cursor (after_scores[q], after_ids[q]): score < after score, or equal score bits and
 *     id > after id (both NULL: no cursor). The cursor is a hit an earlier search of this index returned - its RAW score and its id
 *     (global, as searches return them; on a view the parent's, and an id outside the view still cuts the view's ranking in place).
 * Plain float comparisons on the canonical score; rows whose score is NaN are never hits. Bounds are per query, [nq] each, host
 * pointers or (bounds_on_device = 1) device pointers. k in 1 .. ICD_MAX_K and within the index's max_k.
 *   reweighted = 0  out_raw, out_ids, out_levels in raw order; out_adj is not written.
 *   reweighted = 1  that list through icd_index_search_reweighted's step (adj = (double)raw * w[level], one stable descending
 *                   re-sort of the query's hits): out_adj, out_raw, out_ids, out_levels. The band is on the RAW score.
 * Slots behind the band's last row: score -inf, id -1, level 0. out_levels may be NULL. With no bound at all the outputs equal
 * icd_index_search / icd_index_search_reweighted in ICD_MODE_EXACT bit for bit.
 * ICD_ERR_INVALID before any device call: k out of range, exactly one of after_scores / after_ids, host bounds holding NaN or
 * radius >= range_filter. Device-resident bounds are not validated (that would synchronise): an empty band yields padding.
 * Queries and outputs as in icd_index_search; with device queries, outputs AND bounds the call only enqueues on `stream`
 * (graph-capturable: the bounds' staging is the index's own, allocated at create); host bounds synchronise like host buffers.
 * Up to four queries at k <= 16 are ONE launch (an iterator's page), up to 64 the streaming kernel, more the fp32-MFMA kernel.
 */
int icd_index_search_range(icd_index *idx, const float *queries, int64_t nq, int32_t k, int32_t queries_on_device,
                           const float *radius, const float *range_filter, const float *after_scores, const int64_t *after_ids,
                           int32_t bounds_on_device, int32_t reweighted, double *out_adj, float *out_raw, int64_t *out_ids,
                           int32_t *out_levels, int32_t out_on_device, void *stream);

/*
 * Masked search: a Milvus `filter` applied as a bitset over the index's rows, tested inside the scan - a DIFFERENT filter per
 * query of one batch, and no second index per filter (a view, icd_index_create_view, stays the faster form
 * of ONE filter over a large batch).
 *
 * icd_rowmask_create: the rows of `idx` that may be hits, rows[0 .. n_rows): the index's row indices, strictly increasing, inside
 * [0, n), as for a view (anything else is ICD_ERR_INVALID); host, or device with rows_on_device = 1. n_rows = 0 is allowed: the
 * empty mask. The mask is a device bitset of n / 8 bytes (row r = bit r & 31 of word r >> 5, zero-padded to whole 128-row tiles);
 * a host list is packed on the host and uploaded, a device list is packed by a kernel. Any number of masks per index. A mask
 * keeps no pointer into its index: either may be destroyed first; a search checks that the two belong together (the same
 * handle, the same creation, the same n). On a view: ICD_ERR_UNSUPPORTED - mask the parent. The row-sharded path (icd_group_*)
 * has no masked search.
 *
 * icd_index_search_masked: icd_index_search_range (same arguments, same outputs, same checks) over, for query q, the ranking
 * restricted to the rows of masks[q]: the min(k, rows of the mask inside the band) best of them, best first, then padding
 * (score -inf, id -1, level 0). `masks` is a HOST array of nq handles; a NULL entry leaves that query unfiltered, and with
 * masks NULL or every entry NULL the call IS icd_index_search_range. With the same mask M on every query the outputs equal those
 * of icd_index_create_view(rows of M) searched in ICD_MODE_EXACT, bit for bit; ids are the index's own global ids. An empty mask
 * yields padding. A mask of another index is ICD_ERR_INVALID, a destroyed one ICD_ERR_STATE, a view as `idx`
 * ICD_ERR_UNSUPPORTED. Always exact (the fp16 coarse path has no masked certificate): up to four queries at k <= 16 are ONE
 * launch, up to 64 the streaming kernel, more the fp32-MFMA kernel. The table of bitset pointers goes through staging allocated
 * with the index - nothing is allocated in a search. With device queries, outputs and bounds the call only enqueues on `stream`,
 * like icd_index_search_range (the pinned table is guarded by an event: the NEXT masked call of the index waits until this
 * call's copy of it has run); but the table is filled on the host at call time, so a masked call is NOT graph-capturable
 * (ICD_ERR_INVALID while `stream` is capturing). The event guards the pinned block only: the device copy of the table is ONE
 * buffer per index, like the workspace and the bounds' staging, so the index serves one stream at a time - a masked call
 * enqueued on a second stream while an earlier call's kernels still run on another may overwrite the table under them; order
 * the streams yourself, as for every other search of one index. A mask must outlive the searches that were enqueued with it:
 * icd_rowmask_destroy synchronises the device first.
 */
typedef struct icd_rowmask icd_rowmask;
int icd_rowmask_create(icd_index *idx, const int64_t *rows, int64_t n_rows, int32_t rows_on_device, icd_rowmask **out);
int icd_rowmask_destroy(icd_rowmask *m);
/* rows selected, device bytes held (either pointer may be NULL) */
int icd_rowmask_stats(icd_rowmask *m, int64_t *out_rows, int64_t *out_bytes);
/* The host packer of icd_rowmask_create, on its own (no device, no handle): rows[0 .. n_rows) of an index of n rows ->
 * out_words[0 .. out_count), out_count >= 4 * ceil(n / 128); every word is written (zero where no row is). ICD_ERR_INVALID for a
 * list that is not strictly increasing inside [0, n), or a buffer too short. */
int icd_rowmask_pack(const int64_t *rows, int64_t n_rows, int64_t n, uint32_t *out_words, int64_t out_count);
int icd_index_search_masked(icd_index *idx, icd_rowmask *const *masks, const float *queries, int64_t nq, int32_t k,
                            int32_t queries_on_device, const float *radius, const float *range_filter, const float *after_scores,
                            const int64_t *after_ids, int32_t bounds_on_device, int32_t reweighted, double *out_adj, float *out_raw,
                            int64_t *out_ids, int32_t *out_levels, int32_t out_on_device, void *stream);

/*
 * Hybrid search: Milvus's hybrid_search over dense requests (MilvusClient.hybrid_search(reqs=[AnnSearchRequest, ...], ranker=
 * RRFRanker | WeightedRanker, limit=k); the reference sends one search per phrasing, services/milvus_service.py:280-285, and has
 * no merge of its own). Every query carries R requests, 1 <= R <= ICD_MAX_REQUESTS; request r has a vector, a limit limits[r] in
 * 1 .. ICD_MAX_K shared by all queries of the call, and optionally per (query, request) a row mask and a band. DESIGN.md
 * section 13.
 *   sub-list (q, r)   what icd_index_search_masked returns, raw order, for vector queries[q][r] at k = limits[r] with
 *                     masks[q * R + r], radius[q * R + r], range_filter[q * R + r]; with masks, radius and range_filter all NULL
 *                     what icd_index_search returns in `mode`. Rank j counts from 0; padding slots are not hits.
 *   ICD_RANKER_RRF       fused(id) = sum over r ascending, for every r whose list holds id, of 1.0 / (rrf_c + j_r + 1), in
 *                        double, from 0.0, left to right, every operation rounded once. 0 < rrf_c < 16384 (Milvus: 60).
 *   ICD_RANKER_WEIGHTED  fused(id) = sum over r ascending of weights[r] * norm((double)score_r), product and sum rounded
 *                        separately; weights[r] in [0, 1]; norm: ICD_NORM_NONE s, ICD_NORM_COSINE (1 + s) * 0.5, ICD_NORM_ATAN
 *                        0.5 + atan(s) / pi (Milvus's rule for metric IP; the device's atan need not round as the host's does).
 *   answer            the min(k, distinct ids) best ids by (fused desc, id asc), 1 <= k <= ICD_MAX_K; the other slots are padding:
 *                     fused -inf, id -1, level 0, request bits 0 (adj -inf).
 *   reweighted = 0    out_fused, out_ids, out_levels, out_reqbits in that order; out_adj is not written.
 *   reweighted = 1    that list through icd_index_search_reweighted's step on the double score: out_adj = fused * w[level] and ONE
 *                     stable descending re-sort of the query's hits; fused, ids, levels and request bits travel with the hit.
 *   out_reqbits       uint32 [nq][k]: bit r set iff request r's list held the id. out_levels / out_reqbits may be NULL.
 *
 * icd_fusion_create: the workspace of the hybrid searches of `idx` for up to max_total = nq * R sub-lists per call: their staging
 * (ICD_MAX_K scores and ids each), the staging of host callers (their vectors, and one block of 256 x ICD_MAX_K output slots that
 * a host caller's outputs pass through 256 queries at a time); the per-request limits and weights are copied into the launch. Nothing is allocated in a search. A fusion keeps no pointer into its index: the handle is compared,
 * never followed, and either may be destroyed first. It serves one stream at a time, like the index it belongs to. On an index
 * of 2^31 rows or more: ICD_ERR_UNSUPPORTED. The row-sharded path (icd_group_*) has no hybrid search.
 *
 * icd_index_search_hybrid: queries [nq][R][dim]; masks a HOST array of nq * R handles (NULL entries: unfiltered) or NULL; radius /
 * range_filter nq * R floats each or NULL (host, or device with bounds_on_device = 1; -inf / +inf leave one sub-list unbounded).
 * ONE sub-search over the nq * R vectors at k = max limits[r] into the fusion's staging, then one launch of hybrid_fuse_kernel.
 * ICD_ERR_INVALID before any device call: R, a limit or k out of range, a limit above the index's max_k, nq * R above the
 * fusion's max_total or the index's max_nq, a weight outside [0, 1] or NaN (ICD_RANKER_WEIGHTED), rrf_c out of range
 * (ICD_RANKER_RRF), an unknown ranker / norm / mode, host bounds holding NaN or radius >= range_filter, a fusion or a mask
 * created for another index. A destroyed fusion or mask: ICD_ERR_STATE. On a view bands are allowed and masks are
 * ICD_ERR_UNSUPPORTED, as for icd_index_search_masked; ties break on the local row, which orders as the global id does.
 * With device queries, outputs and bounds and no masks the call only enqueues on `stream` (graph-capturable); with masks it is
 * not graph-capturable, for the reason icd_index_search_masked gives (ICD_ERR_INVALID while capturing).
 */
#define ICD_MAX_REQUESTS 8
typedef struct icd_fusion icd_fusion;
enum { ICD_RANKER_RRF = 0, ICD_RANKER_WEIGHTED = 1 };
enum { ICD_NORM_NONE = 0, ICD_NORM_COSINE = 1, ICD_NORM_ATAN = 2 };
int icd_fusion_create(icd_index *idx, int64_t max_total, icd_fusion **out);
int icd_fusion_destroy(icd_fusion *fusion);
/* sub-lists per call, device bytes held (either pointer may be NULL) */
int icd_fusion_stats(icd_fusion *fusion, int64_t *out_max_total, int64_t *out_bytes);
int icd_index_search_hybrid(icd_index *idx, icd_fusion *fusion, const float *queries, int64_t nq, int32_t R, int32_t queries_on_device,
                            const int32_t *limits, icd_rowmask *const *masks, const float *radius, const float *range_filter,
                            int32_t bounds_on_device, int32_t mode, int32_t ranker, double rrf_c, const double *weights, int32_t norm,
                            int32_t k, int32_t reweighted, double *out_adj, double *out_fused, int64_t *out_ids, int32_t *out_levels,
                            uint32_t *out_reqbits, int32_t out_on_device, void *stream);
/*
 * icd_fusion_fuse_lists: step 2 of icd_index_search_hybrid alone, on the caller's lists - the seam that lets a request be
 * anything that yields a best-first list (a sparse search next to a dense one). scores / ids: DEVICE arrays [nq * R][lmax], list
 * (q, r) at row q * R + r, fp32 scores and global ids of `idx`, best first, padding id -1 (an id outside the index is skipped like
 * padding); list r is read up to limits[r] <= lmax <= ICD_MAX_K. Rankers, answer, outputs, the host-output staging and
 * the errors are icd_index_search_hybrid's; nq * R is bound by the fusion's max_total alone. With device outputs the call only
 * enqueues on `stream` (graph-capturable).
 */
int icd_fusion_fuse_lists(icd_index *idx, icd_fusion *fusion, const float *scores, const int64_t *ids, int64_t nq, int32_t R,
                          int32_t lmax, const int32_t *limits, int32_t ranker, double rrf_c, const double *weights, int32_t norm,
                          int32_t k, int32_t reweighted, double *out_adj, double *out_fused, int64_t *out_ids,
                          int32_t *out_levels, uint32_t *out_reqbits, int32_t out_on_device, void *stream);

/*
 * Grouped hybrid search: group_by_field / group_size on hybrid_search. DESIGN.md section 15 (rules H1 - H6).
 *   sub-lists         list (q, r) is icd_index_search_grouped's RAW output for that vector at k = limits[r] GROUPS and group_size
 *                     members; limits[r] >= 1, limits[r] * group_size <= ICD_MAX_K. One sub-search runs at the largest limit and
 *                     list r is cut in front of its (limits[r] + 1)-th RUN of equal group ids; rank j is the slot index.
 *   fused(id)         icd_index_search_hybrid's rules (RRF, Weighted with none / cosine / atan), unchanged.
 *   answer            the distinct fused ids grouped by the grouping; members rank by (fused desc, id asc), a group by its best
 *                     member: the min(k, groups present) best groups times the min(group_size, members) best rows,
 *                     group-rank-major, hits contiguous, [nq][k * group_size]; padding -inf, -1, 0, 0, -1. k * group_size <=
 *                     ICD_MAX_K. reweighted = 1: adj = fused * w[level], ONE stable descending re-sort; group id and request
 *                     bits travel with the hit. Every row its own group and group_size = 1 IS icd_index_search_hybrid in
 *                     ICD_MODE_EXACT, bit for bit.
 * icd_fusion_fuse_lists_grouped: the same cut by runs and the same fuse on caller-provided device lists [nq * R][lmax]; a hit's
 * group is read from the grouping by row (a slot whose id is no row of the index is a run of its own and no hit).
 * Every check comes before the first device call. ICD_ERR_INVALID: what icd_index_search_hybrid refuses, k * group_size or
 * limits[r] * group_size above ICD_MAX_K, nq * R above the grouping's max_nq or the fusion's max_total, a fusion or grouping of
 * another index, ANY mask table or bound (filter with a view: the grouping is then the view's). ICD_ERR_STATE: a destroyed handle.
 * Lock order: fusion, grouping. With device buffers the calls only enqueue. A host caller's groups leave through the grouping's
 * staging.
 */
int icd_index_search_hybrid_grouped(icd_index *idx, icd_fusion *fusion, icd_grouping *grouping, const float *queries, int64_t nq, int32_t R,
                                    int32_t queries_on_device, const int32_t *limits, icd_rowmask *const *masks, const float *radius,
                                    const float *range_filter, int32_t ranker, double rrf_c, const double *weights, int32_t norm, int32_t k,
                                    int32_t group_size, int32_t reweighted, double *out_adj, double *out_fused, int64_t *out_ids,
                                    int32_t *out_levels, uint32_t *out_reqbits, int32_t *out_groups, int32_t out_on_device, void *stream);
int icd_fusion_fuse_lists_grouped(icd_index *idx, icd_fusion *fusion, icd_grouping *grouping, const float *scores, const int64_t *ids,
                                  int64_t nq, int32_t R, int32_t lmax, const int32_t *limits, int32_t ranker, double rrf_c,
                                  const double *weights, int32_t norm, int32_t k, int32_t group_size, int32_t reweighted, double *out_adj,
                                  double *out_fused, int64_t *out_ids, int32_t *out_levels, uint32_t *out_reqbits, int32_t *out_groups,
                                  int32_t out_on_device, void *stream);

/*
 * Sparse-vector search: Milvus's SPARSE_FLOAT_VECTOR field searched with metric IP (usually filled by its BM25 function), alone
 * or as one request of a hybrid search through icd_fusion_fuse_lists. DESIGN.md section 14.
 *   index             row i of an index of n rows carries a set of (term, value) pairs in CSR form (row_off[n + 1], terms, vals):
 *                     term a uint32 in [0, vocab), strictly increasing within a row, value a finite non-zero fp32; a row may be
 *                     empty. Not on a view, not on the row-sharded path (icd_group_*), n < 2^31. A built sparse index is not
 *                     mutated: rebuild it.
 *   query             0 .. ICD_SPARSE_MAX_QUERY_TERMS pairs under the same rules (q_off[nq + 1], q_terms, q_vals); a query
 *                     without pairs yields padding.
 *   score(q, i)       the sum over the terms t present in both, ascending t, of q_t * d_it: every product rounded once to
 *                     fp32, the sum fp32 from 0.0f left to right, no FMA. A row that shares no term with the query is NOT a hit,
 *                     whatever k is (Milvus's behaviour); a shared term makes the row a hit even when the sum is 0 or below.
 *                     Sums that overflow fp32 are outside the contract.
 *   answer            the min(k, hits) best rows by (score desc, id asc), 1 <= k <= ICD_MAX_K, then padding (score -inf, id -1,
 *                     level 0); ids are global (id_base + row). masks: NULL, or a HOST array of nq row-mask handles of `idx`
 *                     (NULL entries: unmasked) that restrict a query's hits to the mask's rows.
 *   reweighted = 0    out_raw, out_ids, out_levels in that order; out_adj is not written.
 *   reweighted = 1    icd_index_search_reweighted's step: out_adj = (double)raw * w[level], ONE stable descending re-sort.
 *                     out_levels may be NULL.
 *
 * icd_sparse_pack (host only: no device, no handle): checks the rows and builds the inverted index the kernels walk -
 * post_off[vocab + 1], post_row / post_val [row_off[n]], every term's postings by ascending row (a stable counting sort).
 * Nothing is written when the input is refused.
 *
 * icd_sparse_create: packs the host CSR rows (n = the index's n), uploads the postings and allocates every workspace of the
 * searches for up to max_nq queries at k <= max_k: a host caller's query and output staging and the [tiles][max_nq][max_k]
 * partial lists (tiles of icd_sparse_tile_rows() rows). Nothing is allocated in a search. The handle keeps no pointer into its
 * index - it is compared, never followed - and either may be destroyed first; it serves one stream at a time. A masked
 * search reads the index's mask table and so also falls under the index's own one-stream-at-a-time rule, like every masked search.
 *
 * icd_sparse_search: one launch of sparse_accumulate_select_kernel over (query, tile) and one of sparse_merge_kernel. Every check
 * comes before the first device call. ICD_ERR_INVALID: unsorted or duplicate terms, a term >= vocab, a non-finite or zero
 * value, a query longer than ICD_SPARSE_MAX_QUERY_TERMS, k or nq above the handle's limits (nq above the index's max_nq with
 * masks), a sparse index or a mask created for another index. ICD_ERR_UNSUPPORTED: a view, n >= 2^31. ICD_ERR_STATE: a
 * destroyed handle. With queries_on_device = 1 the pairs cannot be read on the host: the call TRUSTS strictly increasing terms
 * (a term >= vocab is skipped, a query is cut at ICD_SPARSE_MAX_QUERY_TERMS pairs; unsorted or repeated terms give sums in
 * another order). With device queries and outputs and no masks the call only enqueues on `stream` (graph-capturable); with masks
 * it is not, for the reason icd_index_search_masked gives. Range bounds and the cursor of offset and iterator pages are
 * icd_sparse_search_range; grouping is icd_sparse_search_grouped below.
 *
 * icd_sparse_search_range: icd_index_search_range's band on the sparse ranking, exact. DESIGN.md section 16. Of a query's hits
 * (the rows that share a term with it, inside its row mask) only those with radius[q] < score <= range_filter[q] (plain float
 * compares on the canonical sum) that rank strictly behind the cursor (after_scores[q], after_ids[q]) - a smaller score, or equal
 * score bits and a larger global id - are ranked; the answer is the min(k, hits in the band) best of them, best first, then
 * padding. Any bound array may be NULL (no such bound); after_scores and after_ids come together. A row without a shared term
 * is no hit under any band (radius = -inf admits none). reweighted = 1 reweights and re-sorts those k; the band is on the raw
 * score. With all four bound arrays NULL the call IS icd_sparse_search (the same kernel instantiations, bit for bit); otherwise
 * one launch of sparse_accumulate_select_kernel<true>, which applies the band before the tile's k best are selected, and
 * sparse_merge_kernel. bounds_on_device = 0: [nq] host arrays, checked (ICD_ERR_INVALID: a NaN bound, radius >= range_filter)
 * and packed on the host into the handle's pinned block - the call synchronises; 1: [nq] device arrays, packed by one launch
 * (a NaN or inverted band there is an empty band: padding). Every check icd_sparse_search makes is made here too, and
 * ICD_ERR_INVALID when only one of after_scores / after_ids is given; all before the first device call. The bands' staging
 * (max_nq entries on the device, as many in pinned host memory) belongs to the sparse handle: nothing is allocated in a search.
 * With device queries, bounds and outputs and no masks the call only enqueues (graph-capturable); with masks it is not.
 */
typedef struct icd_sparse icd_sparse;
#define ICD_SPARSE_MAX_QUERY_TERMS 64
/* rows per tile of the sparse search kernel (a build constant; tests place their shapes around it) */
int icd_sparse_tile_rows(void);
int icd_sparse_pack(const int64_t *row_off, const uint32_t *terms, const float *vals, int64_t n, int64_t vocab,
                    int64_t *post_off, uint32_t *post_row, float *post_val);
int icd_sparse_create(icd_index *idx, const int64_t *row_off, const uint32_t *terms, const float *vals, int64_t vocab,
                      int32_t max_nq, int32_t max_k, icd_sparse **out);
int icd_sparse_destroy(icd_sparse *sp);
/* vocabulary size, postings, device bytes held (any pointer may be NULL) */
int icd_sparse_stats(icd_sparse *sp, int64_t *out_vocab, int64_t *out_nnz, int64_t *out_bytes);
int icd_sparse_search(icd_index *idx, icd_sparse *sp, const int64_t *q_off, const uint32_t *q_terms, const float *q_vals,
                      int64_t nq, int32_t k, int32_t queries_on_device, icd_rowmask *const *masks, int32_t reweighted,
                      double *out_adj, float *out_raw, int64_t *out_ids, int32_t *out_levels, int32_t out_on_device, void *stream);
int icd_sparse_search_range(icd_index *idx, icd_sparse *sp, const int64_t *q_off, const uint32_t *q_terms, const float *q_vals,
                            int64_t nq, int32_t k, int32_t queries_on_device, icd_rowmask *const *masks,
                            const float *radius, const float *range_filter, const float *after_scores, const int64_t *after_ids,
                            int32_t bounds_on_device, int32_t reweighted,
                            double *out_adj, float *out_raw, int64_t *out_ids, int32_t *out_levels, int32_t out_on_device, void *stream);

/*
 * Grouped sparse search: group_by_field / group_size on a sparse field. DESIGN.md section 15.
 *   hits, scores      icd_sparse_search's: only rows that share a term with the query and lie inside the query's row mask
 *                     (masks ARE allowed here: the sparse index has no views, a mask is its only filter).
 *   answer            among the hits, a group's members rank by (score desc, id asc), a group by its best member's key: the
 *                     min(k, groups with a hit) best groups and of each its min(group_size, hit members) best rows; layout,
 *                     padding (-inf, -1, 0, -1) and the reweighted form are icd_index_search_grouped's. k >= 1,
 *                     group_size >= 1, k * group_size <= ICD_MAX_K. Every row its own group and group_size = 1 IS
 *                     icd_sparse_search at the same k, bit for bit; one group at group_size = m IS icd_sparse_search at k = m.
 *
 * icd_grouping_pair_sparse: once per (grouping, sparse index of the same index), outside any search: builds the grouping's
 * row -> position table (n * 4 bytes the grouping owns, counted in icd_grouping_stats from then on; a grouping that is never
 * paired reports what it always did). Idempotent. A grouped sparse search with an unpaired grouping is ICD_ERR_STATE.
 *
 * icd_sparse_search_grouped: per pass of the grouping's query block one launch of sparse_store_kernel (the accumulate phase of
 * icd_sparse_search, the tile's sums stored into the grouping's score block, a NaN for a row that is no hit) and the two
 * reduction kernels of icd_index_search_grouped. Every check comes before the first device call. ICD_ERR_INVALID: what
 * icd_sparse_search refuses, k * group_size > ICD_MAX_K, nq above the sparse index's or the grouping's max_nq, a sparse index,
 * grouping or mask created for another index. ICD_ERR_STATE: a destroyed handle. The handles may be destroyed in any order.
 * Nothing is allocated. With device queries and outputs and no masks the call only enqueues on `stream`. The call holds the
 * sparse index's, then the grouping's, then (masked) the index's lock: one stream at a time per handle.
 */
int icd_grouping_pair_sparse(icd_index *idx, icd_grouping *grouping, icd_sparse *sp);
int icd_sparse_search_grouped(icd_index *idx, icd_sparse *sp, icd_grouping *grouping, const int64_t *q_off, const uint32_t *q_terms,
                              const float *q_vals, int64_t nq, int32_t k, int32_t group_size, int32_t queries_on_device,
                              icd_rowmask *const *masks, int32_t reweighted, double *out_adj, float *out_raw, int64_t *out_ids,
                              int32_t *out_levels, int32_t *out_groups, int32_t out_on_device, void *stream);

/*
 * Keyword match filters: Milvus's TEXT_MATCH(field, "tokens") predicate as row masks, one per query of a batch, built on the
 * device from the sparse index's postings. DESIGN.md section 17.
 *   query q           its distinct known terms q_terms[q_off[q] .. q_off[q + 1]) - icd_sparse_search's rules: strictly increasing,
 *                     below the vocabulary, at most ICD_SPARSE_MAX_QUERY_TERMS - and min_match[q] in 1 .. 64.
 *   mask q            row r is set iff it holds at least min_match[q] of the query's terms AND (base_masks[q] != NULL) lies in
 *                     that base mask. A query without terms, or with min_match above its number of terms, gives the empty mask.
 *
 * icd_sparse_match_rowmasks: creates nq masks of `idx` with one launch of text_match_mask_kernel over (query, tile) on `stream`.
 * out_masks: a HOST array of nq handles. The masks are ordinary icd_rowmask handles in icd_rowmask_create's layout: every masked
 * entry point accepts them, icd_rowmask_stats reports their row count (counted by the kernel and read back by the first such
 * call, which synchronises the device), icd_rowmask_read their words, icd_rowmask_destroy frees them - each alone, in any order,
 * before or after the index (the bitsets of one call share one allocation, released with the last of them). Creation allocates;
 * it is not a search and not graph-capturable (ICD_ERR_INVALID while `stream` is capturing). Masked searches enqueued later on the
 * same stream see the finished bitsets. base_masks: NULL, or a HOST array of nq handles of `idx` (NULL entries: no base); a base
 * mask must outlive the call's kernel, as a mask outlives its searches. With host queries or any base mask the call synchronises
 * the stream before it returns; with queries_on_device = 1 (q_off, q_terms AND min_match are device pointers) and no base mask
 * it only enqueues, and trusts the queries as icd_sparse_search does (a term >= vocab is skipped, a query is cut at 64 terms, a
 * min_match outside 1 .. 64 matches nothing).
 * Every check comes before the first device call; on any error no mask is created and every out_masks[q] is NULL.
 * ICD_ERR_INVALID: unsorted or duplicate terms, a term >= vocab, a query longer than 64 terms, min_match outside 1 .. 64, a sparse
 * index or a base mask created for another index, NULL arrays. ICD_ERR_STATE: a destroyed index, sparse index or base mask.
 * ICD_ERR_UNSUPPORTED: a view as `idx`. nq = 0 creates nothing.
 *
 * icd_rowmask_read: a mask's words on the host, in icd_rowmask_pack's layout, for every mask however it was made; out_count >=
 * 4 * ceil(n / 128) (else ICD_ERR_INVALID). Synchronises the device.
 */
int icd_sparse_match_rowmasks(icd_index *idx, icd_sparse *sp, const int64_t *q_off, const uint32_t *q_terms, const int32_t *min_match,
                              int64_t nq, int32_t queries_on_device, icd_rowmask *const *base_masks, icd_rowmask **out_masks, void *stream);
int icd_rowmask_read(icd_rowmask *m, uint32_t *out_words, int64_t out_count);

/*
 * Filter expressions on the device: the row masks of a batch of boolean filter programs, one per query, any shape of AND / OR / NOT
 * over integer predicates on the rows' columns and keyword matches on the sparse index. DESIGN.md section 18.
 *
 * icd_columns: `ncols` int32 columns of the n rows of ONE index (not a view: ICD_ERR_UNSUPPORTED, as is n >= 2^31), uploaded once
 * from the HOST array cols[ncols][n] (1 <= ncols <= ICD_FILTER_MAX_COLUMNS). The library knows only "int32 column c": what a value
 * means (a level, a flag, the rank of a string among the sorted distinct strings) is the caller's. The handle keeps no pointer into
 * its index - it is compared, never followed - and either may be destroyed first. icd_columns_stats: columns, rows, device bytes
 * (any pointer may be NULL).
 *
 * A program is a postfix sequence of operations over a stack of row sets; query q's program is the uint32 words
 * prog[prog_off[q] .. prog_off[q + 1]) (prog_off[0] = 0). The first word of an operation holds its kind in bits 0 .. 7:
 *   ICD_FILTER_RANGE  { 1, col, lo, hi }                         push the rows with lo <= column[col][row] < hi; lo and hi are int32
 *                                                                bit patterns, lo >= hi is the empty set
 *   ICD_FILTER_SET    { 2 | count << 8, col, ids[count] }        push the rows whose value is one of ids (int32 bit patterns, strictly
 *                                                                increasing as int32); count 0 .. 64, 0 is the empty set
 *   ICD_FILTER_TEXT   { 3 | count << 8 | m << 16, terms[count] } push the rows that hold at least m of the terms, under
 *                                                                icd_sparse_match_rowmasks' rules: terms strictly increasing and
 *                                                                below the vocabulary, count 0 .. 64, m 1 .. 64; m > count is the
 *                                                                empty set. Needs the sparse index.
 *   ICD_FILTER_AND { 4 }, ICD_FILTER_OR { 5 }                    pop two sets, push their intersection / union
 *   ICD_FILTER_NOT { 6 }                                         replace the top set by its complement within the index's n rows
 * All other bits of a first word are 0. A program holds 1 .. 32 operations, at most 16 leaves (RANGE, SET, TEXT) of which at most
 * 4 are TEXT, never more than 8 sets on the stack, never pops from an empty stack and ends with exactly ONE set: mask q.
 *
 * icd_filter_program_check (host only: no device, no handle): validates nq programs against `ncols` columns and a vocabulary of
 * `vocab` terms (0: no sparse index - a TEXT leaf is refused): structure, stack discipline and every bound above. ICD_OK, or
 * ICD_ERR_INVALID with the reason in msg (msg_len bytes, NUL-terminated; msg may be NULL) and in icd_last_error.
 *
 * icd_filter_rowmasks: creates nq masks of `idx` with ONE launch of filter_mask_kernel over (query, tile) on `stream`; mask q = the
 * program's set AND (base_masks[q] != NULL) that base mask. sparse: the index's sparse index, or NULL when no program holds a TEXT
 * leaf. Programs always come from HOST memory and are checked (icd_filter_program_check's rules) before any device call. The masks
 * are ordinary icd_rowmask handles, exactly as icd_sparse_match_rowmasks makes them: every masked entry point accepts them,
 * icd_rowmask_stats reports the row count the kernel counted, icd_rowmask_read their words, icd_rowmask_destroy frees them - each
 * alone, in any order, before or after the index, the columns and the sparse index (the bitsets of one call share one allocation,
 * released with the last of them). The call allocates and synchronises `stream` before it returns: not graph-capturable
 * (ICD_ERR_INVALID while `stream` is capturing). On any error no mask is created and every out_masks[q] is NULL.
 * ICD_ERR_INVALID: a program the checker refuses (a TEXT leaf with sparse = NULL among them), columns, a sparse index or a base
 * mask created for another index, NULL arrays. ICD_ERR_STATE: a destroyed index, columns, sparse index or base mask.
 * ICD_ERR_UNSUPPORTED: a view as `idx`. nq = 0 creates nothing.
 */
typedef struct icd_columns icd_columns;
#define ICD_FILTER_MAX_COLUMNS 256
#define ICD_FILTER_RANGE 1
#define ICD_FILTER_SET 2
#define ICD_FILTER_TEXT 3
#define ICD_FILTER_AND 4
#define ICD_FILTER_OR 5
#define ICD_FILTER_NOT 6
int icd_columns_create(icd_index *idx, const int32_t *cols, int32_t ncols, icd_columns **out);
int icd_columns_destroy(icd_columns *columns);
int icd_columns_stats(icd_columns *columns, int32_t *out_ncols, int64_t *out_rows, int64_t *out_bytes);
int icd_filter_program_check(const int64_t *prog_off, const uint32_t *prog, int64_t nq, int32_t ncols, int64_t vocab, char *msg, int64_t msg_len);
int icd_filter_rowmasks(icd_index *idx, icd_columns *columns, icd_sparse *sparse, const int64_t *prog_off, const uint32_t *prog, int64_t nq,
                        icd_rowmask *const *base_masks, icd_rowmask **out_masks, void *stream);

/*
 * The ordered select over a batch of row masks: what a Milvus query / count(*) / query_iterator asks of a filter once no vector is
 * involved. For every query q of the batch:
 *
 *   out_total[q]            the rows set in masks[q] (a NULL entry: every row of the index, n)
 *   out_taken[q]            clamp(out_total[q] - offsets[q], 0, limit)
 *   out_ids[q][0 .. limit)  the rows of ranks offsets[q] .. offsets[q] + out_taken[q] of the mask in ascending row order, then -1.
 *                           Rows as icd_rowmask_create takes them: 0 .. n - 1 (a hit's id is the row plus the index's id_base).
 *
 * icd_rowmask_select: two launches on `stream` whatever nq and the masks hold (mask_count_kernel, mask_select_kernel over
 * (query, segment of 16 384 rows)); no atomic touches the outputs: the same bytes on every run. masks: icd_index_search_masked's
 * rules - a HOST array of nq entries, each NULL or a live mask of `idx`, staged through the index's pinned table (ICD_ERR_INVALID
 * while `stream` is capturing). offsets: a HOST array of nq entries >= 0, or NULL for 0. limit: 1 .. ICD_SELECT_MAX_LIMIT.
 * out_ids may be NULL: a count (out_taken may then be NULL too). out_on_device = 1: the outputs are device memory and the call only
 * enqueues; 0: host memory, written when the call returns, and nq * limit is bounded by the staging the index allocated at create
 * (max(64 * max_nq, 4 * ICD_SELECT_MAX_LIMIT) ids; ICD_ERR_INVALID above it: use device outputs). Nothing is allocated in a call.
 * Every check comes before the first device call: ICD_ERR_INVALID for a limit or an offset out of range, nq above the index's
 * max_nq, a mask of another index, NULL arrays; ICD_ERR_STATE for a destroyed index or mask; ICD_ERR_UNSUPPORTED for a view as
 * `idx`. nq = 0 does nothing.
 */
#define ICD_SELECT_MAX_LIMIT 16384
int icd_rowmask_select(icd_index *idx, icd_rowmask *const *masks, int64_t nq, const int64_t *offsets, int32_t limit, int64_t *out_ids,
                       int64_t *out_total, int32_t *out_taken, int32_t out_on_device, void *stream);

/*
 * Facet counts: how the rows of every mask of a batch spread over the groups of a grouping - the terms aggregation of a search
 * front end, the count that goes with group_by_field. For every query q and every group j of `grouping`:
 *
 *   out_counts[q][j]        the rows r with bit r set in masks[q] (a NULL entry: every row of the index) whose group is the j-th
 *                           smallest distinct id of the grouping's group_of - the dense number icd_grouping_create assigns.
 *                           int32 [nq][G], G from icd_grouping_stats; a row of it sums to the mask's icd_rowmask_select total.
 *
 * One memset and ONE launch on `stream` (facet_count_kernel over (query, segment of 16 384 rows)) whatever nq and the masks hold.
 * The counts are summed with integer atomic adds, in LDS up to 8 192 groups and in the output above it: integer addition commutes,
 * the result is the same bytes on every run. The call zeroes the output itself: nothing of an earlier call shows. masks:
 * icd_rowmask_select's rules - a HOST array of nq entries, each NULL or a live mask of `idx`, staged through the index's pinned table
 * (ICD_ERR_INVALID while `stream` is capturing). out_on_device = 1: out_counts is device memory and the call only enqueues; 0: host
 * memory, written when the call returns - the counts go through the grouping's per-group key block (idle outside a grouped search,
 * taken under the grouping's lock; twice its query block of queries per launch, a longer batch runs in passes). Nothing is
 * allocated in a call. Every check comes before the first device call: ICD_ERR_INVALID for nq above the index's max_nq, a mask or a
 * grouping of another index, NULL arrays; ICD_ERR_STATE for a destroyed index, grouping or mask; ICD_ERR_UNSUPPORTED for a view as
 * `idx` and for a grouping that was created on a view (group and mask the parent). nq = 0 does nothing. A refused call leaves the
 * index and the grouping usable. The row-sharded path (icd_group_*) has no facet call: count on every shard and add the rows.
 */
int icd_rowmask_group_counts(icd_index *idx, icd_grouping *grouping, icd_rowmask *const *masks, int64_t nq,
                             int32_t *out_counts /* [nq][G] */, int32_t out_on_device, void *stream);

/*
 * MMR search: the k best rows that are not copies of each other - maximal marginal relevance over the exact candidate list, what
 * LangChain's Milvus vector store does on the host in max_marginal_relevance_search(query, k, fetch_k, lambda_mult) (DESIGN.md
 * section 21). Per query q, with 1 <= k <= fetch_k <= ICD_MAX_K, fetch_k <= the index's max_k and lambda a double in [0, 1]:
 *   candidates        what icd_index_search_masked returns for the query at k = fetch_k, reweighted = 0, with the call's masks /
 *                     radius / range_filter (no cursor); with no mask and no bound what icd_index_search_range returns, the
 *                     ICD_MODE_EXACT list. Candidate i has row r_i, raw score rel_i (the canonical score) and a level; C is the
 *                     number of real hits, padding slots are not candidates.
 *   sim(i, j)         the canonical score of row r_j with row r_i as the query: the strict d-ascending fmaf chain from +0.0f over
 *                     the fp32 rows the index holds (oracle/icd_oracle.c chain_score); symmetric in its two rows.
 *   picks             pick 0 is candidate 0. For t >= 1 every unpicked i has pen_i, the float maximum of sim(i, s) over the picked
 *                     s: it starts at sim(i, pick 0) and is updated with plain `s > pen ? s : pen`. value_i = lambda * (double)rel_i
 *                     - (1 - lambda) * (double)pen_i: the two products and the difference each rounded once, in double, no
 *                     contraction; 1 - lambda is computed once on the host. The pick is the unpicked candidate of the greatest
 *                     value under plain `>`, ties to the lower candidate index (the better (score desc, id asc) rank). A NaN value
 *                     never wins; when no unpicked candidate has a comparable value the lowest unpicked index is taken. Picking
 *                     stops after min(k, C) picks.
 *   reweighted = 0    pick order: out_raw, out_ids, out_levels, out_mmr [nq][k]; out_mmr is a double, the value the pick won with
 *                     (pick 0 carries lambda * rel_0). out_adj is not written.
 *   reweighted = 1    the picked hits through icd_index_search_reweighted's step: adj = (double)raw * w[level], ONE stable descending
 *                     re-sort; raw, id, level and mmr value travel with the hit.
 *   unused slots      score -inf, id -1, level 0, mmr -inf, adj -inf. out_levels and out_mmr may be NULL.
 * lambda = 1 returns icd_index_search_masked at k bit for bit (reweighted = 1: that call's reweighted form); k = fetch_k returns a
 * permutation of the candidate list.
 *
 * icd_mmr_create: the workspace of the MMR searches of `idx` for up to max_nq queries per call: the staging of the candidate
 * lists ([max_nq][ICD_MAX_K] raw scores, ids, levels) and of a host caller's outputs. Nothing is allocated in a search. The handle
 * keeps no pointer into its index: it is compared, never followed, and either may be destroyed first. It serves one stream at a
 * time, like the index it belongs to. A view has no MMR search (ICD_ERR_UNSUPPORTED: mask the parent), nor has the row-sharded
 * path (icd_group_*).
 *
 * icd_index_search_mmr: ONE sub-search at fetch_k into the staging, then one launch of mmr_select_kernel (one work-group per
 * query; no atomics: the same call twice gives the same bytes). masks: a HOST array of nq handles (NULL entries: unfiltered) or
 * NULL; radius / range_filter: nq floats each or NULL, host or (bounds_on_device = 1) device. Masks, bounds, synchronisation and
 * the capture rule are icd_index_search_masked's. Every check comes before the first device call. ICD_ERR_INVALID: k or fetch_k
 * out of range, k > fetch_k, fetch_k above the index's max_k, nq above the handle's or the index's max_nq, lambda outside [0, 1]
 * or NaN, host bounds holding NaN or radius >= range_filter, a handle or a mask of another index. ICD_ERR_STATE: a destroyed
 * handle or mask. ICD_ERR_UNSUPPORTED: a view as `idx`. nq = 0 does nothing. A refused call leaves outputs and handles as they were.
 */
typedef struct icd_mmr icd_mmr;
int icd_mmr_create(icd_index *idx, int64_t max_nq, icd_mmr **out);
int icd_mmr_destroy(icd_mmr *mmr);
/* queries per call, device bytes held (either pointer may be NULL) */
int icd_mmr_stats(icd_mmr *mmr, int64_t *out_max_nq, int64_t *out_bytes);
int icd_index_search_mmr(icd_index *idx, icd_mmr *mmr, icd_rowmask *const *masks, const float *queries, int64_t nq, int32_t k,
                         int32_t fetch_k, double lambda, int32_t queries_on_device, const float *radius, const float *range_filter,
                         int32_t bounds_on_device, int32_t reweighted, double *out_adj, float *out_raw, int64_t *out_ids,
                         int32_t *out_levels, double *out_mmr, int32_t out_on_device, void *stream);

/*
 * Boosted search: Milvus 2.6's boost ranker ({"reranker": "boost", "filter", "weight"}) - "rows that match this filter count
 * `weight` times as much" - applied BEFORE the top-k is chosen, exact over every row. A query carries up to
 * ICD_MAX_BOOSTS boosts (M_j, w_j): M_j a row mask of the index, w_j an fp32 weight. Per query q and row r:
 *   boosted(q, r)     starts as the canonical fp32 score of the row (oracle/icd_oracle.c chain_score); for j = 0, 1, 2, 3 in that
 *                     order, if slot j is in use and r is in M_j: s = s * w_j - ONE IEEE fp32 multiply, rounded once, subnormals
 *                     kept, fused with nothing. The slot order is part of the contract: rounding does not commute.
 *   ranking           (boosted desc, id asc). The query's filter mask (masks[q]), radius, range_filter and the cursor
 *                     (after_scores / after_ids) apply to the BOOSTED score and ranking exactly as icd_index_search_masked applies
 *                     them to the raw one: a cursor pages through the boosted ranking. A row whose boosted score is NaN or -inf is
 *                     not a hit; +inf is an ordinary score and ranks first.
 *   outputs           icd_index_search_masked's: out_raw carries the boosted score, reweighted = 1 runs the level reweight on it
 *                     (adj = (double)boosted * w[level], one stable re-sort); padding as there (-inf, id -1, level 0).
 * With every slot unused the outputs are icd_index_search_masked's bit for bit; a boost of weight exactly 1.0f changes nothing.
 *
 * icd_boost_create: the workspace of the boosted searches of `idx` for up to max_nq queries per call: the pinned block the call's
 * boost table is filled in, its device copy, the event that guards the block. Nothing is allocated in a search. The handle keeps
 * no pointer into its index: it is compared, never followed, and either may be destroyed first. It serves one stream at a time,
 * like the index it belongs to. A view has no boosted search (ICD_ERR_UNSUPPORTED: mask the parent), nor has the row-sharded path
 * (icd_group_*): boost on every shard and merge.
 *
 * icd_index_search_boosted: icd_index_search_masked's dispatch and launches, on the kernel instantiations that carry the multiply
 * (up to four queries at k <= 16 one launch, up to 64 the streaming kernel, more the fp32-MFMA kernel). masks: a HOST array of nq
 * handles (NULL entries: unfiltered) or NULL. boost_masks: a HOST array [nq][ICD_MAX_BOOSTS] of handles, NULL = slot unused (holes
 * are allowed: the used slots still apply in slot order), or NULL = no boost at all. boost_weights: HOST floats
 * [nq][ICD_MAX_BOOSTS], read where the mask is not NULL. Bounds, cursor, outputs and synchronisation are
 * icd_index_search_masked's. The boost table is filled on the host at call time, so the call cannot be captured into a graph:
 * ICD_ERR_INVALID on a capturing stream. Every check comes before the first device call. ICD_ERR_INVALID: a weight of a used
 * slot that is NaN, infinite, <= 0 or subnormal, a boost mask, a mask or a workspace of another index, nq above the workspace's
 * or the index's max_nq, and whatever icd_index_search_masked refuses. ICD_ERR_STATE: a destroyed mask, workspace or index.
 * ICD_ERR_UNSUPPORTED: a view as `idx`. nq = 0 does nothing. A refused call leaves outputs and handles as they were.
 */
#define ICD_MAX_BOOSTS 4
typedef struct icd_boost icd_boost;
int icd_boost_create(icd_index *idx, int64_t max_nq, icd_boost **out);
int icd_boost_destroy(icd_boost *b);
/* queries per call, bytes held (either pointer may be NULL) */
int icd_boost_stats(icd_boost *b, int64_t *out_max_nq, int64_t *out_bytes);
int icd_index_search_boosted(icd_index *idx, icd_boost *ws, icd_rowmask *const *masks,
                             icd_rowmask *const *boost_masks /* host [nq][ICD_MAX_BOOSTS], NULL = slot unused */,
                             const float *boost_weights      /* host [nq][ICD_MAX_BOOSTS], read where the mask is not NULL */,
                             const float *queries, int64_t nq, int32_t k, int32_t queries_on_device,
                             const float *radius, const float *range_filter, const float *after_scores, const int64_t *after_ids,
                             int32_t bounds_on_device, int32_t reweighted, double *out_adj, float *out_raw, int64_t *out_ids,
                             int32_t *out_levels, int32_t out_on_device, void *stream);

/*
 * Search by stored rows: Milvus 2.6's search by primary key - the stored vector of an entity is the query - for "which rows are
 * closest to this one?", a related-rows table (every row's neighbours) and a near-duplicate sweep. DESIGN.md section 23. Query q
 * names a row of the index by its global id, ids[q] in [id_base, id_base + n).
 *   answer            icd_index_search_masked's answer (masks[q], radius[q], range_filter[q], no cursor) for the row's stored
 *                     fp32 values as the query vector, ranked over every row EXCEPT row ids[q] itself: the min(k, such rows in the
 *                     mask and band) best by (score desc, id asc), then padding (score -inf, id -1, level 0). The raw form is
 *                     icd_index_search_masked's list at k + 1 with the entry of id ids[q] removed and the gap closed, or, where
 *                     that id is not in it (the row is outside its own mask or band, or holds a NaN), without its last entry.
 *                     Bit-identical rows tie with the row itself and the smaller ids come first: the self hit is not always rank 0.
 *   reweighted = 1    icd_index_search_reweighted's step on those k: out_adj = (double)raw * w[level], ONE stable descending
 *                     re-sort. Where the row is outside its own mask or band this IS icd_index_search_masked at k.
 *   include_self = 1  skips the removal: icd_index_search_masked at k, bit for bit.
 *   k                 1 .. ICD_MAX_K - 1 (include_self = 1: ICD_MAX_K); the sub-search runs at k + 1, which the index's max_k bounds.
 * The same id may appear any number of times in a batch. An index of one row yields padding.
 *
 * icd_byrows_create: the workspace of the searches by rows of `idx` for up to max_nq queries per call: the query block the rows
 * are gathered into, the (k + 1)-wide lists, a host caller's ids and outputs. Nothing is allocated in a search. The handle keeps
 * no pointer into its index: it is compared, never followed, and either may be destroyed first. It serves one stream at a time,
 * like the index it belongs to. A view has no search by rows (ICD_ERR_UNSUPPORTED: mask the parent), nor has the row-sharded path.
 *
 * icd_index_search_by_rows: three steps on `stream`: byrows_gather_kernel (the rows -> the query block, on the device: no vector
 * crosses the bus), icd_index_search_masked's request at k + 1 with device queries and device outputs (the same dispatch: up to
 * four queries at k <= 16 one launch, up to 64 the streaming kernel, more the fp32-MFMA kernel), byrows_drop_self_kernel. ids:
 * int64 [nq], host or (ids_on_device = 1) device; masks, radius, range_filter, bounds_on_device, outputs and synchronisation are
 * icd_index_search_masked's, and so is the capture rule: with device ids, outputs and bounds and no masks the call only enqueues
 * (graph-capturable), otherwise ICD_ERR_INVALID while `stream` is capturing. Device ids are not read on the host: one outside the
 * index searches with a zero vector, never forms an address, and its outputs are padding; the other queries are not affected.
 * Every check comes before the first device call. ICD_ERR_INVALID: a host id outside the index, k out of range (k = ICD_MAX_K with
 * include_self = 0 among them) or k + 1 above the index's max_k, nq above the workspace's or the index's max_nq, a workspace or
 * a mask of another index, and whatever icd_index_search_masked refuses. ICD_ERR_STATE: a destroyed index, workspace or mask.
 * ICD_ERR_UNSUPPORTED: a view as `idx`. nq = 0 does nothing. A refused call leaves outputs as they were.
 */
typedef struct icd_byrows icd_byrows;
int icd_byrows_create(icd_index *idx, int64_t max_nq, icd_byrows **out);
int icd_byrows_destroy(icd_byrows *ws);
/* queries per call, device bytes held (either pointer may be NULL) */
int icd_byrows_stats(icd_byrows *ws, int64_t *out_max_nq, int64_t *out_bytes);
int icd_index_search_by_rows(icd_index *idx, icd_byrows *ws, icd_rowmask *const *masks, const int64_t *ids, int64_t nq, int32_t k,
                             int32_t ids_on_device, int32_t include_self, const float *radius, const float *range_filter,
                             int32_t bounds_on_device, int32_t reweighted, double *out_adj, float *out_raw, int64_t *out_ids,
                             int32_t *out_levels, int32_t out_on_device, void *stream);

/*
 * Rank-of search: where do given rows land in a query's exact ranking, and with what score? The opposite question to every search
 * above - for evaluation (recall@k and MRR need the gold row's rank, also past ICD_MAX_K), for "why not this code?", and for
 * tracking ranks across corpus or model updates. DESIGN.md section 26. Query q carries nt target ids, targets[q][0 .. nt), global
 * ids as searches return them; a slot holding -1 is padding. Per (query, target):
 *   rank      the number of rows of masks[q] that stand STRICTLY AHEAD of the target in the ranking icd_index_search_masked
 *             (reweighted = 0, no band) walks: canonical score descending, the smaller id first among equal scores. If that search
 *             returns id x at position j, the rank of x is j - for every j below its k and for every row behind. (The reweighted
 *             form re-sorts the k hits it has: a position in it depends on k and is no rank.)
 *   raw, adj  the target's canonical score and (double)raw * w[level]: the bits icd_index_search_masked reports for that row.
 *   level     the target's level.
 *   no rank   rank -1, raw and adj NaN, level 0: a padding slot, an id outside [id_base, id_base + n), a row outside masks[q].
 *             A target whose canonical score is NaN has no rank either (no search returns it): rank -1, raw and adj NaN, its level.
 * Per query: selected, the number of rows masks[q] admits (n without a mask). Rows whose score is NaN are never ahead of
 * anything. The same target may appear any number of times in a query; each slot is answered.
 *
 * icd_rankof_create: the workspace of the rank-of calls of `idx` for up to max_nq queries per call: a host caller's queries, the
 * targets, their keys and the outputs. Nothing is allocated in a call. The handle keeps no pointer into its index: it is compared,
 * never followed, and either may be destroyed first. It serves one stream at a time, like the index it belongs to. A view has no
 * rank-of search (ICD_ERR_UNSUPPORTED: mask the parent), nor has the row-sharded path, nor an index of 2^31 rows or more.
 *
 * icd_index_rank_of: two launches on `stream`: rankof_targets_kernel (the targets' canonical scores, keys and levels) and
 * rankof_sweep_kernel (exact_topk_kernel's sweep with the select replaced by a count: one integer add per work-group, query and
 * target - the same bytes on every run). queries: [nq][dim], host or (queries_on_device = 1) device. targets: HOST int64 [nq][nt],
 * 1 <= nt <= ICD_RANKOF_MAX_TARGETS. masks: NULL, or icd_index_search_masked's HOST table of nq entries (NULL entry: every row).
 * Outputs are HOST arrays, [nq][nt] and out_selected [nq]; every one but out_rank may be NULL. The call synchronises `stream` and
 * is not graph-capturable (ICD_ERR_INVALID while capturing). Every check comes before the first device call. ICD_ERR_INVALID: nt
 * out of range, nq above the workspace's max_nq (with masks: above the index's), a workspace or a mask of another index, NULL
 * arrays. ICD_ERR_STATE: a destroyed index, workspace or mask. ICD_ERR_UNSUPPORTED: a view as `idx`. nq = 0 does nothing. A
 * refused call writes no output.
 */
#define ICD_RANKOF_MAX_TARGETS 16
typedef struct icd_rankof icd_rankof;
int icd_rankof_create(icd_index *idx, int64_t max_nq, icd_rankof **out);
int icd_rankof_destroy(icd_rankof *ws);
/* queries per call, device bytes held (either pointer may be NULL) */
int icd_rankof_stats(icd_rankof *ws, int64_t *out_max_nq, int64_t *out_bytes);
int icd_index_rank_of(icd_index *idx, icd_rankof *ws, const float *queries, int64_t nq, int32_t queries_on_device,
                      const int64_t *targets /* host [nq][nt] */, int32_t nt, icd_rowmask *const *masks /* NULL or host [nq] */,
                      int64_t *out_rank, double *out_adj, float *out_raw, int32_t *out_levels, int64_t *out_selected, void *stream);

/*
 * Wide search: the exact ranks first .. first + k - 1 of every query's ranking, for first + k up to ICD_WIDE_MAX_K, in one call -
 * a candidate list for a re-ranker, recall@1000, a deep offset, everything above a similarity floor. DESIGN.md section 27. Every
 * search above stops at ICD_MAX_K hits. The contract, for a query q, its optional row mask masks[q], its optional band
 * (lo[q], hi[q]) = (radius, range_filter), first >= 0 and k >= 1:
 *   1. scores   the canonical ones: the fp32 fmaf chain over d ascending from +0.0f, the bits of icd_index_search in MODE_EXACT.
 *   2. ranking  a row ranks iff the mask admits it, its score is not NaN and lo < score <= hi (plain float compares; an absent
 *               bound makes no test, so without a radius a score of -inf ranks; a NaN device bound empties the band).
 *   3. order    score descending, the smaller row first among equal score bits: the order of the exact searches.
 *   4. raw      (reweighted = 0) ranks first .. first + k - 1 of that ranking, best first: out_raw f32, out_ids i64 (row +
 *               id_base), out_levels i32, [nq][k]; padding -inf, -1, 0 behind. out_count[q] (i32): the real hits of the slice;
 *               out_selected[q] (i64): the rows that rank - the total behind the page.
 *   5. reweighted (reweighted = 1) adj = (double)raw * w[level], ONE stable descending sort of the returned slice (equal adj keeps
 *               raw order): out_adj f64 and raw, id, level with it; padding -inf, -inf, -1, 0.
 *   6. at k <= ICD_MAX_K and first = 0 both forms equal icd_index_search_masked / icd_index_search_range at the same k bit for
 *               bit; at any k they equal the first k entries of the restricted full ranking.
 *   7. the same bytes come back on every run.
 *
 * icd_wide_create: the workspace of the wide searches of `idx` for up to max_nq queries per call and first + k up to max_k: the
 * score block, the candidate block, the threshold records and a host caller's queries, bounds and outputs. The score and
 * candidate blocks hold as many queries as fit a fixed byte budget (256 MiB); a longer batch runs block by block inside the call.
 * Nothing is allocated in a call. The handle keeps no pointer into its index: it is compared, never followed, and either may be
 * destroyed first. It serves one stream at a time, like the index it belongs to. A view has no wide search (ICD_ERR_UNSUPPORTED:
 * mask the parent), nor has the row-sharded path, nor an index of 2^31 rows or more, nor one whose single score run exceeds the
 * budget.
 *
 * icd_index_search_wide: per score block four launches on `stream` (wide_scores_kernel, wide_threshold_kernel,
 * wide_collect_kernel, wide_sort_emit_kernel). queries: [nq][dim], host or (queries_on_device = 1) device. masks: NULL, or
 * icd_index_search_masked's HOST table of nq entries (NULL entry: every row). lo, hi: NULL (no bound) or [nq], host or
 * (bounds_on_device = 1) device; host bounds are checked (no NaN, lo < hi). Outputs: [nq][k] and [nq], host or
 * (outputs_on_device = 1) device; out_adj may be NULL unless reweighted. Device queries, device outputs, device or no bounds and
 * no mask table: the call only enqueues and is graph-capturable. Anything else is staged on the host or synchronises `stream`
 * and is refused while capturing (ICD_ERR_INVALID). Every check comes before the first device call. ICD_ERR_INVALID: k or first
 * out of range, first + k above ICD_WIDE_MAX_K or the workspace's max_k, nq above the workspace's max_nq (with masks: above the
 * index's), a workspace or a mask of another index, NULL arrays. ICD_ERR_STATE: a destroyed index, workspace or mask.
 * ICD_ERR_UNSUPPORTED: a view as `idx`. nq = 0 does nothing. A refused call writes no output.
 */
#define ICD_WIDE_MAX_K 16384
typedef struct icd_wide icd_wide;
int icd_wide_create(icd_index *idx, int64_t max_nq, int32_t max_k, icd_wide **out);
int icd_wide_destroy(icd_wide *ws);
/* queries per call, first + k per call, device bytes held (any pointer may be NULL) */
int icd_wide_stats(icd_wide *ws, int64_t *out_max_nq, int64_t *out_max_k, int64_t *out_bytes);
int icd_index_search_wide(icd_index *idx, icd_wide *ws, icd_rowmask *const *masks /* NULL or host [nq] */, const float *queries,
                          int64_t nq, int32_t k, int32_t first, int32_t queries_on_device, const float *lo /* NULL or [nq] */,
                          const float *hi /* NULL or [nq] */, int32_t bounds_on_device, int32_t reweighted, double *out_adj,
                          float *out_raw, int64_t *out_ids, int32_t *out_levels, int32_t *out_count, int64_t *out_selected,
                          int32_t outputs_on_device, void *stream);

/*
 * Recommend search: rank every row by a request's positive and negative examples - "more like these, less like those" - exact
 * over the whole index, in one call. DESIGN.md section 28. A request has P positive and N negative examples, positives first;
 * list order matters; 1 <= P + N <= ICD_RECOMMEND_MAX_EXAMPLES. An example is a stored row (example_rows[e] in [0, n)) or a
 * caller's vector of dim floats (example_rows[e] = -1: example_vectors[e]). s(e, i) is the canonical score of example vector e
 * and row i: the fp32 fmaf chain over d ascending from +0.0f. The combined score c(i) of a request:
 *   ICD_RECOMMEND_BEST_SCORE      bp = the largest positive-example score, folded in list order from -inf by plain compares
 *                                 (bp = s if s > bp), bn the same over the negatives; c = bp if bp > bn, else -(bn * bn): one
 *                                 fp32 multiply, then the sign flip.
 *   ICD_RECOMMEND_SUM_SCORES      acc = +0.0f; acc = acc + s over the positives in list order, then acc = acc - s over the
 *                                 negatives in list order; plain fp32 adds, nothing reassociated.
 *   ICD_RECOMMEND_AVERAGE_VECTOR  (P >= 1) one target vector t built on the device: per component mp = the positives summed in
 *                                 list order from +0.0f, then ONE correctly rounded fp32 divide by (float)P; mn the same over
 *                                 the negatives; t = mp + (mp - mn) when N > 0, else mp. c(i) = s(t, i).
 * A row ranks iff the request's mask (if any) admits it, it is not one of the request's stored-row examples (a vector example
 * excludes nothing; a bit-identical duplicate of an example row still ranks), no example score of the row is NaN, c is not NaN,
 * and lo < c <= hi (an absent bound makes no test). The ranking is by (c descending, the smaller row first among equal bits).
 * first, k, the raw and the reweighted form, padding, out_count and out_selected are icd_index_search_wide's, with c in place of
 * the raw score. The same bytes come back on every run. One stored positive under BEST_SCORE equals icd_index_search_wide of
 * that row's vector with the row masked out, bit for bit.
 *
 * icd_recommend_create: the workspace for calls of up to max_requests requests holding up to max_examples examples in all
 * (max_requests <= max_examples <= 16 x max_requests) and first + k up to max_k: the example block, its scores, the request
 * block, the candidate block, the request table and a host caller's vectors, bounds and outputs. The blocks hold as many whole
 * requests as fit the wide search's byte budget (256 MiB); a longer batch runs block by block inside the call, a request's
 * examples never straddling two. Nothing is allocated in a call. The handle keeps no pointer into its index and serves one
 * stream at a time. A view has no recommend search (ICD_ERR_UNSUPPORTED: mask the parent), nor has the row-sharded path, nor an
 * index of 2^31 rows or more.
 *
 * icd_index_recommend: per block six launches on `stream` (recommend_examples_kernel, wide_scores_kernel,
 * recommend_combine_kernel, wide_threshold_kernel, wide_collect_kernel, wide_sort_emit_kernel). example_rows [ne],
 * example_off [nr + 1] (from 0) and n_positive [nr] are HOST arrays, checked and staged at call time; example_vectors is NULL (no
 * example is a vector) or [ne][dim], host or (inputs_on_device = 1) device - the entries of stored examples are not read. masks,
 * lo, hi, the outputs and their flags: as in icd_index_search_wide, per request. The request table is staged on the host at call
 * time, so the call is refused while `stream` is capturing (ICD_ERR_INVALID). Every check comes before the first device call; a
 * refused call writes no output. ICD_ERR_INVALID: an unknown strategy, k or first out of range, first + k above the workspace's
 * max_k, nr or the examples above the workspace's, a request of 0 or more than 16 examples, n_positive outside the request,
 * AVERAGE_VECTOR without a positive, a row outside [0, n), a vector example without example_vectors, a workspace or mask of
 * another index, NULL arrays. nr = 0 does nothing.
 *
 * icd_recommend_read_vectors: the first `count` vectors the last block of the last call left in the example block ([count][dim],
 * to the host; synchronises): under AVERAGE_VECTOR the requests' targets, else the examples' vectors. For tests.
 */
#define ICD_RECOMMEND_MAX_EXAMPLES 16
#define ICD_RECOMMEND_AVERAGE_VECTOR 0
#define ICD_RECOMMEND_BEST_SCORE 1
#define ICD_RECOMMEND_SUM_SCORES 2
typedef struct icd_recommend icd_recommend;
int icd_recommend_create(icd_index *idx, int64_t max_requests, int64_t max_examples, int32_t max_k, icd_recommend **out);
int icd_recommend_destroy(icd_recommend *ws);
/* requests per call, examples per call, first + k per call, device bytes held (any pointer may be NULL) */
int icd_recommend_stats(icd_recommend *ws, int64_t *out_max_requests, int64_t *out_max_examples, int64_t *out_max_k, int64_t *out_bytes);
int icd_recommend_read_vectors(icd_recommend *ws, int64_t count, float *out /* host [count][dim] */);
int icd_index_recommend(icd_index *idx, icd_recommend *ws, icd_rowmask *const *masks /* NULL or host [nr] */,
                        const int64_t *example_rows /* host [ne] */, const float *example_vectors /* NULL or [ne][dim] */,
                        const int64_t *example_off /* host [nr + 1] */, const int32_t *n_positive /* host [nr] */, int64_t nr,
                        int32_t strategy, int32_t k, int32_t first, const float *lo /* NULL or [nr] */, const float *hi /* NULL or [nr] */,
                        int32_t bounds_on_device, int32_t reweighted, double *out_adj, float *out_raw, int64_t *out_ids,
                        int32_t *out_levels, int32_t *out_count, int64_t *out_selected, int32_t inputs_on_device,
                        int32_t outputs_on_device, void *stream);

/*
 * Row-sharded search, step 2: merge `G` best-first lists per query (layout [G][nq][k], as produced by
 * all-gathering the outputs of icd_index_search on every shard, together with the level of every
 * hit) into the global top-k, then reweight + stable re-sort as above. Device pointers only;
 * enqueues on `stream`. `device` selects the GPU.
 */
int icd_merge_topk(int32_t device, const float *scores, const int64_t *ids, const int32_t *levels,
                   int32_t G, int64_t nq, int32_t k,
                   double *out_adj, float *out_raw, int64_t *out_ids, int32_t *out_levels, void *stream);

/*
 * Multi-GPU search, one process per GPU. Every rank creates its icd_index first (ROW_SHARD: over its rows, with id_base =
 * index of its first row in the whole corpus; QUERY_SHARD: over the whole corpus), then the group:
 *     rank 0:   icd_group_unique_id(id)   -> hand the ICD_GROUP_ID_BYTES bytes to every rank (file, socket, MPI, ...)
 *     all:      icd_group_create(index, id, rank, world, mode, max_nq, max_k, &group)     (collective: ncclCommInitRank)
 *     all:      icd_group_search(group, queries, nq, k, gather, out_adj, out_raw, out_ids, out_levels, stream)
 * `queries` is the FULL batch [nq][dim] on every rank (device pointer); outputs are device pointers [nq][k] in the order
 * icd_index_search_reweighted gives. ROW_SHARD: identical results on every rank (local raw top-k with global ids and
 * levels -> one grouped ncclAllGather of 16 bytes per hit -> icd_merge_topk). QUERY_SHARD: rank r searches rows
 * [lo_r, hi_r) of the batch (contiguous split, the first nq % world ranks one row more); gather = 1: one grouped
 * ncclAllGather gives every rank all nq rows; gather = 0: no collective at all, rows 0 .. hi_r - lo_r of the outputs hold
 * this rank's slice. Everything is enqueued on `stream`; nothing synchronises. world = 1 needs no id and no RCCL (given
 * an id all the same, a one-rank communicator is created and the collective path runs end to end: tests).
 * librccl.so.1 is opened (dlopen) by the first call that needs it.
 * icd_group_create = icd_group_prepare (everything that can fail on ONE rank alone: argument checks, the device buffers,
 * opening librccl) + icd_group_connect (ncclCommInitRank: COLLECTIVE - a rank that fails before it leaves the others
 * waiting inside it). A host whose ranks can fail locally calls the two itself and lets the ranks agree on the outcome of
 * prepare (any side channel) before any of them connects; rag_project_icd10_amd/sharded.py does exactly that over the
 * torch.distributed group that already exists. Errors of a group call name the rank and the world size.
 */
#define ICD_GROUP_ID_BYTES 128
typedef struct icd_group icd_group;
typedef enum icd_group_mode { ICD_GROUP_ROW_SHARD = 0, ICD_GROUP_QUERY_SHARD = 1 } icd_group_mode;
int icd_group_unique_id(uint8_t *out_id /* [ICD_GROUP_ID_BYTES] */);
int icd_group_create(icd_index *local, const uint8_t *id, int32_t rank, int32_t world, int32_t mode, int32_t max_nq,
                     int32_t max_k, icd_group **out);
/* with_comm: 1 = a communicator will follow (always the case for world > 1; a one-rank group may ask for one: tests) */
int icd_group_prepare(icd_index *local, int32_t with_comm, int32_t rank, int32_t world, int32_t mode, int32_t max_nq,
                      int32_t max_k, icd_group **out);
int icd_group_connect(icd_group *group, const uint8_t *id);
int icd_group_search(icd_group *group, const float *queries, int64_t nq, int32_t k, int32_t gather, double *out_adj,
                     float *out_raw, int64_t *out_ids, int32_t *out_levels, void *stream);
int icd_group_destroy(icd_group *group);   /* (the index stays with the caller) */

/* Level of each hit id (device pointers, [count]); ids < 0 give level 0. Used by the row-sharded
 * path to attach levels to the raw hits before the all-gather. */
int icd_index_lookup_levels(icd_index *idx, const int64_t *ids, int64_t count, int32_t *out_levels,
                            void *stream);

/*
 * Hierarchical rescoring of a batch of hit lists, device side: the string-free arithmetic of
 * HierarchicalSimilarityService.batch_calculate_similarities (services/hierarchical_similarity_service.py:475-518,
 * 243-291, 575) and of the uncertainty boost (services/uncertainty_diagnosis_service.py:190-238) for hits shaped as
 * MilvusService.search returns them, for nq queries at once. IEEE double in the reference's evaluation order:
 * bit-identical to the Python doubles.
 *   adj, ids        [nq][k] outputs of icd_index_search_reweighted (device pointers), k <= 128
 *   row_tags        [n_rows] one byte per corpus row: bits 0-3 index of the code's first letter in the chapter table
 *                   A,B,C,E,I,J,K,N,S (15 = none), bit 7 = the code matches \.9\d*$
 *   q_params        [nq][12] per query, computed from its text on the host: uncertainty weight (0 = none), context
 *                   relevance, exact-match flag, the nine chapter boosts
 *   weights         [7] factor weights hierarchy/entity/coherence/category/context, the coherence value, the level term
 *   outputs         [nq][k] in the final order (enhanced score descending, stable): index of the hit in search order,
 *                   enhanced score, the record's score after the uncertainty boost, the vector_similarity and
 *                   hierarchy_boost factors, the applied uncertainty boost
 */
int icd_hier_rescore(int32_t device, const double *adj, const int64_t *ids, int64_t nq, int32_t k, int64_t id_base,
                     int64_t n_rows, const uint8_t *row_tags, const double *q_params, const double *weights,
                     int32_t *out_order, double *out_enhanced, double *out_score, double *out_vs, double *out_hb,
                     double *out_boost, void *stream);

/* icd_hier_rescore for queries that carry NER entities (the same arguments, checks and outputs). On live-shaped hits every
 * factor the entities feed depends on the query and the first letter of the hit's code only, so it arrives per query:
 *   q_params        [nq][22]: [0..11] as icd_hier_rescore's, the nine chapter boosts with the disease-entity term
 *                   (_calculate_category_semantic_boost, services/hierarchical_similarity_service.py:293-328), [12] the
 *                   entity match score against a live hit's empty title (:341-385), [13..21] the category alignment of each
 *                   chapter of the table (:411-446; 0 for letters outside it)
 * With every entity list empty (entries 12..21 zero) the outputs are byte-identical to icd_hier_rescore's. Bit-identical to
 * batch_calculate_similarities(query, entities, hits) (tests/test_entity_rescoring_gpu.py).
 */
int icd_hier_rescore_entities(int32_t device, const double *adj, const int64_t *ids, int64_t nq, int32_t k, int64_t id_base,
                              int64_t n_rows, const uint8_t *row_tags, const double *q_params, const double *weights,
                              int32_t *out_order, double *out_enhanced, double *out_score, double *out_vs, double *out_hb,
                              double *out_boost, void *stream);

/* SURVEY.md row N3, score statistics. Replaces np.mean / np.std / np.var / max over the candidates' scores in
 * MultiDimensionalConfidenceService._assess_model_uncertainty (services/multidimensional_confidence_service.py:936-963)
 * and ._calculate_prediction_variance (:1087-1099), for nq queries at once, bit-identical to numpy's float64 results.
 *   scores   [nq][k] device doubles (icd_hier_rescore's out_enhanced, or out_adj of a search), k <= 128
 *   order    nullable [nq][k] device: entry j of a query exists iff order[j] >= 0 (icd_hier_rescore's out_order)
 *   use      statistics over the first min(use, existing) entries of every query (the request's top_k)
 *   out      [nq][6] device doubles: mean, std, var, max, model_uncertainty, prediction_variance
 */
int icd_score_stats(int32_t device, const double *scores, const int32_t *order, int64_t nq, int32_t k, int32_t use,
                    double *out, void *stream);

/* The winners of a rescored batch for the host in ONE array (row N2: what MultiDiagnosisService.match_diagnoses_batch turns into
 * Candidate objects - reference services/multi_diagnosis_service.py:147-176 builds them from the rescored hit dicts): for the
 * top kk <= k positions of every query, out[c][q][j] (8-byte slots, c = 0 .. 7; doubles except c = 0, which holds the int64 id's
 * BIT PATTERN: reinterpret that plane as int64) = id, raw score and level-reweighted score of the hit
 * order[q][j] points at, order[q][j] itself, and enhanced / vector-similarity / hierarchy-boost / uncertainty-boost [q][j] of
 * icd_hier_rescore's outputs. One launch and one device-to-host copy instead of three gathers, five slices and eight copies.
 * All pointers device; order int32 [nq][k], ids int64 [nq][k], raw float32 [nq][k], the rest float64 [nq][k]; out [8][nq][kk]. */
int icd_pack_winners(int32_t device, const int32_t *order, const int64_t *ids, const float *raw, const double *adj, const double *enhanced,
                     const double *vs, const double *hb, const double *boost, int64_t nq, int32_t k, int32_t kk, double *out, void *stream);

/* SURVEY.md row N3, semantic coherence. Replaces sklearn cosine_similarity([q], [c])[0][0] in
 * MultiDimensionalConfidenceService._calculate_semantic_factors (:273-280) for nq query vectors at once: rows
 * normalised in double, then their dot product (equal to sklearn's to 1e-14; the summation order differs).
 *   x        [nq][dim] device fp32 query vectors
 *   y        device fp32: [nq][dim] with y_stride = dim, or ONE row shared by every query with y_stride = 0 (the live
 *            /query path embeds the empty string as "the candidate": services/multi_diagnosis_service.py:178-186 hands
 *            the confidence service records without 'preferred_zh')
 *   out      [nq] device doubles
 */
int icd_cosine_rows(int32_t device, const float *x, const float *y, int64_t y_stride, int64_t nq, int32_t dim,
                    double *out, void *stream);

/* The ICD terminology scan of the confidence service. Replaces the loop of
 * MultiDimensionalConfidenceService._get_term_specificity_from_icd (services/multidimensional_confidence_service.py:686-692)
 * that runs when a term is not a name of the cache: for every term t,
 *   out_first[t] = the smallest i with (term in key_i or key_i in term) and len(term) >= 2 and len(key_i) >= 2, else -1,
 * Python str containment on Unicode code points.
 *   key_cp, key_off   device int32: the cache's names in dict order (first occurrence in the CSV), as code points back to back,
 *                     and n_keys + 1 offsets into key_cp (the caller keeps them consistent)
 *   term_cp, term_off device int32: the terms the same way (n_terms + 1 offsets)
 *   out_first         device int32 [n_terms]
 * ICD_ERR_INVALID for NULL pointers, negative counts or decreasing offsets; ICD_ERR_UNSUPPORTED for a term longer than
 * ICD_TERM_MAX_LEN code points (scan that one on the host). n_terms == 0: ICD_OK without a launch. Reads the n_terms + 1
 * term offsets back to the host (a synchronisation of `stream`), then enqueues ONE launch: a work-group per term.
 */
#define ICD_TERM_MAX_LEN 32
int icd_term_first_match(int32_t device, const int32_t *key_cp, const int32_t *key_off, int32_t n_keys, const int32_t *term_cp,
                         const int32_t *term_off, int32_t n_terms, int32_t *out_first, void *stream);

/* The self-attention of the packed BERT encoder (row a3-a5 / N1 of SURVEY.md section 8: the text -> vector forward the
 * reference reaches through sentence-transformers; rag_project_icd10_amd/services/embedding_service.py _PackedBert runs
 * every Linear of the encoder over packed tokens and calls this for the attention): softmax(Q K^T / sqrt(64)) V per
 * sequence and head, fp32.
 *   qkv      [T][ld] device fp32: Q | K | V of a token side by side (ld >= 3 * heads * 64, a multiple of 4)
 *   starts   [nseq + 1] device int32: first packed row of every sequence (sequence s is rows starts[s] .. starts[s + 1])
 *   max_len  the longest sequence (host-known): 1 .. 512 (up to 64 tokens one pass; longer ones in chunks of 64 keys)
 *   out      [T][out_ld] device fp32: heads side by side
 * Enqueues one launch on `stream`. */
int icd_packed_attention(int32_t device, const float *qkv, int64_t ld, const int32_t *starts, int32_t nseq, int32_t heads,
                         int32_t head_dim, int32_t max_len, float *out, int64_t out_ld, void *stream);

/* The A operand of a split-bf16 GEMM, in one pass (the Linear layers inside SentenceTransformer.encode, reference
 * services/embedding_service.py:97-102, run as x_hi W_hi + x_hi W_lo + x_lo W_hi + b on the bf16 MFMA with fp32 accumulation
 * and output): x fp32 [rows][cols] (row stride ld elements; device, 16-byte aligned), optionally through erf-GELU (act = 1:
 * BertIntermediate), -> out bf16 [rows][3 cols + 64] = [hi | hi | lo | 1 1 0 ... 0], hi = bf16(x) rounded to nearest
 * even, lo = bf16(x - hi). The weight operand is [W_hi^T; W_lo^T; W_hi^T; b_hi; b_lo; 0 x 62] (3 cols + 64 rows: K stays a
 * multiple of the GEMM's 64-deep step). cols must be a multiple of 8 and at least 64. Enqueued on `stream`. */
int icd_split_bf16x3(int32_t device, const float *x, int64_t rows, int32_t cols, int64_t ld, int32_t act, void *out, void *stream);

/* (last_fallback: every search copies its counters to pinned host memory behind itself, on its stream; this call waits
 *  for the last search of this handle - an event on that stream - and for nothing else on the device) */
int icd_index_stats(icd_index *idx, icd_stats *out);

/* Diagnostic / test hook: the MEASURED terms of finalize's certificate, in the fp16 image's scaled
 * units 2^cexp (queries: each in its own scale): *cmax = the largest norm of the scaled corpus rows (of the centred rows
 * when the image is centred), *dcmax = the largest | scaled row - its fp16 image |, both rounded up at index creation;
 * qnorm / qres (host memory, [count], either may be NULL) = the same two norms of the first `count` queries of the last
 * AUTO search of this handle that ran the coarse pass (count <= that search's batch). Waits for the device. An index
 * without an fp16 image: ICD_ERR_INVALID. */
int icd_index_cert_terms(icd_index *idx, float *cmax, float *dcmax, int32_t *cexp, float *qnorm, float *qres, int64_t count);

/* Tuning knob / test hook (0 = automatic): aim for about `chunks` candidate lists per query in the coarse pass
 * (the automatic choice gives every CU the same number of 128 x 128 tiles). */
int icd_index_set_chunks(icd_index *idx, int32_t chunks);

/* Test / A-B switch (default 1): 0 turns the second coarse pass (and the adaptive list count that follows from its counters)
 * off - queries the first pass cannot certify then go straight to the exact re-search, as before round 3; 2 keeps the
 * second pass but never switches to the wide partition (every large batch runs narrow plan + second pass). */
int icd_index_set_second_pass(icd_index *idx, int32_t enabled);

/* A/B and test options of ONE index (round 6: these were process-wide icd_debug_set_* switches; a serving process with two
 * indexes must not have one caller's test hook change the other's behaviour). Every one is a performance decision only:
 * results are identical whatever it is set to. Defaults in brackets. Calls on one handle are serialised with its searches.
 *   ICD_OPT_FAMILY_ORDER [1]  0 keeps the wide-window finalize of a family-shaped corpus (icd_stats.wide_mode) in batch order
 *                             instead of visiting the queries family by family, XCD by XCD (finalize.hpp, order_*_kernel).
 *   ICD_OPT_STREAM_ONE   [1]  0 sends calls of one or two queries (the reference's own call shape,
 *                             services/milvus_service.py:280-285) through the general streaming path - memset, stream_topk,
 *                             reduce_lists, finalize: four operations - instead of the single-launch kernel that folds all of it.
 *   ICD_OPT_HOST_ONE     [3]  how a HOST caller's ONE query reaches and leaves the single-launch kernel. Bit 1: the vector
 *                             travels in the kernel's arguments (no host-to-device copy command in front of the launch). Bit 2:
 *                             the call returns when the kernel's last work-group has stored the call's sequence number behind
 *                             the outputs in the index's mapped host block (polled for a bounded time, then the stream
 *                             synchronisation as before). 0 = the copy + hipStreamSynchronize form.
 *   ICD_OPT_PACING_SHIFT [3], ICD_OPT_PACING_LEAD [2]  the coarse sweep over an fp16 image that does not stay in the Infinity
 *                             Cache (a row shard) paces the work-groups that sweep the same corpus tiles: epochs of 2^shift
 *                             tiles, a class stays within `lead` epochs, so that a tile is fetched once per XCD
 *                             (csrc/coarse_flat_kernel.hpp). shift < 0 turns pacing off.
 *   ICD_OPT_EXACT_NARROW [1]  0 makes ICD_MODE_EXACT at k > 32 keep lists of KP >= k (64- / 128-entry candidate buffers, one
 *                             work-group per CU) instead of certified lists of 32 over row-strided chunks with a re-search of
 *                             the queries the certificate cannot clear (k range: /query searches top_k * 2 with top_k <= 50,
 *                             models/icd_models.py:138, services/multi_diagnosis_service.py:153).
 *   ICD_OPT_WIDE_FROM   [48]  searches with k above this keep 24 candidates per coarse list (about k / 6 lists per query) instead of
 *                             16 (about k / 4 lists): a slower sweep, but no query whose top-k crowd one list is left for the
 *                             exact re-search (profiles/r06_k100_lists.log). >= ICD_MAX_K: lists of 16 at every k.
 * No reference counterpart (the reference delegates the search to Milvus Lite). */
enum { ICD_OPT_FAMILY_ORDER = 1, ICD_OPT_STREAM_ONE = 2, ICD_OPT_HOST_ONE = 3, ICD_OPT_PACING_SHIFT = 4, ICD_OPT_PACING_LEAD = 5, ICD_OPT_EXACT_NARROW = 6,
       ICD_OPT_WIDE_FROM = 7 };
int icd_index_set_option(icd_index *idx, int32_t option, int32_t value);

/* Test entry: the unpack step of a query-sharded icd_group_search (one kernel: the all-gathered PADDED slices -> the
 * contiguous [nq][k] outputs) on a caller-made receive buffer, so that its index arithmetic can be checked for any world
 * size on ONE GPU. `gathered` (device) is laid out as the group's receive buffer: with width = ceil(nq / world) and
 * per = width * k, four arrays back to back - adj f64 [world][per] | ids i64 [world][per] | raw f32 [world][per] |
 * levels i32 [world][per]; rank r's slice holds queries [lo_r, hi_r) (contiguous split, the first nq % world ranks one
 * more) in its first hi_r - lo_r rows. Outputs: device pointers, [nq][k]. No reference counterpart (single process). */
int icd_unpack_query_slices(int32_t device, const void *gathered, int32_t world, int64_t nq, int32_t k, double *out_adj,
                                  float *out_raw, int64_t *out_ids, int32_t *out_levels, void *stream);

/* ---- the sentence encoder for SMALL inputs ------------------------------------------------
 * The reference embeds ONE string per call - EmbeddingService.encode_query / encode_single -> SentenceTransformer.encode
 * (services/embedding_service.py:97-102, 117-120) - and a /query request a handful (services/multi_diagnosis_service.py:97,
 * 137). At 10-100 tokens the framework's forward is ~220 kernels of ~5 us (1.1 ms replayed from a graph); this is the same
 * BERT forward (post-LN encoder, absolute positions, erf-GELU, 64-wide heads, fp32) as 7 hand-written launches per layer
 * (csrc/encoder_small.hpp), replayed as ONE graph per token bucket. All pointers are device fp32 (e.g. the torch module's
 * parameters). icd_encoder_create COPIES the four Linear weights of every layer (into the order its GEMMs read them: the
 * caller's may be freed or changed afterwards without effect) and BORROWS the embeddings, biases and LayerNorm parameters:
 * the caller keeps those alive and unchanged while the handle lives. */
typedef struct icd_encoder icd_encoder;
typedef struct {
    int32_t layers, hidden, heads, inter;   /* hidden = heads * 64 = 768 or 1024; inter a multiple of hidden, at most 4 hidden */
    int32_t vocab, max_pos;                 /* rows of word_emb / pos_emb */
    int32_t pos_offset;                     /* position of a sequence's first token: 0 (BERT), padding_idx + 1 (RoBERTa / XLM-R) */
    float ln_eps;
    const float *word_emb, *pos_emb, *type_emb0, *emb_ln_g, *emb_ln_b;
    /* [layers] host arrays of device pointers; Linear weights as torch keeps them, [out][in] row-major */
    const float *const *w_qkv;  const float *const *b_qkv;    /* [3 hidden][hidden]: query | key | value rows stacked */
    const float *const *w_ao;   const float *const *b_ao;     /* attention output dense [hidden][hidden] */
    const float *const *ln1_g;  const float *const *ln1_b;
    const float *const *w_up;   const float *const *b_up;     /* intermediate dense [inter][hidden] */
    const float *const *w_down; const float *const *b_down;   /* output dense [hidden][inter] */
    const float *const *ln2_g;  const float *const *ln2_b;
    int32_t arithmetic;                     /* of the four Linear layers' GEMMs, in BOTH forms (one call / icd_encoder_encode_many) alike:
                                               ICD_ENCODER_ARITH_FP32 (0) fp32-input MFMA, exact products; ICD_ENCODER_ARITH_BF16X3 (1) the
                                               split-bf16 form - x = x_hi + x_lo, w = w_hi + w_lo in bf16, three bf16 MFMAs per 32 k-values
                                               (hi hi, hi lo, lo hi) into fp32: 1 / 5 of the matrix time, ~1e-6 off the fp32 forward */
} icd_encoder_desc;
enum { ICD_ENCODER_ARITH_FP32 = 0, ICD_ENCODER_ARITH_BF16X3 = 1 };
#define ICD_ENCODER_MAX_TOKENS 512   /* packed tokens per call: any ONE sequence a BERT-style encoder takes fits */
#define ICD_ENCODER_MAX_SEQS 64      /* sequences per call */
int icd_encoder_create(int32_t device, const icd_encoder_desc *desc, icd_encoder **out);
/* ids: HOST int32, the sequences' token ids back to back (special tokens included); lengths: HOST int32 [nseq], each >= 1,
 * their sum <= ICD_ENCODER_MAX_TOKENS. pooling 0 = mean over a sequence's tokens, 1 = its first token; normalize 1 =
 * torch.nn.functional.normalize(p = 2). out: [nseq][hidden] fp32, host (the call returns when it is filled) or device
 * (out_on_device = 1: enqueued on `stream`, no synchronisation). hidden_out: NULL, or a DEVICE buffer [sum lengths][hidden]
 * that receives the last hidden state of every token (token classification heads). Calls on one handle are serialised; the
 * handle's activations belong to the handle, not to a stream: a call on ANOTHER stream than the one before waits on the device
 * (an event, no host block) until that call's work has left them - icd_encoder_encode and icd_encoder_encode_many alike. */
int icd_encoder_encode(icd_encoder *e, const int32_t *ids, const int32_t *lengths, int32_t nseq, int32_t pooling, int32_t normalize,
                       float *out, int32_t out_on_device, float *hidden_out, void *stream);
/* ANY number of sequences through the same kernels, in calls of at most ICD_ENCODER_MAX_TOKENS tokens / ICD_ENCODER_MAX_SEQS
 * sequences cut greedily in the given order. The arithmetic of a sequence does not depend on what else shares its call
 * (every reduction runs over the sequence's own tokens in an order fixed by the kernels), so out[i] equals BIT FOR BIT what
 * icd_encoder_encode returns for sequence i alone: the reference embeds corpus rows and queries through the same one-string
 * call (tools/build_database.py:217-222, services/embedding_service.py:117-120) - identical text, identical vector - and this
 * is how a corpus build or a batch of queries keeps that property. lengths[i] in 1 .. min(ICD_ENCODER_MAX_TOKENS, max_pos -
 * pos_offset). out: [nseq][hidden] fp32, device (enqueued on `stream`, no synchronisation) or host (returns when filled). */
int icd_encoder_encode_many(icd_encoder *e, const int32_t *ids, const int32_t *lengths, int64_t nseq, int32_t pooling, int32_t normalize,
                            float *out, int32_t out_on_device, void *stream);
int icd_encoder_destroy(icd_encoder *e);

/* Diagnostic builds only (make ABLATE=1, env ICD_FLAT_VAR with bit 1024): per-wave cycle sums of the coarse kernel,
 * [work-group][wave][8] = {LDS-DMA wait, barrier, stage body, fused select, tiles, ...}. */
int icd_index_debug_counters(icd_index *idx, unsigned long long *out, int32_t count);

/* enabled: 0 off; 1 events around every kernel of every search; N > 1 of every N-th search (an event between two kernels
 * keeps the second from starting under the first one's tail: a timed region samples instead of paying that on every step) */
int icd_index_set_profiling(icd_index *idx, int32_t enabled);
/* Synchronises the events of the most recent search and fills `out`. */
int icd_index_last_profile(icd_index *idx, icd_profile *out);
/* Mean per-kernel times over the profiled searches since the previous summary (at most the last 128),
 * and how many were averaged; resets the window. The events are recorded on the search stream, so this
 * measures the kernels inside a timed region without a synchronisation per search. */
int icd_index_profile_summary(icd_index *idx, icd_profile *out_mean, int32_t *out_count);

#ifdef __cplusplus
}
#endif
#endif /* ICD_SEARCH_H */
