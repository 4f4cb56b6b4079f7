// icd_search.hip — host side of libicdsearch.so (C ABI declared in include/icd_search.h).
// gfx950 (MI355X) only. No allocation and no synchronisation inside a search whose inputs and
// outputs are device buffers.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/icd_search.h"
#include "coarse_flat_kernel.hpp"
#include "attention_kernel.hpp"
#include "exact_kernel.hpp"
#include "finalize.hpp"
#include "group_topk.hpp"
#include "group_aggregate_kernel.hpp"
#include "maxsim_kernel.hpp"
#include "hybrid_fuse.hpp"
#include "sparse_kernel.hpp"
#include "text_match_kernel.hpp"
#include "filter_mask_kernel.hpp"
#include "mask_select_kernel.hpp"
#include "facet_count_kernel.hpp"
#include "mmr_select_kernel.hpp"
#include "byrows_kernel.hpp"
#include "rankof_kernel.hpp"
#include "wide_select_kernel.hpp"
#include "recommend_kernel.hpp"
#include "hier_kernel.hpp"
#include "stats_kernel.hpp"
#include "stream_kernel.hpp"
#include "term_lookup.hpp"
#include "search_policy.hpp"   // (host only: the adaptive rules of the AUTO path, PASS2_SKIP ... WIDE_REPROBE)

using namespace icd;

namespace {
thread_local std::string g_err = "";
}  // namespace

// The ONE error hook: the text icd_last_error returns, thread-local. icd_group.cpp reports through it too (hence the linkage).
extern "C" __attribute__((visibility("hidden"))) int icd_internal_fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

namespace {
constexpr auto &fail = icd_internal_fail;
}  // namespace

// Query-sharded gather (icd_group.cpp): the all-gathered send buffers hold, per rank r, one PADDED slice of `width` queries
// in four arrays (adj f64 | ids i64 | raw f32 | levels i32, each [world][width * k]); rank r's valid part is the first
// (hi_r - lo_r) queries. ONE launch scatters every rank's valid hits to the contiguous [nq][k] outputs (it replaces four
// hipMemcpyAsync per rank: 32 copies at 8 ranks). shard_bounds' arithmetic restated: base = nq / world, rem = nq % world.
__global__ void unpack_query_slices_kernel(const double *r_adj, const long long *r_ids, const float *r_raw, const int *r_lv,
                                           int world, long long nq, int k, long long width, double *out_adj, float *out_raw,
                                           long long *out_ids, int *out_lv) {
    const long long total = nq * (long long)k;
    const long long base = nq / world, rem = nq % world;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        const long long q = e / k;
        const int j = (int)(e - q * k);
        // rank of query q: the first `rem` ranks own base + 1 queries each
        const long long split = rem * (base + 1);
        const int r = q < split ? (int)(q / (base + 1)) : (int)(rem + (q - split) / (base > 0 ? base : 1));
        const long long lo = (long long)r * base + (r < rem ? r : rem);
        const long long src = (long long)r * width * k + (q - lo) * k + j;
        out_adj[e] = r_adj[src]; out_ids[e] = r_ids[src]; out_raw[e] = r_raw[src]; out_lv[e] = r_lv[src];
    }
}
extern "C" __attribute__((visibility("hidden"))) int icd_internal_unpack_query_slices(const void *r_adj, const void *r_ids, const void *r_raw,
        const void *r_lv, int world, long long nq, int k, long long width, void *out_adj, void *out_raw, void *out_ids, void *out_lv, void *stream) {
    const long long total = nq * (long long)k;
    if (total <= 0) return 0;
    const int blocks = (int)std::min<long long>((total + 255) / 256, 2048);
    hipLaunchKernelGGL(unpack_query_slices_kernel, dim3(blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       static_cast<const double *>(r_adj), static_cast<const long long *>(r_ids), static_cast<const float *>(r_raw),
                       static_cast<const int *>(r_lv), world, nq, k, width, static_cast<double *>(out_adj), static_cast<float *>(out_raw),
                       static_cast<long long *>(out_ids), static_cast<int *>(out_lv));
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

namespace {

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(e_ == hipErrorOutOfMemory ? ICD_ERR_NOMEM : ICD_ERR_HIP, "%s: %s (%s:%d)", \
                        #expr, hipGetErrorString(e_), __FILE__, __LINE__);                         \
    } while (0)

// ... with something to unwind first: a half-built index or owned handle (the ONE allocate-or-free-everything form)
#define HIP_TRY_OR(undo, expr)                                                                                             \
    do {                                                                                                                   \
        hipError_t e_ = (expr);                                                                                            \
        if (e_ != hipSuccess) {                                                                                            \
            undo;                                                                                                          \
            return fail(e_ == hipErrorOutOfMemory ? ICD_ERR_NOMEM : ICD_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
        }                                                                                                                  \
    } while (0)

constexpr size_t PACE_WORDS = (size_t)1 << 18;   // arrival counters of a paced coarse sweep: classes x epochs (1 MB)
constexpr size_t COARSE_CACHED_IMAGE_BYTES = (size_t)96 << 20;   // fp16 images up to this size take CF_CACHED_VAR (both corpus copies then fit the 256 MiB Infinity Cache)
constexpr int FAST_MAX_K = 100;      // the rescoring window holds up to 256 candidates (four per lane): k + the rows inside 2 eps of the k-th
// (COARSE_MAX_P, PASS2_CHUNKS, PASS2_MAX_P, PASS2_BELOW: the list planner's, flat_partition.hpp; PASS2_SKIP, SPARSE_DISARM_AFTER,
//  PASS2_DISARM_AFTER, WIDE_MIN_NQ, WIDE_REPROBE: the adaptive rules', search_policy.hpp)
static_assert(FLAT_TILE_ROWS == CO_BN, "flat_partition.hpp plans tiles of CO_BN rows");
constexpr int NUM_EV = 6;
constexpr int EV_RING = 128;         // profiled searches kept for icd_index_profile_summary

// hipFuncAttributeMaxDynamicSharedMemorySize is a property of (kernel, device): every kernel keeps, per device, the
// largest size it has configured and raises it when a launch needs more (two indexes of different dim share kernels).
constexpr int MAX_DEVICES = 64;
template <auto KERN>
hipError_t ensure_dynamic_lds(int device, size_t bytes) {
    static int configured[MAX_DEVICES] = {};   // (guarded by the caller's one-stream-per-handle contract; worst case a repeated call)
    if (device < 0 || device >= MAX_DEVICES) return hipErrorInvalidDevice;
    if ((size_t)configured[device] >= bytes) return hipSuccess;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) configured[device] = (int)bytes;
    return e;
}
// ONE launch of a kernel with dynamic LDS: its limit raised to `lds_limit` when this device has not seen as much (some launchers
// ask for more than the launch's own `lds`), the launch, the launch's error.
template <auto KERN, typename... Args>
hipError_t launch_lds(int device, size_t lds_limit, dim3 grid, dim3 block, size_t lds, hipStream_t s, const Args &...args) {
    const hipError_t e = ensure_dynamic_lds<KERN>(device, lds_limit);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(KERN, grid, block, lds, s, args...);
    return hipGetLastError();
}

template <typename T>
hipError_t dmalloc(T **p, size_t count) {
    return hipMalloc(reinterpret_cast<void **>(p), std::max<size_t>(count, 1) * sizeof(T));
}

}  // namespace

struct icd_index {
    uint32_t magic = 0x1CD10A3Du;
    int device = 0;
    // A/B and test options, PER HANDLE (icd_index_create flags, icd_index_set_option): performance decisions only, results are
    // identical whatever they are set to. Read and written under `mu`.
    bool opt_permute = true;        // ICD_CREATE_ROW_ORDER clears it: row order of the fp16 corpus copy
    bool opt_probe = true;          // ICD_CREATE_NO_PROBE: the corpus-shape probe of icd_index_create
    bool opt_center = true;         // ICD_CREATE_NO_CENTER: the fp16 image is centred when the rows share a large common component
    int opt_pace_shift = 3, opt_pace_lead = 2;   // ICD_OPT_PACING_*: epochs of 2^shift tiles, classes kept within `lead` epochs; shift < 0: no pacing
    bool opt_exact_narrow = true;   // ICD_OPT_EXACT_NARROW: EXACT mode at k > 32 runs certified lists of 32 over row-strided chunks
    int opt_host_one = 3;           // ICD_OPT_HOST_ONE: a host caller's ONE query 1 = travels in the kernel arguments, 2 = completion by a polled word
    bool opt_stream_one = true;     // ICD_OPT_STREAM_ONE: one or two queries per call take the single-launch streaming kernel
    bool opt_family_order = true;   // ICD_OPT_FAMILY_ORDER: the wide-window finalize visits the queries in family order
    int opt_wide_from = 48;         // ICD_OPT_WIDE_FROM: k above this keeps 24 candidates per coarse list instead of 16 (>= ICD_MAX_K: never). 64 until round 5.
                                    // Lists of 16 leave 1-5 of 10 000 queries to the exact re-search at k = 40 ... 64: 0.18-0.20 ms per batch while the streaming
                                    // re-search started its lists at -inf, 0.06-0.07 since it takes finalize's threshold (round 6). With that the two list
                                    // widths meet at k = 50 ... 64 and 16 wins below (profiles/r06_k100_lists.log)
    int64_t n = 0, id_base = 0;
    long long *row_map = nullptr;   // a view (icd_index_create_view): [n] the parent's global id of every row (finalize.hpp FinArgs::row_map)
    int n_pad = 0;
    int dim = 0;
    int max_nq = 0, max_nq_pad = 0, max_k = 0;
    bool fast = false;
    float rmax = 0.f;        // largest row norm (unscaled; reported by icd_index_stats)
    float rmax_scaled = 0.f; // largest norm of the scaled fp16 rows
    float dcmax_scaled = 0.f;   // largest | scaled row - its fp16 image | (the certificate's measured rounding error, cert_bound.hpp)
    int cexp = 0;            // fp16 corpus = fp32 corpus * 2^cexp
    float *cmean = nullptr;  // [dim] column mean subtracted from the fp16 image (nullptr: not centred; coarse_common.hpp)
    float rmax_unc_scaled = 0.f;   // centred image: largest norm of the UNcentred rows, in the image's scale
    float mean_share = 0.f;  // |mu|^2 / mean |row|^2 (the mean pairwise cosine of unit rows): reported by icd_index_stats
    int num_cu = 256;
    // corpus
    float *corpus = nullptr;
    _Float16 *c16 = nullptr;
    int *levels = nullptr;
    // workspace
    float *qdev = nullptr;  // staging for host queries
    _Float16 *q16 = nullptr;
    float *qnorm = nullptr;
    float *qres = nullptr;   // [query] | scaled query - its fp16 image |
    int *qexp = nullptr;
    unsigned char *qbad = nullptr;
    float *thr0 = nullptr;   // [query] threshold an uncertified query hands to its exact re-search (finalize.hpp)
    unsigned int *shared_thr = nullptr;   // [max_nq_pad] coarse pass: per-query threshold shared by its lists
    long long perm_mul = 0; int perm_mod = 0;   // row order of the fp16 corpus: position p holds row (p * perm_mul) mod perm_mod
    float *partc_s = nullptr; int *partc_r = nullptr; float *partc_b = nullptr; size_t partc_cap = 0;   // coarse lists + bounds
    float *part2_s = nullptr; int *part2_r = nullptr; float *part2_b = nullptr; size_t part2_cap = 0;   // lists of the second coarse pass
    float *partx_s = nullptr; int *partx_r = nullptr; size_t partx_cap = 0;
    float *lists_s = nullptr; int *lists_r = nullptr; size_t lists_cap = 0;   // streaming kernel: [slot][4 nwg][KP]
    int *nflag = nullptr; int *flagged = nullptr;   // [8]: fallback counters [0..3], [4] = consecutive fast-path searches whose exact re-search had nothing to do (kept by the device); lists [3][max_nq_pad] and lists [3][max_nq_pad]: after the first finalize, after its wide-window retry, after the second coarse pass
    int fallback_word = 0;                           // which counter / list the last search's exact re-search read
    int *h_nflag = nullptr;                          // pinned (mapped) host copy of nflag[4], written by the last kernel of every search
    int *h_nflag_dev = nullptr;                      // its device-side address
    hipEvent_t ev_nflag = nullptr;                   // recorded behind that copy: icd_index_stats waits for it and nothing else
    unsigned int *scratch_u32 = nullptr;  // [0]=rmax bits, [1]=any_bad, [2]=largest component, [3]=largest uncentred norm, [4]=largest residual norm
    int *order = nullptr, *order_key = nullptr; unsigned int *order_hist = nullptr;   // wide-window finalize in family order (finalize.hpp, order_*_kernel)
    // output staging (used when the caller's buffers are host memory)
    float *o_scores = nullptr; long long *o_ids = nullptr;
    double *o_adj = nullptr; float *o_adj_raw = nullptr; long long *o_adj_ids = nullptr; int *o_adj_lv = nullptr;
    // small host calls (the reference's one-query-per-call shape): ONE pinned, mapped block - the query goes through its first
    // part (CPU copy + a true asynchronous H2D copy; a pageable source makes hipMemcpyAsync stage and wait), the kernels write
    // the results straight into its second part (zero-copy stores over PCIe) and the host copies them out after the stream
    // synchronisation: no D2H memcpy call at all (six of them to pageable memory cost ~60 us of a 113-us call)
    char *h_pin = nullptr, *h_pin_dev = nullptr;
    // ... and for ONE query per call (services/milvus_service.py:280-285) two commands less: the vector travels IN the kernel
    // arguments of the single-launch kernel (no H2D copy in front of it: host_q is set for the duration of that call), and the
    // kernel's last work-group stores a sequence number behind its outputs (the block's last 64 bytes) that the host polls
    // instead of waiting for the stream's completion signal (done_seq counts the calls that asked for it)
    const float *host_q = nullptr;
    bool host_one_call = false;    // the current call is ONE query from host memory with host outputs in the mapped block: it may poll
    unsigned long long done_seq = 0;
    bool done_armed = false;       // the current call's launch carries the word's address
    size_t bytes_ws = 0;
    // knobs / counters
    int chunks_override = 0;
    SearchPolicy pol;              // what the AUTO path remembers between searches: wide mode of large batches, the second pass and the streaming pair armed or not (search_policy.hpp)
    std::mutex mu;   // host-side state of the handle (plans, adaptive counters, profiling ring): calls on one handle are serialised; the DEVICE workspace still belongs to one stream at a time (header)
    int probe_flagged = -1, probe_left = -1;   // the corpus-shape probe of icd_index_create: queries its first finalize flagged / its second pass left (-1: not run)
    bool pass2_enabled = true;     // test hook (icd_index_set_second_pass)
    bool adapt_enabled = true;     // ... 2 = second pass without the adaptive list count
    bool profiling = false;
    int prof_every = 1;            // events on every prof_every-th search (a recorded event keeps the next kernel from
    long prof_tick = 0;            // overlapping the previous one's tail: sampling keeps that cost out of a timed region)
    bool prof_now = false;
    bool capturing = false;        // the current search is being captured into a HIP graph (run_search): no event queries, no host-side adaptation
    hipEvent_t evring[EV_RING][NUM_EV + 1] = {};
    bool evring_valid[EV_RING][NUM_EV + 1] = {};
    long prof_count = 0;           // profiled searches since the last summary
    hipEvent_t *ev = evring[0];    // event set of the current / most recent search
    bool *ev_valid = evring_valid[0];
    int64_t last_nq = 0;
    int last_chunks = 0, last_mode = 0;
    int last_p2 = 0, last_p2_word = 0;   // lists per query of the last search's second pass (0: none) and the counter that fed it
    // range search (icd_index_search_range): the packed bands of a call's queries. Device bounds are packed by band_pack_kernel;
    // host bounds on the host (a view's row map is kept there too) into the pinned block, copied only where a path wants them
    // in device memory - the single-launch kernel takes up to four in its arguments. Allocated at create, like everything else.
    BandQ *band_dev = nullptr, *h_band = nullptr;   // [max_nq] each
    std::vector<long long> h_row_map;   // a view: the host's copy of row_map (the cursor's id -> first local row behind it)
    int band_pending = 0;               // host-packed bands of the current call not yet copied to band_dev
    // masked search (icd_index_search_masked): [query] -> bitset, filled on the host into the pinned table and copied to the
    // device one per call; mask_ones = the all-ones bitset (rows [0, n)) an unmasked query of a masked batch reads
    const uint32_t **mask_dev = nullptr, **h_mask = nullptr;   // [max_nq] each
    uint32_t *mask_ones = nullptr;
    hipEvent_t ev_mask = nullptr;       // recorded behind the table's copy: the next masked call waits for it before it refills the
    bool mask_copy_pending = false;     // pinned table - whatever became of the call in between (an error return included)
    // ordered select over row masks (icd_rowmask_select): the per-(query, segment) counts of a call, its
    // offsets (pinned h_sel_off -> sel_off, behind the mask table's event), and the staging of a call with host outputs
    int *sel_counts = nullptr;          // [max_nq][ms_segments(n)]
    long long *sel_off = nullptr, *h_sel_off = nullptr;   // [max_nq] each
    long long *sel_ids = nullptr, *sel_total = nullptr;   // [sel_out_cap], [max_nq]
    int *sel_taken = nullptr;           // [max_nq]
    size_t sel_out_cap = 0;             // id slots of a call with host outputs (ms_host_slots)
    unsigned long long uid = 0;         // identity of this index among all ever created in the process (a row mask remembers it)
    unsigned long long *dbg = nullptr;  // diagnostic cycle counters [8192][4][4]
    unsigned int *pace = nullptr;       // [PACE_WORDS] arrival counters of the paced coarse sweep (coarse_flat_kernel.hpp, 67108864)
};

namespace {

bool valid(icd_index *idx) { return idx && idx->magic == 0x1CD10A3Du; }

}  // namespace

// (icd_group.cpp: a view cannot be a row shard)
extern "C" __attribute__((visibility("hidden"))) int icd_internal_is_view(const icd_index *idx) {
    return idx && idx->row_map ? 1 : 0;
}

namespace {

void free_all(icd_index *x) {
    if (!x) return;
    hipFree(x->corpus); hipFree(x->c16); hipFree(x->levels); hipFree(x->qdev); hipFree(x->q16);
    hipFree(x->qnorm); hipFree(x->qres); hipFree(x->qexp); hipFree(x->qbad); hipFree(x->thr0); hipFree(x->shared_thr); hipFree(x->partc_s); hipFree(x->partc_r); hipFree(x->partc_b); hipFree(x->partx_s);
    hipFree(x->part2_s); hipFree(x->part2_r); hipFree(x->part2_b);
    hipFree(x->partx_r); hipFree(x->lists_s); hipFree(x->lists_r); hipFree(x->nflag); hipFree(x->flagged); hipFree(x->scratch_u32);
    hipFree(x->order); hipFree(x->order_key); hipFree(x->order_hist); hipFree(x->cmean);
    hipFree(x->o_scores); hipFree(x->o_ids); hipFree(x->o_adj); hipFree(x->o_adj_raw);
    hipFree(x->o_adj_ids); hipFree(x->o_adj_lv);
    hipFree(x->dbg);
    hipFree(x->pace);
    hipFree(x->row_map);
    hipFree(x->band_dev);
    if (x->h_band) hipHostFree(x->h_band);
    hipFree(x->mask_dev); hipFree(x->mask_ones);
    if (x->h_mask) hipHostFree(x->h_mask);
    hipFree(x->sel_counts); hipFree(x->sel_off); hipFree(x->sel_ids); hipFree(x->sel_total); hipFree(x->sel_taken);
    if (x->h_sel_off) hipHostFree(x->h_sel_off);
    if (x->ev_mask) hipEventDestroy(x->ev_mask);
    if (x->h_nflag) hipHostFree(x->h_nflag);
    if (x->h_pin) hipHostFree(x->h_pin);
    if (x->ev_nflag) hipEventDestroy(x->ev_nflag);
    for (int r = 0; r < EV_RING; ++r)
        for (int i = 0; i <= NUM_EV; ++i)
            if (x->evring[r][i]) hipEventDestroy(x->evring[r][i]);
    x->magic = 0;
    delete x;
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------

// candidates per exact list: the smallest of 16 / 32 / 64 / 128 that holds k. (32 is round 4's: the serving path searches
// top_k * 2 = 20, and finalize merges at most 512 candidates per query - 8 lists of 64 gave a few hundred flagged queries 80
// two-wave work-groups, 16 lists of 32 give them 160.)
int exact_kp_for(int k) { return k <= 16 ? 16 : (k <= 32 ? 32 : (k <= 64 ? 64 : 128)); }

// the chunk count in [c_lo, c_hi] whose last round of `slots` work-groups is fullest (mtiles x c work-groups in all); the
// first count whose last round is at least `enough` full is taken at once
int fullest_round(int mtiles, int slots, int c_lo, int c_hi, double enough) {
    double best = 0;
    int bestc = c_lo;
    for (int c = c_lo; c <= c_hi; ++c) {
        const long items = (long)mtiles * c;
        const double util = (double)items / (double)(((items + slots - 1) / slots) * slots);
        if (util > best + 1e-9) { best = util; bestc = c; }
        if (util >= enough) { bestc = c; break; }
    }
    return bestc;
}

// chunk count heuristic: enough work-groups to fill the chip, few enough lists to merge. `slots` = the work-groups the
// chip holds at once: ONE per CU for every instantiation of exact_topk (its LDS - two 33-KB operand stages + the candidate
// buffers - is 90 - 130 KB). Round 3 planned against two per CU: 79 query tiles x 4 chunks = 316 work-groups ran as a full
// round of 256 and a second one of 60 (MFMA pipe busy 56 % of the launch); against the real count 79 x 3 = 237 fill 93 % of
// ONE round.
int pick_chunks(int mtiles, int row_tiles, int pmax, int slots) {
    int p = 1;
    if (mtiles * 2 <= slots) p = std::max(1, slots / mtiles);
    else p = fullest_round(mtiles, slots, 1, std::min(pmax, 8), 0.9);   // the smallest p whose last round of work-groups is at least 90 % full (else the fullest)
    p = std::min(p, pmax);
    p = std::min(p, std::max(1, row_tiles));
    return std::max(1, p);
}

template <int KP, int E, int NW, int CAPV = 64 * E, int BK = 32, int OCC = 1, int GROUP = 32, bool BAND = false, bool MASK = false, bool BOOST = false>
int launch_exact(icd_index *x, const ExactArgs &a, int mtiles, hipStream_t s) {
    constexpr auto kern = exact_topk_kernel<KP, E, NW, CAPV, BK, OCC, GROUP, BAND, MASK, BOOST>;
    const size_t lds = exact_lds_bytes<KP, E, NW, CAPV, BK>();
    HIP_TRY(launch_lds<kern>(x->device, (size_t)((int)lds), dim3(mtiles * a.P), dim3(NW * 64), lds, s, a));
    return ICD_OK;
}

template <int D, int VAR = CF_PRODUCT_VAR, int KP = CO_KP, bool PERSIST = false>
int launch_coarse_flat(icd_index *x, const CoarseFlatArgs &a, int nwg, hipStream_t s) {
    constexpr auto kern = coarse_flat_kernel<D, VAR, KP, PERSIST>;
    constexpr int lds = cf_lds_bytes(VAR);
    HIP_TRY(launch_lds<kern>(x->device, (size_t)(lds), dim3(nwg), dim3(256), lds, s, a));
    return ICD_OK;
}

// streaming exact kernel + list reduction for a sparse query set (device-side gated when nq_ptr is given).
// p_out = 0: choose the smallest number of output lists (direct tiny-batch path); returns it in *p_used.
constexpr int LDS_LIMIT = 160 * 1024;   // LDS per CU (MI355X_MICROARCH.md)
constexpr size_t PIN_Q_BYTES = 64 * 1024;     // queries of a small host call (16 x 1024 floats)
constexpr size_t PIN_DONE_BYTES = 64;          // the completion word of a ONE-query host call (its own cache line)
constexpr size_t PIN_OUT_BYTES = 96 * 1024;   // their results: nq * k * 36 bytes over the six output arrays (nq * k <= 2730)

// does a pass of qb queries fit LDS with the minimum ring of two stages per wave?
inline bool stream_fits(int kp, int qb, int dim) {
    const int e = kp <= 32 ? 2 : (kp == 64 ? 3 : 4);
    return (size_t)qb * dim * 4 + (size_t)4 * 2 * ST_STAGE_BYTES + (size_t)4 * qb * 64 * e * 8 <= (size_t)LDS_LIMIT;
}

template <int KP, int E, int QB, bool BAND = false, bool MASK = false, bool BOOST = false>
int launch_stream(icd_index *x, const float *dq, const int *qlist, const int *nq_ptr, int nq, int max_active,
                  int p_out, int *p_used, hipStream_t s, const float *thr0 = nullptr, const BandQ *band = nullptr, RowMasks mask = nullptr,
                  const BoostQ *boost = nullptr) {
    const int n = (int)x->n;
    const int per_max = FIN_MAX_CAND / KP;                       // lists one reduce wave can merge
    const int p_cap = FIN_MAX_CAND / KP;                         // lists finalize<false> can merge
    const int rows_per_wg = stream_rows_per_wg(n, x->num_cu);   // (flat_partition.hpp)
    if ((long long)rows_per_wg * x->dim * 4 > FLAT_DESC_MAX_BYTES) return fail(ICD_ERR_UNSUPPORTED, "stream kernel: %d rows x dim %d per work-group exceed its buffer descriptor", rows_per_wg, x->dim);
    const int nwg = (n + rows_per_wg - 1) / rows_per_wg;
    int plan[8];
    const int levels = plan_reduce_levels(4 * nwg, per_max, p_out, p_cap, plan);
    if (levels <= 0) return fail(ICD_ERR_INVALID, "stream kernel: no reduction plan for %d lists (KP=%d, P=%d)", 4 * nwg, KP, p_out);
    p_out = plan[levels - 1];
    if (p_used) *p_used = p_out;
    StreamArgs a{};
    a.corpus = x->corpus; a.queries = dq; a.qlist = qlist; a.nq_ptr = nq_ptr; a.nq = std::min(nq, max_active);
    a.max_active = max_active; a.n = n; a.dim = x->dim; a.rows_per_wg = rows_per_wg; a.nwg = nwg;
    a.list_scores = x->lists_s; a.list_rows = x->lists_r; a.thr0 = thr0; a.band.q = band; a.mask = mask; a.boost = boost;
    // wave-private LDS ring: as many 8-KB stages per wave as fit next to the queries and candidate buffers
    int stages = 4;
    while (stages > 2 && stream_lds_bytes<KP, E, QB>(x->dim, stages) > (size_t)LDS_LIMIT) --stages;
    a.ring_stages = stages;
    if ((size_t)a.nq * 4 * nwg * KP > x->lists_cap) return fail(ICD_ERR_INVALID, "stream workspace too small");
    for (int l = 0; l < levels; ++l) {
        const size_t cap = (l % 2 == 0) ? x->partx_cap + (size_t)128 * FIN_MAX_CAND_X : x->lists_cap;
        if ((size_t)a.nq * plan[l] * KP > cap) return fail(ICD_ERR_INVALID, "stream workspace too small for reduction level %d", l);
    }
    constexpr auto kern = stream_topk_kernel<KP, E, QB, false, BAND, MASK, BOOST>;
    const size_t lds = stream_lds_bytes<KP, E, QB>(x->dim, stages);
    if (lds > (size_t)LDS_LIMIT) return fail(ICD_ERR_INVALID, "stream kernel: dim=%d does not fit LDS with %d queries per pass", x->dim, QB);
    HIP_TRY(launch_lds<kern>(x->device, (size_t)((int)lds), dim3(nwg), dim3(256), lds, s, a));
    int nlists = 4 * nwg;
    for (int l = 0; l < levels; ++l) {   // lists -> partx -> lists -> ... -> partx
        ReduceArgs r{};
        r.list_scores = (l % 2 == 0) ? x->lists_s : x->partx_s; r.list_rows = (l % 2 == 0) ? x->lists_r : x->partx_r;
        r.part_scores = (l % 2 == 0) ? x->partx_s : x->lists_s; r.part_rows = (l % 2 == 0) ? x->partx_r : x->lists_r;
        r.nlists = nlists; r.KP = KP; r.P_out = plan[l];
        r.nq_ptr = nq_ptr; r.nq = a.nq; r.max_active = max_active;
        hipLaunchKernelGGL(reduce_lists_kernel, dim3((a.nq * plan[l] + 3) / 4), dim3(256), 4 * 512 * 8, s, r);
        HIP_TRY(hipGetLastError());
        nlists = plan[l];
    }
    return ICD_OK;
}

// The reference's call shape - ONE query per MilvusService.search call (services/milvus_service.py:280-285), or two - as ONE
// launch: stream_topk_kernel<..., ONE = true> (stream_kernel.hpp) spreads the rows over every CU, merges the lists in the
// kernel (last-arriver ticket) and writes the final outputs itself. Geometry: rows per wave and step = the CU's share / 4,
// rounded up to whole 8-row LDS-DMA pieces (at most 64); the ring takes the stages that fit next to the candidate buffers.
struct StreamOnePlan { int rps, rows_per_wg, nwg, stages; };
inline bool plan_stream_one(int n, int dim, int num_cu, int qb, int cap_entries, StreamOnePlan *p) {
    const StreamOneRows g = plan_stream_one_rows(n, num_cu);   // (flat_partition.hpp)
    const int rps = g.rps;
    p->rps = g.rps; p->rows_per_wg = g.rows_per_wg; p->nwg = g.nwg;
    if ((long long)g.rows_per_wg * dim * 4 > FLAT_DESC_MAX_BYTES) return false;   // (the work-group's buffer descriptor)
    const size_t fixed = (size_t)qb * dim * 4 + (size_t)4 * qb * cap_entries * 8;
    if (fixed + (size_t)4 * 2 * rps * 128 > (size_t)LDS_LIMIT) return false;
    p->stages = (int)std::min<size_t>(8, ((size_t)LDS_LIMIT - fixed) / ((size_t)4 * rps * 128));
    return p->nwg >= 1 && p->nwg <= 256 && p->stages >= 2;
}

template <int KP, int E, int QB, bool BAND = false, bool MASK = false, bool BOOST = false>
int launch_stream_one(icd_index *x, const float *dq, int nq, const FinArgs &f, hipStream_t s, const float *host_q = nullptr, bool poll_done = false,
                      const BandArgs *band = nullptr, RowMasks mask = nullptr, const BoostQ *boost = nullptr) {
    StreamOnePlan pl;
    if (!plan_stream_one((int)x->n, x->dim, x->num_cu, QB, 64 * E, &pl)) return fail(ICD_ERR_INVALID, "single-launch stream kernel: no plan for n=%lld dim=%d", (long long)x->n, x->dim);
    if ((size_t)nq * pl.nwg * KP * 2 > x->lists_cap) return fail(ICD_ERR_INVALID, "stream workspace too small");
    StreamArgs a{};
    a.corpus = x->corpus; a.queries = dq; a.qlist = nullptr; a.nq_ptr = nullptr; a.nq = nq; a.max_active = nq;
    a.n = (int)x->n; a.dim = x->dim; a.rows_per_wg = pl.rows_per_wg; a.nwg = pl.nwg; a.ring_stages = pl.stages;
    a.rows_per_step = pl.rps;
    a.wg_keys = reinterpret_cast<u64 *>(x->lists_s);                    // (the per-wave lists' workspace: unused by this form)
    a.ticket = reinterpret_cast<u64 *>(x->nflag + 6);                   // nflag[6..7]: 8-byte aligned, zeroed at create, only ever counts up
    a.fin = f;
    a.fin.counters = x->nflag; a.fin.host_counters = x->h_nflag_dev;
    if (band) a.band = *band;
    a.mask = mask; a.boost = boost;
    if (poll_done) {
        a.done = reinterpret_cast<u64 *>(x->h_pin_dev + PIN_Q_BYTES + PIN_OUT_BYTES);
        a.done_value = ++x->done_seq;
        x->done_armed = true;
    }
    // (at least 84 KB: ONE work-group per CU whatever the corpus size - the fence-free sc1 hand-off of the kernel's tail is the
    //  form measured for one work-group per CU, MI355X_MICROARCH.md visibility table)
    const size_t lds = std::max<size_t>(stream_one_lds_bytes<KP, E, QB>(x->dim, pl.stages, pl.rps), (size_t)84 * 1024);
    constexpr auto kern = stream_topk_kernel<KP, E, QB, true, BAND, MASK, BOOST>;
    if constexpr (QB == 1) {
        if (host_q) {   // the vector in the kernel arguments: no copy command in front of the launch
            constexpr auto kern_in = stream_one_inline_kernel<KP, E, BAND, MASK, BOOST>;
            StreamInlineQuery iq;
            memcpy(iq.v, host_q, (size_t)x->dim * sizeof(float));
            a.queries = nullptr;
            HIP_TRY(launch_lds<kern_in>(x->device, (size_t)LDS_LIMIT, dim3(pl.nwg), dim3(256), lds, s, a, iq));
            return ICD_OK;
        }
    }
    HIP_TRY(launch_lds<kern>(x->device, (size_t)LDS_LIMIT, dim3(pl.nwg), dim3(256), lds, s, a));
    return ICD_OK;
}

template <bool RESCORE, bool DEEP, int EWM>
int launch_finalize_t(icd_index *x, const FinArgs &a, hipStream_t s) {
    constexpr auto kern = finalize_kernel<RESCORE, DEEP, EWM>;
    const size_t lds = 4 * fin_wave_lds_bytes(RESCORE, x->dim, a.lds_cand > 0 ? a.lds_cand : a.P * a.KP, EWM);
    // (the limit: the largest window this instantiation is ever launched with)
    const size_t lds_limit = (size_t)((int)(4 * fin_wave_lds_bytes(RESCORE, x->dim, (!RESCORE && EWM >= 4) ? FIN_MAX_CAND_X : FIN_MAX_CAND, EWM)));
    HIP_TRY(launch_lds<kern>(x->device, lds_limit, dim3((a.nq + 3) / 4), dim3(256), lds, s, a));
    return ICD_OK;
}

template <bool RESCORE>
int launch_finalize(icd_index *x, const FinArgs &a, hipStream_t s) {
    // one wave per query: up to ~28 waves per CU are resident, so a launch of a few thousand queries is a single
    // round of waves and its duration is one wave's latency: prefetch the rescoring rows deeper there
    const bool deep = RESCORE && a.nq <= 8 * x->num_cu;
    if (!RESCORE && std::max(a.lds_cand, a.P * a.KP) > FIN_MAX_CAND) return launch_finalize_t<false, false, 4>(x, a, s);   // (32 keys per lane)
    if (a.k <= 32) return deep ? launch_finalize_t<RESCORE, true, 1>(x, a, s) : launch_finalize_t<RESCORE, false, 1>(x, a, s);
    return deep ? launch_finalize_t<RESCORE, true, 4>(x, a, s) : launch_finalize_t<RESCORE, false, 4>(x, a, s);
}

void rec(icd_index *x, int i, hipStream_t s) {
    if (x->prof_now) {
        hipEventRecord(x->ev[i], s);
        x->ev_valid[i] = true;
    }
}

struct Outs {
    float *scores; long long *ids;
    double *adj; float *adj_raw; long long *adj_ids; int *adj_lv;
    int *lv;   // raw order (the range search's raw form; never together with adj_lv: the two share the staging of host callers)
};

// rows 0, stride, 2 stride, ... of the fp32 corpus as a query batch (the corpus-shape probe of icd_index_create)
__global__ void gather_rows_kernel(const float *src, float *dst, long long stride, int dim, int rows) {
    const int r = blockIdx.x;
    if (r >= rows) return;
    const float4 *s4 = reinterpret_cast<const float4 *>(src + (size_t)r * stride * dim);
    float4 *d4 = reinterpret_cast<float4 *>(dst + (size_t)r * dim);
    for (int i = threadIdx.x; i < dim / 4; i += blockDim.x) d4[i] = s4[i];
}

// A view's rows out of its parent (icd_index_create_view): ONE wave per selected row copies it from the parent's fp32 corpus with
// dwordx4 loads and stores (768 floats = three per lane), lane 0 its level. `map` holds the parent's global ids (validated on the
// host: strictly increasing, inside the parent), id_base is the parent's.
__global__ __launch_bounds__(256) void gather_view_rows_kernel(const float *src, const int *src_levels, const long long *map,
                                                               long long id_base, long long rows, int dim, float *dst, int *dst_levels) {
    const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= rows) return;
    const long long r = map[i] - id_base;
    const float4 *s4 = reinterpret_cast<const float4 *>(src + (size_t)r * dim);
    float4 *d4 = reinterpret_cast<float4 *>(dst + (size_t)i * dim);
    for (int c = lane; c < dim / 4; c += 64) d4[c] = s4[c];
    if (dst_levels && lane == 0) dst_levels[i] = src_levels[r];
}

// ---- A/B switches of the shipped kernels -------------------------------------------------------------------------------------
// `make ABLATE=1` builds a library whose searches read these from the environment (scripts/gpu_ab_*.sh, scripts/probe/); the
// product build knows the defaults only. Performance switches: the results are the same whatever they are set to.
struct SearchOverrides {
    int exact_cfg = 0;            // ICD_EXACT_CFG: 1 / 2 = earlier forms of exact_topk at k <= 16, 3 = the one-work-group-per-CU form at k <= 32
    int flat_u = 0;               // ICD_FLAT_U: at least this many tiles per work-group of the coarse sweep
    int flat_list = 0;            // ICD_FLAT_LIST: tiles per list (0: the planner's)
    int flat_boot = -1;           // ICD_FLAT_BOOT: bootstrap tiles (-1: the rule's)
    int flat_sparse = -1;         // ICD_FLAT_SPARSE: first tile of a list with the group pre-filter (-1: CO_SPARSE_FROM)
    int xcd_mode = -1;            // ICD_XCD_MODE: 0 identity, 1 XCD swizzle only, 2 classes unsplit
    bool dim1024_full = false;    // ICD_1024_FULL: dim 1024 with the 768 form of the coarse kernel
    bool fin_skip_walk = false;   // ICD_FIN_SKIP_WALK
    bool has_flat_var = false;    // ICD_FLAT_VAR: stage / select variants of the flat kernel (dim 768), those of ICD_FV_LIST when the build names them
    int flat_var = 0;
};
#ifdef ICD_ABLATE
SearchOverrides search_overrides() {
    SearchOverrides o;
    if (const char *e = getenv("ICD_EXACT_CFG")) o.exact_cfg = atoi(e);
    if (const char *e = getenv("ICD_FLAT_U")) o.flat_u = atoi(e);
    if (const char *e = getenv("ICD_FLAT_LIST")) o.flat_list = std::max(1, atoi(e));
    if (const char *e = getenv("ICD_FLAT_BOOT")) o.flat_boot = std::max(0, atoi(e));
    if (const char *e = getenv("ICD_FLAT_SPARSE")) o.flat_sparse = std::max(0, atoi(e));
    if (const char *e = getenv("ICD_XCD_MODE")) o.xcd_mode = atoi(e);
    o.dim1024_full = getenv("ICD_1024_FULL") != nullptr;
    o.fin_skip_walk = getenv("ICD_FIN_SKIP_WALK") != nullptr;
    if (const char *e = getenv("ICD_FLAT_VAR")) { o.has_flat_var = true; o.flat_var = atoi(e); }
    return o;
}
// the variant of exact_topk the overrides ask for at this list width, if any: true = taken, *rc its result
bool launch_exact_variant(icd_index *x, const SearchOverrides &ov, int kpx, const ExactArgs &a, int mtx, hipStream_t s, int *rc) {
    if (kpx == 16 && ov.exact_cfg == 1) *rc = launch_exact<16, 1, 4>(x, a, mtx, s);
    else if (kpx == 16 && ov.exact_cfg == 2) *rc = launch_exact<16, 1, 4, 64, 16, 1>(x, a, mtx, s);
    else if (kpx == 32 && ov.exact_cfg == 3) *rc = launch_exact<32, 2, 4, 112>(x, a, mtx, s);
    else return false;
    return true;
}
// ... and of the first coarse pass
bool launch_coarse_variant(icd_index *x, const SearchOverrides &ov, const CoarseFlatArgs &a, int nwg, hipStream_t s, int *rc) {
    if (x->dim == 1024) {
        if (!ov.dim1024_full) return false;
        *rc = launch_coarse_flat<1024, CF_PRODUCT_VAR>(x, a, nwg, s);   // A/B: the 768 form
        return true;
    }
    if (!ov.has_flat_var) return false;
    const int v = ov.flat_var;
    if (false) {}
#define ICD_FV_CASE(V) else if (v == V) *rc = launch_coarse_flat<768, V>(x, a, nwg, s);
#ifdef ICD_FV_LIST
    // (the look-ahead select's A/B, profiles/coarse_lookahead_ab.log: 6326427 = CF_CACHED_VAR without it, + 134217728 blocks of
    //  4, + 268435456 blocks of 8, + 536870912 the quad-maximum test; each also + 4096 for the compare path alone and + 1024 for
    //  the stamps and the append count)
    ICD_FV_LIST
#else
    ICD_FV_CASE(0) ICD_FV_CASE(139) ICD_FV_CASE(143) ICD_FV_CASE(155) ICD_FV_CASE(171) ICD_FV_CASE(187) ICD_FV_CASE(2187) ICD_FV_CASE(2203)
    ICD_FV_CASE(2235) ICD_FV_CASE(1163) ICD_FV_CASE(4235) ICD_FV_CASE(4251)
    ICD_FV_CASE(34971) ICD_FV_CASE(35995) ICD_FV_CASE(39067) ICD_FV_CASE(100507) ICD_FV_CASE(104603) ICD_FV_CASE(32923) ICD_FV_CASE(32955) ICD_FV_CASE(34843) ICD_FV_CASE(166043) ICD_FV_CASE(297115) ICD_FV_CASE(559259) ICD_FV_CASE(1083547)
#endif
#undef ICD_FV_CASE
    else *rc = fail(ICD_ERR_INVALID, "ICD_FLAT_VAR=%d is not built", v);
    return true;
}
#else
inline SearchOverrides search_overrides() { return SearchOverrides{}; }
inline bool launch_exact_variant(icd_index *, const SearchOverrides &, int, const ExactArgs &, int, hipStream_t, int *) { return false; }
inline bool launch_coarse_variant(icd_index *, const SearchOverrides &, const CoarseFlatArgs &, int, hipStream_t, int *) { return false; }
#endif

// ---- the search paths --------------------------------------------------------------------------------------------------------
// The boost table of a boosted search as the kernels get it (icd_boost.hpp stages it): [query] -> BoostQ, and the all-zero bitset.
struct BoostDev {
    const BoostQ *q;
    const uint32_t *zeros;
};

// What the four paths of a search share, computed once by search_device.
struct SearchCtx {
    icd_index *x;
    const float *dq;
    int nq, k;
    hipStream_t s;
    SearchOverrides ov;
    bool use_fast;       // AUTO on an index with an fp16 image
    int row_tiles;
    FinArgs f;           // what every finalize launch of this search starts from
    // exact-kernel configuration (full run, or fallback over the flagged list)
    int kpx, nwx;
    int wg_per_cu_x;     // work-groups of exact_topk a CU holds (its LDS)
    int bmq, mtx;
    int cand_x, pmax_x;  // lists per query finalize<false> merges: 2048 candidates at k <= 64 (its top-k prefilter keeps that cheap), 512 above
    int p_dense_max;     // chunk limit of the device-sized partition of a flagged list
    // sparse: streaming kernel (+ list reduction) instead of / next to the MFMA exact kernel
    // queries per pass: host-known for direct calls (1, 2, 4 or 8), 8 for the device-gated fallback
    int p_sparse;        // lists per slot that finalize<false> merges (32 / 8 / 4)
    int sparse_max;      // how many flagged queries still go to the streaming kernel
    bool stream_ok;      // small batches (the reference's one-query-per-call shape): stream the corpus once, exact, no coarse pass
    const BandArgs *band;   // range search: the queries' bands (nullptr: none, and no band kernel runs)
    RowMasks mask;          // masked search (with band): [query] -> bitset in device memory (nullptr: none, and no mask kernel runs)
    const BoostDev *boost;  // boosted search (with band and mask): [query] -> boosts in device memory (nullptr: none, and no boost kernel runs)
};

SearchCtx make_search_ctx(icd_index *x, const float *dq, int nq, int k, bool use_fast, const Outs &o, hipStream_t s, const BandArgs *band, RowMasks mask,
                          const BoostDev *boost) {
    SearchCtx c{};
    c.x = x; c.dq = dq; c.nq = nq; c.k = k; c.s = s; c.use_fast = use_fast; c.band = band; c.mask = mask; c.boost = boost;
    c.ov = search_overrides();
    c.row_tiles = (int)((x->n + 127) / 128);
    FinArgs &f = c.f;
    f.k = k; f.queries = dq; f.corpus = x->corpus; f.dim = x->dim; f.qnorm = x->qnorm; f.qbad = x->qbad;
    f.qexp = x->qexp; f.qres = x->qres; f.cexp = x->cexp; f.nflag = x->nflag; f.flagged = x->flagged;
    f.cmax16 = cert_cmax16(x->rmax_scaled, x->dcmax_scaled); f.dcmax = x->dcmax_scaled; f.acc_rel = cert_acc_rel(x->dim);
    if (use_fast) f.thr0 = x->thr0;
    if (x->cmean) { f.rmax_unc = x->rmax_unc_scaled; f.eps_f32 = 2.0f * (float)x->dim * 5.9604645e-8f; }
    f.levels = x->levels; f.id_base = x->id_base; f.row_map = x->row_map;
    f.out_scores = o.scores; f.out_ids = o.ids; f.out_adj = o.adj; f.out_adj_raw = o.adj_raw;
    f.out_adj_ids = o.adj_ids; f.out_adj_levels = o.adj_lv; f.out_levels = o.lv;

    c.kpx = exact_kp_for(k);
    c.nwx = c.kpx <= 64 ? 4 : 2;
    c.wg_per_cu_x = c.kpx <= 32 ? 2 : 1;
    if (c.kpx == 32 && c.ov.exact_cfg == 3) c.wg_per_cu_x = 1;
    c.bmq = c.nwx * 32;
    c.mtx = (nq + c.bmq - 1) / c.bmq;
    c.cand_x = c.kpx <= 64 ? FIN_MAX_CAND_X : FIN_MAX_CAND;
    c.pmax_x = std::min(64, c.cand_x / c.kpx);
    c.p_dense_max = c.cand_x / c.kpx;
    c.p_sparse = FIN_MAX_CAND / c.kpx;
    // How many flagged queries still go to the streaming kernel: it re-reads the corpus once per 8 queries (~37 us at
    // 37k rows); the fp32-MFMA kernel, its short list cut into up to 2048 / KP chunks, needs ~0.22 ms for any count up to a
    // few hundred: they meet near 45 (ST_FALLBACK_MAX_ACTIVE, stream_kernel.hpp); the list workspace caps it by k.
    // (the first reduction level leaves at most 512 lists per slot in the second workspace)
    c.sparse_max = (int)std::min<size_t>(std::min<size_t>(ST_FALLBACK_MAX_ACTIVE, x->lists_cap / ((size_t)1024 * c.kpx)),
                                         c.kpx == 16 ? (size_t)ST_FALLBACK_MAX_ACTIVE : x->partx_cap / ((size_t)512 * c.kpx));
    c.stream_ok = x->dim % (32 * ST_PF) == 0 && stream_fits(c.kpx, 1, x->dim);
    return c;
}

int run_stream(const SearchCtx &c, const int *qlist, const int *nq_ptr, int nqs, int p_out, int *p_used, const float *thr0 = nullptr) {
    icd_index *x = c.x;
    int qb = nq_ptr ? 8 : (nqs <= 1 ? 1 : (nqs <= 2 ? 2 : (nqs <= 4 ? 4 : 8)));
    const int max_act = nq_ptr ? c.sparse_max : std::max(c.sparse_max, nqs);   // (a direct call - up to ST_MAX_ACTIVE queries - is not gated)
    while (qb > 1 && !stream_fits(c.kpx, qb, x->dim)) qb >>= 1;
#define ICD_ST_B(KPV, EV, BANDV, BQ, MASKV, MQ, BOOSTV, OQ) \
    (qb == 1 ? launch_stream<KPV, EV, 1, BANDV, MASKV, BOOSTV>(x, c.dq, qlist, nq_ptr, nqs, max_act, p_out, p_used, c.s, thr0, BQ, MQ, OQ) : \
     qb == 2 ? launch_stream<KPV, EV, 2, BANDV, MASKV, BOOSTV>(x, c.dq, qlist, nq_ptr, nqs, max_act, p_out, p_used, c.s, thr0, BQ, MQ, OQ) : \
     qb == 4 ? launch_stream<KPV, EV, 4, BANDV, MASKV, BOOSTV>(x, c.dq, qlist, nq_ptr, nqs, max_act, p_out, p_used, c.s, thr0, BQ, MQ, OQ) : \
               launch_stream<KPV, EV, 8, BANDV, MASKV, BOOSTV>(x, c.dq, qlist, nq_ptr, nqs, max_act, p_out, p_used, c.s, thr0, BQ, MQ, OQ))
#define ICD_ST_M(KPV, EV, BANDV, BQ, MASKV, MQ) ICD_ST_B(KPV, EV, BANDV, BQ, MASKV, MQ, false, nullptr)
#define ICD_ST(KPV, EV, BANDV, BQ) ICD_ST_M(KPV, EV, BANDV, BQ, false, nullptr)
    if (c.band && c.mask && c.boost) {   // (boosted search: the masked instantiations with the boost multiply)
        if (c.kpx == 16) return ICD_ST_B(16, 2, true, c.band->q, true, c.mask, true, c.boost->q);
        if (c.kpx == 32) return ICD_ST_B(32, 2, true, c.band->q, true, c.mask, true, c.boost->q);
        if (c.kpx == 64) return ICD_ST_B(64, 3, true, c.band->q, true, c.mask, true, c.boost->q);
        return ICD_ST_B(128, 4, true, c.band->q, true, c.mask, true, c.boost->q);
    }
    if (c.band && c.mask) {   // (masked search: the band instantiations with the row-mask term)
        if (c.kpx == 16) return ICD_ST_M(16, 2, true, c.band->q, true, c.mask);
        if (c.kpx == 32) return ICD_ST_M(32, 2, true, c.band->q, true, c.mask);
        if (c.kpx == 64) return ICD_ST_M(64, 3, true, c.band->q, true, c.mask);
        return ICD_ST_M(128, 4, true, c.band->q, true, c.mask);
    }
    if (c.band) {   // (range search: the same sweep, band instantiations)
        if (c.kpx == 16) return ICD_ST(16, 2, true, c.band->q);
        if (c.kpx == 32) return ICD_ST(32, 2, true, c.band->q);
        if (c.kpx == 64) return ICD_ST(64, 3, true, c.band->q);
        return ICD_ST(128, 4, true, c.band->q);
    }
    if (c.kpx == 16) return ICD_ST(16, 2, false, nullptr);
    if (c.kpx == 32) return ICD_ST(32, 2, false, nullptr);
    if (c.kpx == 64) return ICD_ST(64, 3, false, nullptr);
    return ICD_ST(128, 4, false, nullptr);
#undef ICD_ST
#undef ICD_ST_M
#undef ICD_ST_B
}

// A chunk count the exact kernel's list workspace holds for EVERY query of the batch (all of them may be flagged: all-zero
// queries, duplicate rows): lowered until it fits, an error if one chunk does not, then rounded to whole row tiles per chunk.
int fit_chunks(const SearchCtx &c, int *p) {
    const icd_index *x = c.x;
    int px = *p;
    while (px > 1 && (size_t)c.nq * px * c.kpx > x->partx_cap) --px;
    if ((size_t)c.nq * px * c.kpx > x->partx_cap) return fail(ICD_ERR_INVALID, "workspace too small for nq=%d k=%d", c.nq, c.k);
    const int tiles_per = (c.row_tiles + px - 1) / px;
    *p = (c.row_tiles + tiles_per - 1) / tiles_per;
    return ICD_OK;
}

// The exact search of every path: over all queries (qlist / nq_ptr null) or over a flagged list whose length only the device
// knows. `stream`: the streaming kernel + list reduction takes up to sparse_max queries; `mfma`: exact_topk takes the rest;
// finalize<false> merges either's lists and is the last launch of the search (it copies the counters to the host).
int run_exact(const SearchCtx &c, const int *qlist, const int *nq_ptr, int px, bool mfma, bool stream, bool stream_launch = true,
              bool track_run = false, const float *thr0 = nullptr) {
    icd_index *x = c.x;
    const int nq = c.nq, kpx = c.kpx;
    hipStream_t s = c.s;
    const int sparse_here = stream_launch ? c.sparse_max : 0;   // (streaming pair left out: the MFMA kernel takes every count >= 1)
    if (!nq_ptr) x->last_chunks = px;   // (the fallback keeps the coarse pass's chunk count)
    int rc = ICD_OK;
    if (stream && stream_launch) {
        int used = px;
        rc = run_stream(c, qlist, nq_ptr, nq, mfma ? px : 0, &used, thr0);   // alone: fewest output lists
        if (rc) return rc;
        px = used;
        if (!nq_ptr) x->last_chunks = px;
    }
    int px_dense = 0;
    if (mfma) {
        // The MFMA kernel may have to take EVERY query (all of them flagged): its list count is sized against
        // the workspace like a full exact run; only the streaming kernel (<= ST_MAX_ACTIVE slots) uses px.
        int pm = px;
        if (stream) {
            pm = pick_chunks(c.mtx, c.row_tiles, c.pmax_x, x->num_cu * c.wg_per_cu_x);
            rc = fit_chunks(c, &pm);
            if (rc) return rc;
            px_dense = pm;
        }
        ExactArgs a{};
        a.corpus = x->corpus; a.queries = c.dq; a.qlist = qlist; a.nq_ptr = nq_ptr; a.nq = nq;
        a.min_active = stream ? sparse_here : 0;
        a.adaptive_one_per_cu = c.wg_per_cu_x > 1 ? x->num_cu : 0;
        a.adaptive_max_p = stream ? c.p_dense_max : 0;   // fallback: the chunk count follows the actual flagged count
        a.n = (int)x->n; a.dim = x->dim; a.P = pm;
        a.rows_per_chunk = ((c.row_tiles + pm - 1) / pm) * 128;
        a.part_scores = x->partx_s; a.part_rows = x->partx_r; a.thr0 = thr0;
        // (LDS: k <= 16 two work-groups per CU - 17 KB of stage + 60-entry buffers; k <= 64 one of four waves - 34 KB +
        //  112-entry buffers; larger k two waves. Eight waves on 64-entry buffers at k <= 32 - two per SIMD - were built and
        //  are slower, 9.2 against 7.2 ms per 10 000 queries: a 64-entry buffer with 32 kept is compacted after every append)
        if (c.band && c.mask && c.boost) {   // (boosted search: the masked instantiations with the boost multiply)
            a.band = c.band->q; a.mask = c.mask; a.boost = c.boost->q; a.boost_zeros = c.boost->zeros;
            if (kpx == 16) rc = launch_exact<16, 1, 4, 60, 16, 2, 32, true, true, true>(x, a, c.mtx, s);
            else if (kpx == 32) rc = launch_exact<32, 1, 4, 62, 16, 2, 16, true, true, true>(x, a, c.mtx, s);
            else if (kpx == 64) rc = launch_exact<64, 2, 4, 112, 32, 1, 32, true, true, true>(x, a, c.mtx, s);
            else rc = launch_exact<128, 3, 2, 192, 32, 1, 32, true, true, true>(x, a, c.mtx, s);
        }
        else if (c.band && c.mask) {   // (masked search: the band instantiations with the row-mask term)
            a.band = c.band->q; a.mask = c.mask;
            if (kpx == 16) rc = launch_exact<16, 1, 4, 60, 16, 2, 32, true, true>(x, a, c.mtx, s);
            else if (kpx == 32) rc = launch_exact<32, 1, 4, 62, 16, 2, 16, true, true>(x, a, c.mtx, s);
            else if (kpx == 64) rc = launch_exact<64, 2, 4, 112, 32, 1, 32, true, true>(x, a, c.mtx, s);
            else rc = launch_exact<128, 3, 2, 192, 32, 1, 32, true, true>(x, a, c.mtx, s);
        }
        else if (c.band) {   // (range search: the same four configurations, band instantiations)
            a.band = c.band->q;
            if (kpx == 16) rc = launch_exact<16, 1, 4, 60, 16, 2, 32, true>(x, a, c.mtx, s);
            else if (kpx == 32) rc = launch_exact<32, 1, 4, 62, 16, 2, 16, true>(x, a, c.mtx, s);
            else if (kpx == 64) rc = launch_exact<64, 2, 4, 112, 32, 1, 32, true>(x, a, c.mtx, s);
            else rc = launch_exact<128, 3, 2, 192, 32, 1, 32, true>(x, a, c.mtx, s);
        }
        else if (launch_exact_variant(x, c.ov, kpx, a, c.mtx, s, &rc)) {}
        else if (kpx == 16) rc = launch_exact<16, 1, 4, 60, 16, 2>(x, a, c.mtx, s);
        else if (kpx == 32) rc = launch_exact<32, 1, 4, 62, 16, 2, 16>(x, a, c.mtx, s);
        else if (kpx == 64) rc = launch_exact<64, 2, 4, 112>(x, a, c.mtx, s);
        else rc = launch_exact<128, 3, 2>(x, a, c.mtx, s);
        if (rc) return rc;
    }
    rec(x, 4, s);
    FinArgs g = c.f;
    g.part_scores = x->partx_s; g.part_rows = x->partx_r; g.P = px; g.KP = kpx;
    g.P_dense = px_dense; g.sparse_max = sparse_here; g.track_run = track_run ? 1 : 0; g.lds_cand = std::max(px, (stream && mfma) ? c.p_dense_max : px_dense) * kpx;
    g.dense_grid = c.mtx * std::max(1, px_dense); g.dense_bmq = c.bmq; g.dense_max_p = (stream && mfma) ? c.p_dense_max : 0; g.dense_one_per_cu = c.wg_per_cu_x > 1 ? x->num_cu : 0; g.n_rows = (int)x->n;
    g.nq = nq; g.nq_ptr = nq_ptr; g.qlist = qlist;
    g.counters = x->nflag; g.host_counters = x->h_nflag_dev;   // (the last launch of every search: no separate copy)
    rc = launch_finalize<false>(x, g, s);
    rec(x, 5, s);
    return rc;
}

// a host caller's ONE query whose copy run_search left out (host_q): every path but the single-launch kernel wants it
// in device memory after all - the copy it would have got, enqueued before anything that reads dq
int stage_host_query(const SearchCtx &c) {
    icd_index *x = c.x;
    if (!x->host_q) return ICD_OK;
    const size_t qbytes = (size_t)x->dim * sizeof(float);
    memcpy(x->h_pin, x->host_q, qbytes);
    HIP_TRY(hipMemcpyAsync(x->qdev, x->h_pin, qbytes, hipMemcpyHostToDevice, c.s));
    x->host_q = nullptr;
    return ICD_OK;
}

// host-packed bands of a range search (icd_index_search_range left them in the pinned block): every path but the single-launch
// kernel - which takes them in its arguments - reads them from device memory
int stage_host_bands(const SearchCtx &c) {
    icd_index *x = c.x;
    if (!c.band || x->band_pending <= 0) return ICD_OK;
    HIP_TRY(hipMemcpyAsync(x->band_dev, x->h_band, (size_t)x->band_pending * sizeof(BandQ), hipMemcpyHostToDevice, c.s));
    x->band_pending = 0;
    return ICD_OK;
}

// (the fallback counter starts every search at zero: the exact-only paths clear it themselves, the fast path in its
//  query-prep launch - one launch less per step)

// ---- path 1: a handful of queries, streamed (exact, no coarse pass) ---------------------------------------------------------
int search_tiny(const SearchCtx &c) {
    icd_index *x = c.x;
    const int nq = c.nq;
    hipStream_t s = c.s;
    x->last_mode = ICD_MODE_EXACT;
    x->last_chunks = c.p_sparse;
    StreamOnePlan pl;
    // (up to FOUR queries: at eight the sweep is bound by the lanes' fmaf chains, not by memory - 40 of a wave's 64 lanes hold
    //  rows in this form - and the general path is 12 us faster: profiles/r05_single_query.log)
    const int qb1 = nq <= 1 ? 1 : (nq <= 2 ? 2 : 4);
    const bool one = nq <= 4 && c.kpx == 16 && x->opt_stream_one && plan_stream_one((int)x->n, x->dim, x->num_cu, qb1, 64 * 2, &pl) &&
                     (size_t)nq * pl.nwg * c.kpx * 2 <= x->lists_cap;
    if (one) {   // up to four queries (the reference's call shape is ONE; a /query request batches its D diagnoses): ONE launch,
                 // no memset, no reduction, no finalize
        rec(x, 3, s);
        const float *hq = qb1 == 1 ? x->host_q : nullptr;   // (a host caller's ONE query: run_search left the copy out)
        if (!hq) { const int rcq = stage_host_query(c); if (rcq) return rcq; }
        const bool poll = x->host_one_call && (x->opt_host_one & 2) != 0;
        if (c.band) {   // a page of a range search: still ONE launch (host-packed bands travel in the arguments)
            BandArgs b = *c.band;
            if (x->band_pending > 0) { b.q = nullptr; x->band_pending = 0; }
            if (c.mask && c.boost) {   // (the boost table is in device memory already, like the pointer table: run_search copied both)
                const int rco = qb1 == 1 ? launch_stream_one<16, 2, 1, true, true, true>(x, c.dq, 1, c.f, s, hq, poll, &b, c.mask, c.boost->q)
                              : qb1 == 2 ? launch_stream_one<16, 2, 2, true, true, true>(x, c.dq, 2, c.f, s, nullptr, false, &b, c.mask, c.boost->q)
                                         : launch_stream_one<16, 2, 4, true, true, true>(x, c.dq, (int)nq, c.f, s, nullptr, false, &b, c.mask, c.boost->q);
                rec(x, 4, s);
                rec(x, 5, s);
                return rco;
            }
            if (c.mask) {   // (the pointer table is in device memory already: run_search copied it)
                const int rcm = qb1 == 1 ? launch_stream_one<16, 2, 1, true, true>(x, c.dq, 1, c.f, s, hq, poll, &b, c.mask)
                              : qb1 == 2 ? launch_stream_one<16, 2, 2, true, true>(x, c.dq, 2, c.f, s, nullptr, false, &b, c.mask)
                                         : launch_stream_one<16, 2, 4, true, true>(x, c.dq, (int)nq, c.f, s, nullptr, false, &b, c.mask);
                rec(x, 4, s);
                rec(x, 5, s);
                return rcm;
            }
            const int rcb = qb1 == 1 ? launch_stream_one<16, 2, 1, true>(x, c.dq, 1, c.f, s, hq, poll, &b)
                          : qb1 == 2 ? launch_stream_one<16, 2, 2, true>(x, c.dq, 2, c.f, s, nullptr, false, &b)
                                     : launch_stream_one<16, 2, 4, true>(x, c.dq, (int)nq, c.f, s, nullptr, false, &b);
            rec(x, 4, s);
            rec(x, 5, s);
            return rcb;
        }
        const int rc1 = qb1 == 1 ? launch_stream_one<16, 2, 1>(x, c.dq, 1, c.f, s, hq, poll) : qb1 == 2 ? launch_stream_one<16, 2, 2>(x, c.dq, 2, c.f, s)
                      : launch_stream_one<16, 2, 4>(x, c.dq, (int)nq, c.f, s);
        rec(x, 4, s);
        rec(x, 5, s);
        return rc1;
    }
    { const int rcq = stage_host_query(c); if (rcq) return rcq; }
    { const int rcb = stage_host_bands(c); if (rcb) return rcb; }
    HIP_TRY(hipMemsetAsync(x->nflag, 0, sizeof(int), s));
    rec(x, 3, s);
    return run_exact(c, nullptr, nullptr, c.p_sparse, false, true);
}

// ---- path 2: EXACT at k > 32, NARROW certified lists ------------------------------------------------------------------------
// Lists of KP >= k need 64- or 128-entry candidate buffers: one work-group of four waves per CU at k <= 64, of two above
// (0.39 / 0.15 of the fp32 MFMA peak at k = 50 / 100, against 0.59 at k = 20). Instead: the k <= 32 configuration (lists
// of 32, two work-groups per CU) over ROW-STRIDED chunks - chunk c holds rows c, c + P, ... so that neighbouring rows
// (an ICD family in code order) spread evenly - with P large enough that a list holds ~k / P << 32 members of the top-k,
// and finalize CHECKS it: a full list whose worst kept key beats the k-th best of the merge may have dropped a member
// of the top-k; such a query is re-searched with KP >= k lists (the flagged-list machinery of the AUTO fallback).
// Results are the exact top-k either way. *taken = false: the lists do not fit the workspace, the plain path takes the search.
int search_exact_narrow(const SearchCtx &c, bool *taken) {
    icd_index *x = c.x;
    const int nq = c.nq, k = c.k;
    hipStream_t s = c.s;
    *taken = false;
    HIP_TRY(hipMemsetAsync(x->nflag, 0, sizeof(int), s));
    const int slots = x->num_cu * 2;
    const int mtx_n = (nq + 127) / 128;                   // query tiles of THIS configuration (four waves x 32 queries; c.mtx counts the KP >= k configuration's tiles, 64 queries at k > 64: ADVICE r5)
    const int p_need = std::max(2, (k + 7) / 8);          // ~8 members of the top-k per list when they spread evenly
    // the count at or above p_need whose last round of work-groups is fullest (a short batch: enough chunks to fill the chip)
    const int pn = fullest_round(mtx_n, slots, p_need, std::min(FIN_MAX_CAND_X / 32, std::max(p_need + 8, slots / std::max(1, mtx_n))), 2.0);
    if (!((size_t)nq * pn * 32 <= x->partx_cap && pn * 32 <= FIN_MAX_CAND_X)) return ICD_OK;
    *taken = true;
    x->last_chunks = pn;
    x->fallback_word = 0;
    rec(x, 3, s);
    ExactArgs a{};
    a.corpus = x->corpus; a.queries = c.dq; a.nq = nq; a.n = (int)x->n; a.dim = x->dim; a.P = pn; a.strided = 1;
    a.rows_per_chunk = 128;   // (unused by the strided form)
    a.part_scores = x->partx_s; a.part_rows = x->partx_r;
    int rc = launch_exact<32, 1, 4, 62, 16, 2, 16>(x, a, mtx_n, s);
    if (rc) return rc;
    rec(x, 4, s);
    FinArgs g = c.f;
    g.part_scores = x->partx_s; g.part_rows = x->partx_r; g.P = pn; g.KP = 32; g.nq = nq; g.lds_cand = pn * 32;
    g.narrow_check = 1; g.nflag = x->nflag; g.flagged = x->flagged;
    rc = launch_finalize<false>(x, g, s);
    if (rc) return rc;
    rec(x, 5, s);
    // the queries the check could not clear (none on data whose rows spread): KP >= k lists over the flagged list
    return run_exact(c, x->flagged, x->nflag, std::min(c.p_sparse, c.row_tiles), true, c.stream_ok, true, false, nullptr);
}

// ---- path 3: plain EXACT ------------------------------------------------------------------------------------------------------
int search_exact(const SearchCtx &c) {
    icd_index *x = c.x;
    HIP_TRY(hipMemsetAsync(x->nflag, 0, sizeof(int), c.s));
    int px = pick_chunks(c.mtx, c.row_tiles, c.pmax_x, x->num_cu * c.wg_per_cu_x);
    const int rc = fit_chunks(c, &px);
    if (rc) return rc;
    x->last_chunks = px;
    rec(x, 3, c.s);
    return run_exact(c, nullptr, nullptr, px, true, false);
}

// ---- path 4: AUTO = prep -> coarse -> finalize(certify + rescore) -> retry -> second pass -> exact fallback -----------------
// The plan of the two coarse passes of one AUTO search.
struct AutoPlan {
    bool wide_lists;     // 24 candidates per list instead of 16 (large k)
    bool wide_now;       // wide mode: the first pass planned with the second pass's list count
    bool sparse_off;     // the exact re-search goes without the streaming pair
    int kp_c;            // candidates per list of the first pass
    int ctiles, U, nwg;  // corpus tiles swept, tiles per work-group and work-groups of the first pass
    int pc;              // its lists per query
    CoarseFlatArgs a;
    int p2, nwg2;        // the second pass: lists per query (0: none) and logical work-groups of a full batch
    CoarseFlatArgs a2;   // (nq_ptr / qlist set at the launch: which flag word / list feeds it)
};

// query prep: fp16 queries, norms and scales; clears the coarse thresholds and the fallback counters
int auto_prep(const SearchCtx &c, int nq_pad) {
    icd_index *x = c.x;
    ConvertArgs cv{};
    cv.src = c.dq; cv.dst = x->q16; cv.rows = c.nq; cv.rows_pad = nq_pad; cv.dim = x->dim; cv.mode = 0;
    cv.norm = x->qnorm; cv.res = x->qres; cv.scale_exp = x->qexp; cv.bad = x->qbad; cv.zero_u32 = x->shared_thr; cv.zero_i32 = x->nflag;
    cv.zero_u32b = x->shared_thr + x->max_nq_pad;
    hipLaunchKernelGGL(convert_rows_kernel, dim3((nq_pad + 3) / 4), dim3(256), 0, c.s, cv);
    HIP_TRY(hipGetLastError());
    rec(x, 1, c.s);
    return ICD_OK;
}

// A class of work-groups that stream the same tiles should have about a dozen members per XCD-local group: many more and
// they all hit the same L2 channel at the same time (measured slower), so large classes are split into sub-classes
// (l mod T s also start on the same tile). xcd_mode: the A/B switch (0 identity, 1 XCD swizzle only, 2 classes unsplit).
int split_class_period(int U, int ctiles, int nwg, int xcd_mode = -1) {
    int period = flat_class_period(U, ctiles);
    const int members = nwg / std::max(1, period);
    int split = (members + 11) / 12;
    if (xcd_mode == 0) period = 0;
    else if (xcd_mode == 1) period = 1 << 30;
    else if (xcd_mode == 2) split = 1;
    if (period > 0 && period < (1 << 20)) period *= std::max(1, split);
    return period;
}

// Takes in the previous search's counters (when they have arrived), decides this search's shape and plans both passes:
// the flat partition of the (query tile x corpus tile) grid over the CUs (coarse_flat_kernel.hpp).
int auto_plan(const SearchCtx &c, int nq_pad, AutoPlan &pl) {
    icd_index *x = c.x;
    const int nq = c.nq, k = c.k;
    const int mtc = nq_pad / 128;
    // corpus tiles to sweep and tiles per work-group (flat_partition.hpp: a few zero tiles behind the corpus buy a tile
    // count that shares a factor with U, i.e. work-groups that stream the same tiles together)
    const int ctiles_min = (int)((x->n + 127) / 128);
    const FlatPlan plan = plan_flat_tiles(mtc, ctiles_min, x->n_pad / 128 - ctiles_min, x->num_cu);
    const int ctiles = plan.ctiles;
    pl.ctiles = ctiles;
    pl.wide_lists = k > x->opt_wide_from && x->dim == 768;
    // ---- adaptive list count of large batches (search_policy.hpp) ------------------------------------------------------
    // The counters of the previous search sit in pinned host memory once its copy event has completed (hipEventQuery: no
    // wait).
    // (while the stream is being captured into a HIP graph nothing may be queried: the plan is the one the host state gives now,
    //  and it is frozen into the graph - a performance decision only, the replayed search returns the exact top-k either way)
    const bool counters_in = !x->capturing && hipEventQuery(x->ev_nflag) == hipSuccess;   // (every search enqueued so far has completed)
    if (counters_in) policy_take_counters(x->pol, search_counters(x->h_nflag));
    const SearchDecision dec = policy_decide(x->pol, x->adapt_enabled, nq, k, x->chunks_override);
    pl.sparse_off = dec.sparse_off;
    pl.wide_now = dec.wide_now;
    pl.kp_c = pl.wide_lists ? CO_KP_WIDE : CO_KP;

    CoarseFlatArgs &a = pl.a;
    a = CoarseFlatArgs{};
    a.q16 = x->q16; a.c16 = x->c16; a.nq = nq; a.n = (int)x->n; a.n_pad = ctiles * 128; a.ctiles = ctiles;
    a.total_units = mtc * ctiles;
    // The bootstrap level (6th best of the first boot_tiles * 128 rows of a list) must stay far below the k-th best
    // of the whole corpus or the list's bound lands inside the window: fewer tiles for larger k (measured at
    // k = 48 with 8 tiles: 1.6 % of the queries uncertified).
    a.boot_tiles = c.ov.flat_boot >= 0 ? c.ov.flat_boot : std::max(1, std::min(CO_BOOT_TILES, 96 / std::max(1, k)));
    a.sparse_from = c.ov.flat_sparse >= 0 ? c.ov.flat_sparse : CO_SPARSE_FROM;
    // ---- the list plan of both passes (flat_partition.hpp plan_coarse_lists): lists per query, tiles per list and
    // per work-group. No list is longer than the kernel's per-list buffer descriptor reaches (flat_max_list_tiles).
    CoarsePlanIn pin{};
    pin.mtc = mtc; pin.ctiles = ctiles; pin.U = std::max(plan.U, c.ov.flat_u); pin.nq = nq; pin.k = k;
    pin.kp = pl.kp_c; pin.kp2 = CO_KP; pin.max_cand = FIN_MAX_CAND;
    pin.wide_lists = pl.wide_lists; pin.wide_now = pl.wide_now; pin.chunks_override = x->chunks_override;
    pin.pass2 = x->pass2_enabled && x->pol.pass2_armed() && x->part2_s;
    pin.partc_cap = (long long)x->partc_cap; pin.part2_cap = (long long)x->part2_cap;
    pin.max_list_tiles = flat_max_list_tiles(x->dim);
    if (c.ov.flat_list > 0) pin.list_override = c.ov.flat_list;
    const CoarsePlan cp = plan_coarse_lists(pin);
    if (!cp.ok)
        return fail(ICD_ERR_UNSUPPORTED, "coarse pass: no list plan for n=%lld dim=%d nq=%d k=%d (lists per query %d, at most %d tiles per list)",
                    (long long)x->n, x->dim, nq, k, cp.P, pin.max_list_tiles);
    const int U = cp.U;
    pl.U = U; pl.pc = cp.P;
    x->last_chunks = cp.P;
    pl.nwg = (a.total_units + U - 1) / U;
    a.list_tiles = cp.list_tiles;
    a.units_per_wg = U; a.P = cp.P;
    a.pos_period = split_class_period(U, ctiles, pl.nwg, c.ov.xcd_mode);
    a.part_scores = x->partc_s; a.part_rows = x->partc_r; a.bounds = x->partc_b; a.shared_thr = x->shared_thr;
    a.dbg = x->dbg;
    a.nwg_virtual = pl.nwg;
    // ---- the second pass's plan: the same sweep cut into about PASS2_CHUNKS lists per query, every work-group's run
    // one list (the shape icd_index_set_chunks asks for). Everything the host must know is independent of how many
    // queries will be flagged: U2, the list slots per query (worst case over all query tiles of the full batch), the
    // logical work-group count of a full batch. The kernel sizes the sweep from the flagged count on the device.
    pl.p2 = 0; pl.nwg2 = 0;
    pl.a2 = CoarseFlatArgs{};
    if (cp.P2 > 0) {
        const int U2 = cp.U2;
        CoarseFlatArgs &a2 = pl.a2;
        pl.p2 = cp.P2;
        a2 = a;
        a2.nq_ptr = nullptr; a2.qlist = nullptr;
        a2.units_per_wg = U2; a2.list_tiles = cp.list_tiles2; a2.P = pl.p2;
        a2.boot_tiles = a.boot_tiles;
        pl.nwg2 = (int)(((long long)mtc * ctiles + U2 - 1) / U2);
        a2.pos_period = split_class_period(U2, ctiles, pl.nwg2);
        a2.nwg_virtual = pl.nwg2;
        a2.part_scores = x->part2_s; a2.part_rows = x->part2_r; a2.bounds = x->part2_b;
        a2.shared_thr = x->shared_thr + x->max_nq_pad;
    }
    return ICD_OK;
}

// the first coarse pass: which form of the flat kernel sweeps the fp16 image
int auto_coarse(const SearchCtx &c, AutoPlan &pl) {
    icd_index *x = c.x;
    hipStream_t s = c.s;
    CoarseFlatArgs &a = pl.a;
    const int nwg = pl.nwg;
    int rc;
    // (dim 1024: the query fragments alone are 256 registers: no pinning, no deeper fragment prefetch and the 32x32x16
    //  shape there; the quad select and the synchronised compaction apply)
    if (launch_coarse_variant(x, c.ov, a, nwg, s, &rc)) return rc;   // (A/B builds only)
    if (x->dim == 1024) return launch_coarse_flat<1024, (CF_PRODUCT_VAR & (3 | 16 | 2048))>(x, a, nwg, s);
    if (pl.wide_lists) return launch_coarse_flat<768, CF_PRODUCT_VAR, CO_KP_WIDE>(x, a, nwg, s);
    if ((size_t)x->n_pad * x->dim * 2 <= COARSE_CACHED_IMAGE_BYTES) return launch_coarse_flat<768, CF_CACHED_VAR>(x, a, nwg, s);   // (the image stays in the Infinity Cache)
    // an image streamed from HBM (a row shard): the classes of work-groups that sweep the same tiles are paced so that a
    // tile is fetched once per XCD instead of once per work-group (coarse_flat_kernel.hpp, VAR 67108864)
    const int t0 = flat_class_period(pl.U, pl.ctiles);
    const int members0 = t0 > 0 ? nwg / t0 : 0;
    const int epochs = x->opt_pace_shift >= 0 ? (pl.U >> x->opt_pace_shift) + 1 : 0;
    if (x->opt_pace_shift >= 0 && members0 >= 4 && (size_t)t0 * epochs <= PACE_WORDS) {
        a.pace = x->pace; a.pace_period = t0; a.pace_epochs = epochs; a.pace_shift = x->opt_pace_shift; a.pace_lead = std::max(1, x->opt_pace_lead);
        HIP_TRY(hipMemsetAsync(x->pace, 0, (size_t)t0 * epochs * sizeof(unsigned int), s));
    }
    return launch_coarse_flat<768, CF_PACED_VAR>(x, a, nwg, s);
}

// The first finalize: certifies and rescores every query from the first pass's lists; `g` is left as the base of the
// launches behind it (all queries, in query order). *wide_fin: it ran with the widest window already.
int auto_first_finalize(const SearchCtx &c, const AutoPlan &pl, FinArgs &g, bool *wide_fin) {
    icd_index *x = c.x;
    const int nq = c.nq, k = c.k;
    hipStream_t s = c.s;
    g = c.f;
    g.part_scores = x->partc_s; g.part_rows = x->partc_r; g.bounds = x->partc_b; g.P = pl.pc; g.KP = pl.kp_c; g.nq = nq;
    g.perm_mul = x->perm_mul; g.perm_mod = x->perm_mod;
    g.perm_inv = (x->perm_mod > 0 && (double)x->perm_mod * (double)x->perm_mod < 9007199254740992.0) ? 1.0 / (double)x->perm_mod : 0.0;
    // Wide mode (a corpus of tight families, decided from earlier counters): the window sized for k would certify
    // next to nothing and its rescoring be thrown away (0.13 of 1.5 ms per 10 000 queries): the widest window takes
    // every query at once, and the retry below has nothing to add.
    *wide_fin = pl.wide_now && k <= 32 && pl.pc * g.KP >= 128;
    if (*wide_fin) g.wide_window = 1;
    if (c.ov.fin_skip_walk) g.skip_walk = 1;
    if (*wide_fin && x->opt_family_order && nq >= 1024) {
        // every query's window is its family (the corpus is in code order): visit the queries family by family, XCD by XCD
        OrderArgs o{};
        o.part_scores = g.part_scores; o.part_rows = g.part_rows; o.P = g.P; o.KP = g.KP; o.nq = nq;
        o.perm_mul = g.perm_mul; o.perm_mod = g.perm_mod; o.perm_inv = g.perm_inv;
        o.shift = 6;
        while (((long long)x->n >> o.shift) >= ORDER_BUCKETS) ++o.shift;
        o.key = x->order_key; o.hist = x->order_hist; o.order = x->order;
        // (the scatter kernel leaves the histogram zero again; a search that failed between the two launches would not:
        //  cleared here, 4 KB, so that a stale count can never push a position past the order buffer)
        HIP_TRY(hipMemsetAsync(x->order_hist, 0, 2 * ORDER_BUCKETS * sizeof(unsigned int), s));
        hipLaunchKernelGGL(order_keys_kernel, dim3((nq + 3) / 4), dim3(256), 0, s, o);
        hipLaunchKernelGGL(order_scatter_kernel, dim3((nq + 1023) / 1024), dim3(1024), 0, s, o);
        HIP_TRY(hipGetLastError());
        g.qlist = x->order; g.lists_by_query = 1; g.nq = 4 * ((nq + 3) / 4);
    }
    const int rc = *wide_fin ? launch_finalize_t<true, false, 4>(x, g, s) : launch_finalize<true>(x, g, s);
    g.qlist = nullptr; g.lists_by_query = 0; g.nq = nq;
    return rc;
}

// Second chance before the exact re-search. A query fails the first pass when more candidates lie within 2 eps of
// its k-th best than the window sized for k holds (32 or 64 for k <= 32): a family of near-identical rows, the
// shape ICD sibling codes have. Its lists may hold 128-512 candidates: the same kernel with the widest window
// (256) certifies it from them in microseconds where the exact sweep costs 2.5-5 us per query
// (profiles/r02_family_corpus_probe.log: 1 000 queries 2.7 / 5.2 ms -> see there). Only launched when the lists can
// fill a wider window (mid-size batches; 10 000 queries have 5 lists of 16); gated on the flagged count on the device.
int auto_wide_retry(const SearchCtx &c, const FinArgs &g) {
    icd_index *x = c.x;
    FinArgs g2 = g;
    g2.qlist = x->flagged; g2.nq_ptr = x->nflag; g2.lists_by_query = 1; g2.wide_window = 1;
    g2.nflag = x->nflag + 1; g2.flagged = x->flagged + x->max_nq_pad;
    const int rc = launch_finalize_t<true, false, 4>(x, g2, c.s);
    if (rc) return rc;
    x->fallback_word = 1;
    return ICD_OK;
}

// Second coarse pass, over the queries that are still flagged only. A large batch gives a query 5-8 lists of 16
// candidates: a family of near-identical rows larger than that (ICD sibling codes repeat their ancestors' names:
// 124-row families of mutual cosine 0.99 sit inside 2 eps of each other) cannot be certified from them, whatever
// the window. The same kernel sweeps the corpus again for the flagged queries with about PASS2_CHUNKS lists each
// (the partition sized on the device from the flagged count, one block per CU looping over the logical
// work-groups), finalize certifies from those lists with the widest window, and only what still fails goes to the
// exact re-search. A batch with nothing flagged pays two launches that read one counter and leave.
int auto_second_pass(const SearchCtx &c, AutoPlan &pl, const FinArgs &g) {
    icd_index *x = c.x;
    hipStream_t s = c.s;
    CoarseFlatArgs &a2 = pl.a2;
    const int w_in = x->fallback_word;
    a2.nq_ptr = x->nflag + w_in;
    a2.qlist = x->flagged + (size_t)w_in * x->max_nq_pad;
    a2.skip_below = PASS2_SKIP;
    const int grid2 = std::max(8, std::min(pl.nwg2, x->num_cu) & ~7);
    int rc;
    if (x->dim == 1024) rc = launch_coarse_flat<1024, (CF_PRODUCT_VAR & (3 | 16 | 2048)), CO_KP, true>(x, a2, grid2, s);
    else rc = launch_coarse_flat<768, CF_PRODUCT_VAR, CO_KP, true>(x, a2, grid2, s);
    if (rc) return rc;
    FinArgs g3 = g;
    g3.part_scores = x->part2_s; g3.part_rows = x->part2_r; g3.bounds = x->part2_b; g3.P = pl.p2; g3.KP = CO_KP;
    g3.qlist = a2.qlist; g3.nq_ptr = a2.nq_ptr; g3.lists_by_query = 0; g3.wide_window = 1; g3.skip_below = PASS2_SKIP;
    g3.nflag = x->nflag + 2; g3.flagged = x->flagged + (size_t)2 * x->max_nq_pad;
    rc = launch_finalize_t<true, false, 4>(x, g3, s);
    if (rc) return rc;
    x->fallback_word = 2;
    x->last_p2 = pl.p2; x->last_p2_word = w_in;
    return ICD_OK;
}

// fallback over the flagged list, both device-side gated on its length: the streaming kernel for
// a sparse list (<= ST_MAX_ACTIVE queries), the fp32-MFMA kernel for a dense one. Both leave
// [slot][p_sparse][KP] lists for the same finalize launch.
int auto_fallback(const SearchCtx &c, bool sparse_off) {
    icd_index *x = c.x;
    const int *fl_list = x->flagged + (size_t)x->fallback_word * x->max_nq_pad;
    const int *fl_count = x->nflag + x->fallback_word;
    int px = std::min(c.p_sparse, c.row_tiles);
    if (px < c.p_sparse) {   // tiny corpus: MFMA kernel only. EVERY query may be flagged (all-zero queries, duplicate rows):
        // the list count is sized against the workspace like a full exact run
        const int rc = fit_chunks(c, &px);
        if (rc) return rc;
        return run_exact(c, fl_list, fl_count, px, true, false, true, true, c.f.thr0);
    }
    return run_exact(c, fl_list, fl_count, c.p_sparse, true, c.stream_ok, !sparse_off, true, c.f.thr0);
}

int search_auto(const SearchCtx &c) {
    icd_index *x = c.x;
    const int nq_pad = ((c.nq + 127) / 128) * 128;
    int rc = auto_prep(c, nq_pad);
    if (rc) return rc;
    AutoPlan pl;
    rc = auto_plan(c, nq_pad, pl);
    if (rc) return rc;
    rc = auto_coarse(c, pl);
    if (rc) return rc;
    rec(x, 2, c.s);
    FinArgs g;
    bool wide_fin = false;
    rc = auto_first_finalize(c, pl, g, &wide_fin);
    if (rc) return rc;
    x->fallback_word = 0;
    if (!wide_fin && c.k <= 32 && pl.pc * g.KP >= 128) {
        rc = auto_wide_retry(c, g);
        if (rc) return rc;
    }
    if (pl.p2 > 0) {
        rc = auto_second_pass(c, pl, g);
        if (rc) return rc;
    }
    policy_note_search(x->pol, x->adapt_enabled, x->pass2_enabled, c.nq, pl.p2, pl.wide_now, x->chunks_override, pl.pc * pl.kp_c);
    rec(x, 3, c.s);
    return auto_fallback(c, pl.sparse_off);
}

// Enqueue a search whose queries and outputs are device pointers.
// band: a range search (icd_index_search_range; mode EXACT) - the streaming forms up to ST_MAX_ACTIVE queries, plain lists of
// KP >= k on the MFMA kernel above; nullptr for every other caller, and no band kernel runs.
// mask (with band): a masked search (icd_index_search_masked) - the same dispatch, the instantiations with the row-mask term.
// boost (with band and mask): a boosted search (icd_index_search_boosted) - the same dispatch again, the instantiations with the multiply.
int search_device(icd_index *x, const float *dq, int nq, int k, int mode, const Outs &o, hipStream_t s, const BandArgs *band = nullptr, RowMasks mask = nullptr,
                  const BoostDev *boost = nullptr) {
    const bool use_fast = !band && (mode == ICD_MODE_AUTO) && x->fast && k <= FAST_MAX_K && (x->dim == 768 || x->dim == 1024);
    x->prof_now = !x->capturing && x->profiling && (x->prof_tick++ % x->prof_every == 0);
    if (x->prof_now) {
        const int slot = (int)(x->prof_count % EV_RING);
        x->ev = x->evring[slot];
        x->ev_valid = x->evring_valid[slot];
        ++x->prof_count;
        for (int i = 0; i <= NUM_EV; ++i) x->ev_valid[i] = false;
    }
    x->last_nq = nq;
    x->fallback_word = 0;
    x->last_p2 = 0;
    x->last_mode = use_fast ? ICD_MODE_AUTO : ICD_MODE_EXACT;
    rec(x, 0, s);
    const SearchCtx c = make_search_ctx(x, dq, nq, k, use_fast, o, s, band, mask, boost);
    // (k > 16 needs the 64-entry lists of the streaming kernel, ~0.9 ms per 16 queries: the coarse pass is faster there)
    const bool tiny = c.stream_ok && nq <= (use_fast ? (k <= 16 ? 16 : 0) : ST_MAX_ACTIVE);
    if ((tiny || !use_fast) && (x->pol.last_narrow_large || x->pol.p2_eval_pending)) {
        // every path but search_auto overwrites the counters the last planned search left (search_policy.hpp): judged now or never
        const bool arrived = !x->capturing && x->h_nflag && x->ev_nflag && hipEventQuery(x->ev_nflag) == hipSuccess;
        const SearchCounters left = arrived ? search_counters(x->h_nflag) : SearchCounters{};
        policy_unplanned_search(x->pol, arrived ? &left : nullptr);
    }
    if (tiny) return search_tiny(c);
    { const int rcq = stage_host_query(c); if (rcq) return rcq; }
    { const int rcb = stage_host_bands(c); if (rcb) return rcb; }
    if (!band && !use_fast && c.kpx > 32 && x->opt_exact_narrow && nq > ST_MAX_ACTIVE && c.row_tiles >= 64) {
        bool taken = false;
        const int rc = search_exact_narrow(c, &taken);
        if (rc || taken) return rc;
    }
    return use_fast ? search_auto(c) : search_exact(c);
}

}  // namespace

extern "C" {

int icd_abi_version(void) { return ICD_ABI_VERSION; }

const char *icd_last_error(void) { return g_err.c_str(); }

int icd_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return fail(ICD_ERR_HIP, "hipGetDeviceCount: %s", hipGetErrorString(e));
    return n;
}

}  // extern "C"

// icd_index_create, and the build of a view (icd_index_create_view): with `view_map` the corpus and levels are the PARENT's device
// buffers and the index takes rows view_map[i] - id_base of them (gather_view_rows_kernel) instead of a copy of the first n; the rest
// of the build - fp16 image, centring, workspace, probe - is the same. The caller owns view_map (it becomes the view's row map).
static int create_index(const float *corpus, int64_t n, int32_t dim, const int32_t *levels, int64_t id_base,
                        int32_t device, int32_t max_nq, int32_t max_k, int32_t flags, const long long *view_map,
                        icd_index **out) {
    if (!out) return fail(ICD_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (flags & ~(ICD_CREATE_CORPUS_ON_DEVICE | ICD_CREATE_ROW_ORDER | ICD_CREATE_NO_PROBE | ICD_CREATE_NO_CENTER)) return fail(ICD_ERR_INVALID, "flags=0x%x: unknown bits", flags);
    const int32_t corpus_on_device = flags & ICD_CREATE_CORPUS_ON_DEVICE;
    if (!corpus || n <= 0 || n > 0x7FFFFF00ll) return fail(ICD_ERR_INVALID, "corpus NULL or n=%lld out of range", (long long)n);
    if (dim <= 0 || dim % 32 != 0 || dim > 4096) return fail(ICD_ERR_UNSUPPORTED, "dim=%d: must be a multiple of 32, <= 4096", dim);
    if (max_nq <= 0 || max_k <= 0 || max_k > ICD_MAX_K) return fail(ICD_ERR_INVALID, "max_nq=%d max_k=%d (max_k <= %d)", max_nq, max_k, ICD_MAX_K);
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(ICD_ERR_INVALID, "device %d of %d", device, ndev);
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(ICD_ERR_UNSUPPORTED, "device %d is %s; this library is built for gfx950 (MI355X) only", device, prop.gcnArchName);

    icd_index *x = new (std::nothrow) icd_index();
    if (!x) return fail(ICD_ERR_NOMEM, "host allocation failed");
    x->device = device; x->n = n; x->id_base = id_base; x->dim = dim;
    { static std::atomic<unsigned long long> next_uid{0}; x->uid = ++next_uid; }
    x->opt_permute = !(flags & ICD_CREATE_ROW_ORDER); x->opt_probe = !(flags & ICD_CREATE_NO_PROBE); x->opt_center = !(flags & ICD_CREATE_NO_CENTER);
    x->n_pad = (int)(((n + 127) / 128 + FLAT_SPARE_TILES) * 128);   // (zero tiles behind the fp16 image: plan_flat_tiles)
    x->max_nq = max_nq; x->max_nq_pad = ((max_nq + 127) / 128) * 128; x->max_k = max_k;
    x->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    const bool fast_dim = (dim == 768 || dim == 1024);

#define CR_TRY(expr) HIP_TRY_OR(free_all(x), expr)
    const size_t nelem = (size_t)n * dim;
    // ST_PAD_ROWS zero rows behind the corpus: the streaming kernel's stages run to the next 256-row boundary
    CR_TRY(dmalloc(&x->corpus, nelem + (size_t)ST_PAD_ROWS * dim));
    CR_TRY(hipMemset(x->corpus + nelem, 0, (size_t)ST_PAD_ROWS * dim * sizeof(float)));
    if (levels) CR_TRY(dmalloc(&x->levels, (size_t)n));
    if (view_map) {   // (the parent's rows, gathered on the device: nothing crosses PCIe)
        hipLaunchKernelGGL(gather_view_rows_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, 0, corpus, levels, view_map,
                           (long long)id_base, (long long)n, dim, x->corpus, x->levels);
        CR_TRY(hipGetLastError());
    } else {
        CR_TRY(hipMemcpy(x->corpus, corpus, nelem * sizeof(float), corpus_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
        if (levels)
            CR_TRY(hipMemcpy(x->levels, levels, (size_t)n * sizeof(int), corpus_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    }
    CR_TRY(dmalloc(&x->scratch_u32, 8));
    CR_TRY(hipMemset(x->scratch_u32, 0, 8 * sizeof(unsigned)));
    size_t ws = 0;
    auto wsalloc = [&](auto **p, size_t count) -> hipError_t {
        hipError_t e = dmalloc(p, count);
        if (e == hipSuccess) ws += std::max<size_t>(count, 1) * sizeof(**p);
        return e;
    };
    if (fast_dim) {
        CR_TRY(dmalloc(&x->c16, (size_t)x->n_pad * dim));
        // Row order of the fp16 copy: a corpus in code order keeps families of near-identical rows next to each
        // other, so ONE candidate list would collect a query's whole family, end on a bound inside it and fail the
        // certificate. An affine permutation with a golden-ratio stride spreads neighbours evenly over the lists;
        // finalize maps list positions back with the same formula (no table). (ICD_CREATE_ROW_ORDER keeps the order:
        // a process-wide test switch, read at create; results are identical either way.)
        if (n > 2 && x->opt_permute) {
            long long a_ = (long long)(0.6180339887498949 * (double)n) | 1;
            auto gcd = [](long long u, long long v) { while (v) { const long long t = u % v; u = v; v = t; } return u; };
            while (gcd(a_, n) != 1) a_ += 2;
            x->perm_mul = a_ % n; x->perm_mod = (int)n;
        }
        // pass 0: the column mean; the image is centred when the rows share a large common component (coarse_common.hpp)
        if (n >= 64) {
            const int nb = (int)std::min<int64_t>(256, n);
            // the three temporaries of this pass come out of ONE allocation that a scope guard frees on every way out: a failure
            // between the allocations and the end of the pass (the next dmalloc, a launch, the copy) used to leak them, on the
            // 1.25 M-row shards exactly when memory is tightest (CR_TRY only frees the index)
            float *tmp3 = nullptr;
            struct Guard { float *&p; ~Guard() { if (p) hipFree(p); p = nullptr; } } tmp3_guard{tmp3};
            CR_TRY(dmalloc(&tmp3, (size_t)nb * dim + (size_t)nb + 2));
            float *part = tmp3, *sqp = tmp3 + (size_t)nb * dim, *out2 = sqp + nb;
            CR_TRY(dmalloc(&x->cmean, (size_t)dim));
            hipLaunchKernelGGL(column_sum_partial_kernel, dim3(nb), dim3(256), 0, 0, x->corpus, (int)n, dim, part, sqp);
            hipLaunchKernelGGL(column_sum_final_kernel, dim3(1), dim3(256), 0, 0, part, sqp, nb, (int)n, dim, x->cmean, out2);
            CR_TRY(hipGetLastError());
            float h2[2] = {0.f, 0.f};
            CR_TRY(hipMemcpy(h2, out2, sizeof h2, hipMemcpyDeviceToHost));
            x->mean_share = h2[1] > 0.f ? h2[0] / h2[1] : 0.f;
            if (!x->opt_center || !(x->mean_share >= CENTER_MIN_SHARE) || !std::isfinite(h2[0]) || !std::isfinite(h2[1])) { hipFree(x->cmean); x->cmean = nullptr; }
        }
        // pass 1: largest component of the corpus -> ONE power-of-two scale for its fp16 image; pass 2: convert
        ConvertArgs cv{};
        cv.src = x->corpus; cv.dst = x->c16; cv.rows = (int)n; cv.rows_pad = x->n_pad; cv.dim = dim; cv.mu = x->cmean;
        cv.amax_bits = x->scratch_u32 + 2; cv.any_bad = x->scratch_u32 + 1; cv.mode = 2;
        hipLaunchKernelGGL(convert_rows_kernel, dim3((x->n_pad + 3) / 4), dim3(256), 0, 0, cv);
        CR_TRY(hipGetLastError());
        unsigned hv[5] = {0, 0, 0, 0, 0};
        CR_TRY(hipMemcpy(hv, x->scratch_u32, sizeof hv, hipMemcpyDeviceToHost));
        float amax = 0.f;
        memcpy(&amax, &hv[2], 4);
        x->cexp = scale_exp_for(amax);
        cv.mode = 1; cv.fixed_exp = x->cexp; cv.amax_bits = nullptr;
        cv.rmax_bits = x->scratch_u32; cv.resmax_bits = x->scratch_u32 + 4;
        if (x->cmean) cv.norm_raw_max = reinterpret_cast<float *>(x->scratch_u32 + 3);
        cv.perm_mul = x->perm_mul; cv.perm_mod = x->perm_mod;
        hipLaunchKernelGGL(convert_rows_kernel, dim3((x->n_pad + 3) / 4), dim3(256), 0, 0, cv);
        CR_TRY(hipGetLastError());
        CR_TRY(hipMemcpy(hv, x->scratch_u32, sizeof hv, hipMemcpyDeviceToHost));
        memcpy(&x->rmax_scaled, &hv[0], 4);
        memcpy(&x->dcmax_scaled, &hv[4], 4);
        x->rmax = ldexpf(x->rmax_scaled, -x->cexp);
        if (x->cmean) {   // (rmax as reported stays the largest UNcentred norm; the certificate uses both)
            float raw = 0.f;
            memcpy(&raw, &hv[3], 4);
            x->rmax = raw;
            x->rmax_unc_scaled = ldexpf(raw, x->cexp);
        }
        x->fast = (hv[1] == 0) && std::isfinite(x->rmax_scaled);
        if (!x->fast) { hipFree(x->c16); x->c16 = nullptr; }
    }
    if (x->fast) {
        CR_TRY(wsalloc(&x->q16, (size_t)x->max_nq_pad * dim));
        // candidate lists of the coarse pass: about k / 4 lists of 16 up to k = 64, about k / 6 lists of 24 above (+ the
        // lists that work-group boundaries add)
        // (+ the wide partition of large batches on family-shaped corpora, wide_mode: PASS2_MAX_P lists of CO_KP; flat_partition.hpp)
        x->partc_cap = (size_t)coarse_partc_entries(x->max_nq_pad, std::min(max_k, FAST_MAX_K), CO_KP, CO_KP_WIDE, FIN_MAX_CAND);
        CR_TRY(wsalloc(&x->partc_s, x->partc_cap));
        CR_TRY(wsalloc(&x->partc_r, x->partc_cap));
        CR_TRY(wsalloc(&x->partc_b, x->partc_cap / CO_KP));
        x->part2_cap = (size_t)coarse_part2_entries(x->max_nq_pad, CO_KP);
        CR_TRY(wsalloc(&x->part2_s, x->part2_cap));
        CR_TRY(wsalloc(&x->part2_r, x->part2_cap));
        CR_TRY(wsalloc(&x->part2_b, x->part2_cap / CO_KP));
    }
    CR_TRY(wsalloc(&x->qnorm, (size_t)x->max_nq_pad));
    CR_TRY(wsalloc(&x->qres, (size_t)x->max_nq_pad));
    CR_TRY(wsalloc(&x->qexp, (size_t)x->max_nq_pad));
    CR_TRY(wsalloc(&x->qbad, (size_t)x->max_nq_pad));
    CR_TRY(wsalloc(&x->thr0, (size_t)x->max_nq_pad));
    CR_TRY(wsalloc(&x->shared_thr, (size_t)2 * x->max_nq_pad));   // [0]: first coarse pass, [1]: second
    CR_TRY(wsalloc(&x->qdev, (size_t)max_nq * dim));
    x->partx_cap = std::max<size_t>((size_t)x->max_nq_pad * 2 * exact_kp_for(max_k), (size_t)1 << 21);
    if (exact_kp_for(max_k) > 16)   // multi-level reduction of the streaming kernel's lists: ST_MAX_ACTIVE slots x 512 lists
        x->partx_cap = std::max<size_t>(x->partx_cap, (size_t)ST_MAX_ACTIVE * 512 * exact_kp_for(max_k));
    // (+ one query tile of the widest layout: the device-chosen chunk count of the fallback rounds the slot count up)
    CR_TRY(wsalloc(&x->partx_s, x->partx_cap + (size_t)128 * FIN_MAX_CAND_X));
    CR_TRY(wsalloc(&x->partx_r, x->partx_cap + (size_t)128 * FIN_MAX_CAND_X));
    x->lists_cap = std::max((size_t)ST_MAX_ACTIVE * 1024 * exact_kp_for(max_k), (size_t)ST_FALLBACK_MAX_ACTIVE * 1024 * 16);
    CR_TRY(wsalloc(&x->lists_s, x->lists_cap));
    CR_TRY(wsalloc(&x->lists_r, x->lists_cap));
    CR_TRY(wsalloc(&x->nflag, 8));
    CR_TRY(hipMemset(x->nflag, 0, 8 * sizeof(int)));
    CR_TRY(hipHostMalloc(reinterpret_cast<void **>(&x->h_nflag), 8 * sizeof(int), hipHostMallocMapped));
    memset(x->h_nflag, 0, 8 * sizeof(int));
    CR_TRY(hipHostGetDevicePointer(reinterpret_cast<void **>(&x->h_nflag_dev), x->h_nflag, 0));
    CR_TRY(hipEventCreateWithFlags(&x->ev_nflag, hipEventDisableTiming));
    CR_TRY(hipHostMalloc(reinterpret_cast<void **>(&x->h_pin), PIN_Q_BYTES + PIN_OUT_BYTES + PIN_DONE_BYTES, hipHostMallocMapped));
    CR_TRY(hipHostGetDevicePointer(reinterpret_cast<void **>(&x->h_pin_dev), x->h_pin, 0));
    memset(x->h_pin + PIN_Q_BYTES + PIN_OUT_BYTES, 0, PIN_DONE_BYTES);   // (the completion word: sequence numbers start at 1)
    CR_TRY(wsalloc(&x->band_dev, (size_t)max_nq));
    CR_TRY(hipHostMalloc(reinterpret_cast<void **>(&x->h_band), (size_t)max_nq * sizeof(BandQ), hipHostMallocDefault));
    if (!view_map) {   // (row masks are the parent's alternative to a view: a view has none)
        CR_TRY(wsalloc(&x->mask_dev, (size_t)max_nq));
        CR_TRY(hipHostMalloc(reinterpret_cast<void **>(&x->h_mask), (size_t)max_nq * sizeof(uint32_t *), hipHostMallocDefault));
        CR_TRY(hipEventCreateWithFlags(&x->ev_mask, hipEventDisableTiming));
        const size_t mw = (size_t)rowmask_tile_words(n) + ROWMASK_TAIL_WORDS;
        std::vector<uint32_t> ones(mw, 0u);
        for (int64_t r = 0; r < n; r += 32) ones[(size_t)(r >> 5)] = n - r >= 32 ? ~0u : ((1u << (n - r)) - 1u);
        CR_TRY(wsalloc(&x->mask_ones, mw));
        CR_TRY(hipMemcpy(x->mask_ones, ones.data(), mw * sizeof(uint32_t), hipMemcpyHostToDevice));
        // the ordered select's scratch and staging (icd_rowmask_select allocates nothing)
        CR_TRY(wsalloc(&x->sel_counts, (size_t)ms_scratch_counts(n, max_nq)));
        CR_TRY(wsalloc(&x->sel_off, (size_t)max_nq));
        CR_TRY(hipHostMalloc(reinterpret_cast<void **>(&x->h_sel_off), (size_t)max_nq * sizeof(long long), hipHostMallocDefault));
        x->sel_out_cap = (size_t)ms_host_slots(max_nq);
        CR_TRY(wsalloc(&x->sel_ids, x->sel_out_cap));
        CR_TRY(wsalloc(&x->sel_total, (size_t)max_nq));
        CR_TRY(wsalloc(&x->sel_taken, (size_t)max_nq));
    }
    CR_TRY(wsalloc(&x->pace, PACE_WORDS));
    CR_TRY(wsalloc(&x->dbg, (size_t)8192 * 16));
    CR_TRY(hipMemset(x->dbg, 0, (size_t)8192 * 16 * 8));
    CR_TRY(wsalloc(&x->flagged, (size_t)3 * x->max_nq_pad));
    CR_TRY(wsalloc(&x->order, (size_t)x->max_nq_pad + 8));
    CR_TRY(wsalloc(&x->order_key, (size_t)x->max_nq_pad));
    CR_TRY(wsalloc(&x->order_hist, (size_t)2 * ORDER_BUCKETS));
    CR_TRY(hipMemset(x->order_hist, 0, 2 * ORDER_BUCKETS * sizeof(unsigned int)));
    const size_t no = (size_t)max_nq * max_k;
    CR_TRY(wsalloc(&x->o_scores, no)); CR_TRY(wsalloc(&x->o_ids, no)); CR_TRY(wsalloc(&x->o_adj, no));
    CR_TRY(wsalloc(&x->o_adj_raw, no)); CR_TRY(wsalloc(&x->o_adj_ids, no)); CR_TRY(wsalloc(&x->o_adj_lv, no));
    for (int r = 0; r < EV_RING; ++r)
        for (int i = 0; i <= NUM_EV; ++i) CR_TRY(hipEventCreate(&x->evring[r][i]));
    CR_TRY(hipDeviceSynchronize());
    x->bytes_ws = ws;
    // ---- corpus-shape probe ---------------------------------------------------------------------------------------------
    // Whether large batches should start with the wide partition (wide_mode) is a property of the CORPUS: families of
    // near-identical rows (ICD sibling codes repeat their ancestors' names) put more rows inside 2 eps of a query's k-th
    // best than the narrow plan's 5-8 lists can hold. The counters of a first user batch would tell (and later ones do,
    // search_device) - but the corpus can be asked now: WIDE_MIN_NQ of its own rows, evenly spaced, are searched as one
    // large batch (each finds itself and its family), and the same rule decides. A fresh index on a family corpus then
    // answers its FIRST large batch in 1.5 ms per 10 000 queries instead of 2.0-2.2; a Gaussian corpus flags nothing
    // and stays narrow. Costs one 2 048-query search at create; state and counters are reset afterwards.
    if (x->fast && max_nq >= WIDE_MIN_NQ && n >= (int64_t)4 * WIDE_MIN_NQ && dim % 4 == 0 && x->opt_probe) {
        const int pq = WIDE_MIN_NQ, pk = std::min(10, max_k);
        hipLaunchKernelGGL(gather_rows_kernel, dim3(pq), dim3(192), 0, 0, x->corpus, x->qdev, (long long)(n / pq), dim, pq);
        CR_TRY(hipGetLastError());
        Outs o{};
        o.adj = x->o_adj; o.adj_raw = x->o_adj_raw; o.adj_ids = x->o_adj_ids; o.adj_lv = x->o_adj_lv;
        const int prc = search_device(x, x->qdev, pq, pk, ICD_MODE_AUTO, o, 0);
        if (prc) { free_all(x); return prc; }
        CR_TRY(hipDeviceSynchronize());
        x->probe_flagged = x->h_nflag[0]; x->probe_left = x->h_nflag[2];
        policy_take_counters(x->pol, search_counters(x->h_nflag));   // (the rule of every later search decides)
        x->pol.reset();
        x->last_nq = 0; x->last_p2 = 0; x->fallback_word = 0; x->last_chunks = 0; x->last_mode = ICD_MODE_AUTO;
        CR_TRY(hipMemset(x->nflag, 0, 8 * sizeof(int)));
        memset(x->h_nflag, 0, 8 * sizeof(int));
    }
#undef CR_TRY
    *out = x;
    return ICD_OK;
}

// ---- what the search entry points share ----------------------------------------------------------------------------------------
// One body per concern; every entry family (plain, reweighted, range, masked, grouped, hybrid) goes through these.

// The identity of the index an owned handle (row mask, grouping, fusion) was created for. A handle keeps no pointer INTO the index:
// address and identity are compared, never followed. The uid tells an index re-created at the address of a closed one from it.
struct OwnerStamp {
    const icd_index *owner = nullptr;
    unsigned long long uid = 0;
    int device = 0, dim = 0;
    int64_t n = 0;
    void stamp(const icd_index *idx) { owner = idx; uid = idx->uid; device = idx->device; dim = idx->dim; n = idx->n; }
    bool belongs_to(const icd_index *idx) const { return owner == idx && uid == idx->uid && device == idx->device && dim == idx->dim && n == idx->n; }
};
static int check_owner(const OwnerStamp &at, const icd_index *idx, const char *what, long long entry = -1) {
    if (at.belongs_to(idx)) return ICD_OK;
    char name[48];
    if (entry >= 0) { snprintf(name, sizeof name, "%s[%lld]", what, entry); what = name; }   // (an entry of a table)
    return fail(ICD_ERR_INVALID, "%s was created for another index", what);
}

// What the three owned handles are made of: magic, stamp, and their device allocations - everything alloc() handed out goes in
// free_handle. Each handle type adds MAGIC, NOUN (its name in messages) and its own fields.
struct OwnedHandle {
    uint32_t magic = 0;
    OwnerStamp at;
    std::vector<void *> allocs;
    std::vector<void *> pinned;   // pinned host blocks (hipHostMalloc), freed with the handle
    size_t bytes = 0;
    template <typename T>
    hipError_t alloc(T **p, size_t count) {
        const hipError_t e = dmalloc(p, count);
        if (e == hipSuccess) allocs.push_back(*p);
        return e;
    }
};
template <typename H>
H *new_handle(const icd_index *idx) {
    H *h = new (std::nothrow) H();
    if (h) { h->magic = H::MAGIC; h->at.stamp(idx); }
    return h;
}
template <typename H>
bool valid_handle(const H *h) { return h && h->magic == H::MAGIC; }
template <typename H>
void free_handle(H *h) {
    if (!h) return;
    for (void *p : h->allocs) hipFree(p);
    for (void *p : h->pinned) hipHostFree(p);
    h->magic = 0;
    delete h;
}
template <typename H>
int destroy_handle(H *h) {
    if (!valid_handle(h)) return fail(ICD_ERR_STATE, "invalid %s handle", H::NOUN);
    hipSetDevice(h->at.device);
    hipDeviceSynchronize();
    free_handle(h);
    return ICD_OK;
}

// The capture state of a stream and what it forbids. Device-in / device-out searches are graph-capturable (no allocation, no
// synchronisation, no query while capturing); whatever synchronises or is staged on the host at call time is refused.
static bool stream_capturing(hipStream_t s) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    return s != nullptr && hipStreamIsCapturing(s, &cs) == hipSuccess && cs == hipStreamCaptureStatusActive;
}
static int check_capture(hipStream_t s, bool host_buffers, bool host_bounds, bool mask_table, bool *capturing = nullptr, bool boost_table = false) {
    const bool on = stream_capturing(s);
    if (capturing) *capturing = on;
    if (!on) return ICD_OK;
    if (host_buffers) return fail(ICD_ERR_INVALID, "a search with host buffers synchronises: it cannot be captured into a graph");
    if (host_bounds) return fail(ICD_ERR_INVALID, "a range search with host bounds synchronises: it cannot be captured into a graph");
    if (boost_table) return fail(ICD_ERR_INVALID, "a boosted search stages its boost table on the host at call time: it cannot be captured into a graph");
    if (mask_table) return fail(ICD_ERR_INVALID, "a masked search stages its mask table on the host at call time: it cannot be captured into a graph");
    return ICD_OK;
}

// A call whose queries or outputs may be host memory: the queries go to a device staging, the kernels write to device staging in
// place of host outputs, the outputs are copied back behind them and the call ends with ONE stream synchronisation.
struct HostOut { void *host; const void *dev; size_t elem; };   // (host == nullptr: an output the caller did not ask for)
struct HostCall {
    hipStream_t s;
    bool q_on_device, out_on_device;
    int upload(const float *src, float *staging, size_t floats, const float **dq) const {
        *dq = src;
        if (q_on_device) return ICD_OK;
        HIP_TRY(hipMemcpyAsync(staging, src, floats * sizeof(float), hipMemcpyHostToDevice, s));
        *dq = staging;
        return ICD_OK;
    }
    template <typename T>
    T *target(T *user, T *staging) const { return (user && !out_on_device) ? staging : user; }   // where the kernels write this output
    int copy_back(std::initializer_list<HostOut> outs, size_t slots) const {
        if (out_on_device) return ICD_OK;
        for (const HostOut &o : outs)
            if (o.host) HIP_TRY(hipMemcpyAsync(o.host, o.dev, slots * o.elem, hipMemcpyDeviceToHost, s));
        return ICD_OK;
    }
    int finish(bool also = false) const {
        if (!q_on_device || !out_on_device || also) HIP_TRY(hipStreamSynchronize(s));
        return ICD_OK;
    }
};

struct RangeBounds;
struct BoostRequest;
// ONE dense search as every entry point hands it to run_search, its own arguments already checked.
struct SearchRequest {
    const float *queries;
    int64_t nq;
    int k;
    bool q_on_device, out_on_device;
    int mode;
    Outs outs;
    const RangeBounds *range;       // nullptr: no band
    icd_rowmask *const *masks;      // nullptr: no mask table (never an all-NULL table: that is the range search)
    hipStream_t stream;
    const bool *capture_checked = nullptr;   // the stream's capture state when the caller has run check_capture for this very request (hybrid)
    const BoostRequest *boost = nullptr;     // a boosted search (icd_boost.hpp; with a band, never an all-unused table: that is the masked search)
};
static int run_search(icd_index *x, const SearchRequest &r);

// the outputs of the raw (scores, ids, levels) or the reweighted (adj, raw, ids, levels) form
static Outs outs_for(bool reweighted, double *adj, float *raw, int64_t *ids, int *levels) {
    Outs o{};
    if (reweighted) {
        o.adj = adj; o.adj_raw = raw; o.adj_ids = reinterpret_cast<long long *>(ids); o.adj_lv = levels;
    } else {
        o.scores = raw; o.ids = reinterpret_cast<long long *>(ids); o.lv = levels;
    }
    return o;
}

// range and masked search: the bounds, the row masks, their two entry points
#include "icd_range_mask.hpp"
// boosted search: the workspace, the boost table and its staging, the entry point
#include "icd_boost.hpp"

extern "C" {

int icd_index_create(const float *corpus, int64_t n, int32_t dim, const int32_t *levels, int64_t id_base,
                     int32_t device, int32_t max_nq, int32_t max_k, int32_t flags,
                     icd_index **out) {
    return create_index(corpus, n, dim, levels, id_base, device, max_nq, max_k, flags, nullptr, out);
}

int icd_index_create_view(icd_index *parent, const int64_t *rows, int64_t n_rows, int32_t rows_on_device,
                          int32_t max_nq, int32_t max_k, int32_t flags, icd_index **out) {
    if (!out) return fail(ICD_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!valid(parent)) return fail(ICD_ERR_STATE, "invalid parent handle");
    if (!rows || n_rows <= 0) return fail(ICD_ERR_INVALID, "rows NULL or n_rows=%lld: a view holds at least one row", (long long)n_rows);
    if (n_rows > parent->n) return fail(ICD_ERR_INVALID, "n_rows=%lld exceeds the parent's %lld rows", (long long)n_rows, (long long)parent->n);
    if (flags & ~(ICD_CREATE_CORPUS_ON_DEVICE | ICD_CREATE_ROW_ORDER | ICD_CREATE_NO_PROBE | ICD_CREATE_NO_CENTER)) return fail(ICD_ERR_INVALID, "flags=0x%x: unknown bits", flags);
    HIP_TRY(hipSetDevice(parent->device));
    // the ids are checked (and the parent's id_base added) on the host: a few hundred KB at most, the corpus itself stays on the device
    std::vector<long long> map((size_t)n_rows);
    if (rows_on_device) HIP_TRY(hipMemcpy(map.data(), rows, (size_t)n_rows * sizeof(long long), hipMemcpyDeviceToHost));
    else memcpy(map.data(), rows, (size_t)n_rows * sizeof(long long));
    for (int64_t i = 0; i < n_rows; ++i) {
        if (map[i] < 0 || map[i] >= parent->n) return fail(ICD_ERR_INVALID, "rows[%lld]=%lld outside the parent's [0, %lld)", (long long)i, map[i], (long long)parent->n);
        if (i > 0 && map[i] <= map[i - 1]) return fail(ICD_ERR_INVALID, "rows[%lld]=%lld: row ids must be strictly increasing", (long long)i, map[i]);
    }
    // (behind the check, not inside it: rows[i] was compared with rows[i - 1] + id_base, and no view of an index with an id_base could be made)
    for (int64_t i = 0; i < n_rows; ++i) map[i] += parent->id_base;
    long long *dmap = nullptr;
    HIP_TRY(dmalloc(&dmap, (size_t)n_rows));
    hipError_t e = hipMemcpy(dmap, map.data(), (size_t)n_rows * sizeof(long long), hipMemcpyHostToDevice);
    if (e != hipSuccess) { hipFree(dmap); return fail(ICD_ERR_HIP, "hipMemcpy (row map): %s", hipGetErrorString(e)); }
    const int rc = create_index(parent->corpus, n_rows, parent->dim, parent->levels, parent->id_base, parent->device, max_nq, max_k,
                                flags | ICD_CREATE_CORPUS_ON_DEVICE, dmap, out);
    if (rc) { hipFree(dmap); return rc; }
    (*out)->row_map = dmap;
    (*out)->h_row_map = std::move(map);
    (*out)->bytes_ws += (size_t)n_rows * sizeof(long long);
    return ICD_OK;
}

int icd_index_destroy(icd_index *idx) {
    if (!valid(idx)) return fail(ICD_ERR_STATE, "invalid handle");
    hipSetDevice(idx->device);
    hipDeviceSynchronize();
    free_all(idx);
    return ICD_OK;
}

constexpr long DONE_POLL_US = 500;   // how long a ONE-query host call polls its completion word before it waits for the stream instead
// results of a small host call: out of the mapped block (the six arrays back to back, 8-byte ones first)
static void copy_pinned_out(icd_index *x, const Outs &user, size_t no_small) {
    const char *h = x->h_pin + PIN_Q_BYTES;
    if (user.adj) memcpy(user.adj, h, no_small * 8);              h += no_small * 8;
    if (user.ids) memcpy(user.ids, h, no_small * 8);              h += no_small * 8;
    if (user.adj_ids) memcpy(user.adj_ids, h, no_small * 8);      h += no_small * 8;
    if (user.scores) memcpy(user.scores, h, no_small * 4);        h += no_small * 4;
    if (user.adj_raw) memcpy(user.adj_raw, h, no_small * 4);      h += no_small * 4;
    if (user.adj_lv) memcpy(user.adj_lv, h, no_small * 4);
    else if (user.lv) memcpy(user.lv, h, no_small * 4);
}

}  // extern "C"

// The internal search call: takes the handle's mutex, owns the capture flags, packs the bands and stages the mask table. The
// public entry points and the hybrid search's step 1 call it with a request whose own arguments they have checked; what is
// checked here is the request against THIS index.
static int run_search(icd_index *x, const SearchRequest &r) {
    if (!valid(x)) return fail(ICD_ERR_STATE, "invalid handle");
    std::lock_guard<std::mutex> guard(x->mu);
    const int64_t nq = r.nq;
    const int k = r.k;
    if (nq < 0 || nq > x->max_nq) return fail(ICD_ERR_INVALID, "nq=%lld exceeds max_nq=%d", (long long)nq, x->max_nq);
    if (k <= 0 || k > x->max_k) return fail(ICD_ERR_INVALID, "k=%d exceeds max_k=%d", k, x->max_k);
    if (r.mode != ICD_MODE_AUTO && r.mode != ICD_MODE_EXACT) return fail(ICD_ERR_INVALID, "mode=%d", r.mode);
    if (nq == 0) return ICD_OK;
    if (!r.queries) return fail(ICD_ERR_INVALID, "queries is NULL");
    HIP_TRY(hipSetDevice(x->device));
    hipStream_t s = r.stream;
    const HostCall hc{s, r.q_on_device, r.out_on_device};
    const bool host_bands = r.range && !r.range->on_device;
    int rc = ICD_OK;
    if (r.capture_checked) x->capturing = *r.capture_checked;
    else if ((rc = check_capture(s, !r.q_on_device || !r.out_on_device, host_bands, r.masks != nullptr, &x->capturing, r.boost != nullptr))) return rc;
    if ((r.masks || r.boost) && (rc = stage_masks(x, r.masks, (int)nq, s))) return rc;   // (a boosted search without a mask table: every query unfiltered)
    BoostDev boost{};
    if (r.boost && (rc = stage_boosts(*r.boost, (int)nq, s, &boost))) return rc;
    BandArgs band{};
    x->band_pending = 0;
    if (r.range && (rc = pack_bands(x, *r.range, (int)nq, s, &band))) return rc;
    const float *dq = x->qdev;
    const size_t qbytes = (size_t)nq * x->dim * sizeof(float);
    if (!r.q_on_device && nq == 1 && (x->opt_host_one & 1) && qbytes <= sizeof(StreamInlineQuery) && !x->capturing) {
        x->host_q = r.queries;   // ONE query: search_device puts it into the single-launch kernel's arguments (or copies it after all)
    } else {
        const float *src = r.queries;
        if (!r.q_on_device && qbytes <= PIN_Q_BYTES) { memcpy(x->h_pin, src, qbytes); src = reinterpret_cast<const float *>(x->h_pin); }
        if ((rc = hc.upload(src, x->qdev, (size_t)nq * x->dim, &dq))) return rc;
    }
    const Outs &user = r.outs;
    Outs dev = user;
    const size_t no = (size_t)nq * k;
    const bool pinned_out = !r.out_on_device && no * 36 <= PIN_OUT_BYTES;
    if (pinned_out) {   // the six arrays back to back in the mapped block, 8-byte ones first
        char *d = x->h_pin_dev + PIN_Q_BYTES;
        dev.adj = user.adj ? reinterpret_cast<double *>(d) : nullptr;                          d += no * 8;
        dev.ids = user.ids ? reinterpret_cast<long long *>(d) : nullptr;                       d += no * 8;
        dev.adj_ids = user.adj_ids ? reinterpret_cast<long long *>(d) : nullptr;               d += no * 8;
        dev.scores = user.scores ? reinterpret_cast<float *>(d) : nullptr;                     d += no * 4;
        dev.adj_raw = user.adj_raw ? reinterpret_cast<float *>(d) : nullptr;                   d += no * 4;
        dev.adj_lv = user.adj_lv ? reinterpret_cast<int *>(d) : nullptr;
        dev.lv = (user.lv && !user.adj_lv) ? reinterpret_cast<int *>(d) : nullptr;
    } else {
        dev.scores = hc.target(user.scores, x->o_scores); dev.ids = hc.target(user.ids, x->o_ids);
        dev.adj = hc.target(user.adj, x->o_adj); dev.adj_raw = hc.target(user.adj_raw, x->o_adj_raw);
        dev.adj_ids = hc.target(user.adj_ids, x->o_adj_ids);
        dev.adj_lv = hc.target(user.adj_lv, x->o_adj_lv); dev.lv = hc.target(user.lv, x->o_adj_lv);   // (never both: Outs)
    }
    x->done_armed = false;
    x->host_one_call = !r.q_on_device && nq == 1 && pinned_out && !x->capturing;
    rc = search_device(x, dq, (int)nq, k, r.mode, dev, s, r.range ? &band : nullptr, (r.masks || r.boost) ? x->mask_dev : nullptr, r.boost ? &boost : nullptr);
    x->band_pending = 0;
    x->host_q = nullptr;
    x->host_one_call = false;
    if (rc) return rc;
    rec(x, NUM_EV, s);
    if (x->done_armed && pinned_out) {
        // ONE query through the single-launch kernel: its last work-group stores the call's sequence number behind the outputs
        // (system-scope release). Poll it for a bounded time - no event record, no wait for the queue's completion signal -
        // and fall back to the stream synchronisation (always correct) when the word does not arrive (a busy GPU, a failed launch).
        const volatile unsigned long long *done = reinterpret_cast<const volatile unsigned long long *>(x->h_pin + PIN_Q_BYTES + PIN_OUT_BYTES);
        const auto t0 = std::chrono::steady_clock::now();
        bool seen = false;
        for (unsigned spin = 0;; ++spin) {
            if (__atomic_load_n(done, __ATOMIC_ACQUIRE) == x->done_seq) { seen = true; break; }
            if ((spin & 255u) == 255u && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(DONE_POLL_US)) break;
        }
        if (!seen) HIP_TRY(hipStreamSynchronize(s));
        copy_pinned_out(x, user, no);
        return ICD_OK;
    }
    // the search's last kernel has written the fallback counters to pinned host memory: icd_index_stats reads them after
    // waiting for THIS event only (no device-wide synchronisation: other streams - an encoder - keep running)
    if (!x->capturing) HIP_TRY(hipEventRecord(x->ev_nflag, s));   // (an event recorded inside a capture could not be waited for by icd_index_stats)
    if (pinned_out) {
        HIP_TRY(hipStreamSynchronize(s));   // (the kernels' stores to the mapped block are visible behind it, like the counters')
        copy_pinned_out(x, user, no);
        return ICD_OK;
    }
    if ((rc = hc.copy_back({{user.scores, dev.scores, 4}, {user.ids, dev.ids, 8}, {user.adj, dev.adj, 8}, {user.adj_raw, dev.adj_raw, 4},
                            {user.adj_ids, dev.adj_ids, 8}, {user.adj_lv, dev.adj_lv, 4}, {user.lv, dev.lv, 4}}, no)))
        return rc;
    return hc.finish(host_bands);   // (host bounds went through the pinned block; the mask table's block is guarded by its own event, stage_masks)
}

extern "C" {

int icd_index_search(icd_index *idx, const float *queries, int64_t nq, int32_t k, int32_t queries_on_device,
                     int32_t mode, float *out_scores, int64_t *out_ids, int32_t out_on_device, void *stream) {
    if (!out_scores || !out_ids) return fail(ICD_ERR_INVALID, "output pointer is NULL");
    return run_search(idx, SearchRequest{queries, nq, k, queries_on_device != 0, out_on_device != 0, mode,
                                         outs_for(false, nullptr, out_scores, out_ids, nullptr), nullptr, nullptr, reinterpret_cast<hipStream_t>(stream)});
}

int icd_index_search_reweighted(icd_index *idx, const float *queries, int64_t nq, int32_t k,
                                int32_t queries_on_device, int32_t mode, double *out_adj, float *out_raw,
                                int64_t *out_ids, int32_t *out_levels, int32_t out_on_device, void *stream) {
    if (!out_adj || !out_ids) return fail(ICD_ERR_INVALID, "output pointer is NULL");
    return run_search(idx, SearchRequest{queries, nq, k, queries_on_device != 0, out_on_device != 0, mode,
                                         outs_for(true, out_adj, out_raw, out_ids, out_levels), nullptr, nullptr, reinterpret_cast<hipStream_t>(stream)});
}

int icd_index_lookup_levels(icd_index *idx, const int64_t *ids, int64_t count, int32_t *out_levels, void *stream) {
    if (!valid(idx)) return fail(ICD_ERR_STATE, "invalid handle");
    if (idx->row_map) return fail(ICD_ERR_UNSUPPORTED, "icd_index_lookup_levels: not supported on a view (its hits carry their levels)");
    std::lock_guard<std::mutex> guard(idx->mu);
    if (!ids || !out_levels || count < 0) return fail(ICD_ERR_INVALID, "bad arguments");
    if (count == 0) return ICD_OK;
    HIP_TRY(hipSetDevice(idx->device));
    hipLaunchKernelGGL(lookup_levels_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const long long *>(ids),
                       (long long)count, idx->levels, (long long)idx->id_base, (long long)idx->n, out_levels);
    HIP_TRY(hipGetLastError());
    return ICD_OK;
}

int icd_index_stats(icd_index *idx, icd_stats *out) {
    if (!valid(idx)) return fail(ICD_ERR_STATE, "invalid handle");
    std::lock_guard<std::mutex> guard(idx->mu);
    if (!out) return fail(ICD_ERR_INVALID, "out is NULL");
    memset(out, 0, sizeof *out);
    out->n = idx->n; out->dim = idx->dim; out->device = idx->device; out->id_base = idx->id_base;
    out->bytes_corpus_f32 = (int64_t)idx->n * idx->dim * 4;
    out->bytes_corpus_f16 = idx->c16 ? (int64_t)idx->n_pad * idx->dim * 2 : 0;
    out->bytes_workspace = (int64_t)idx->bytes_ws;
    out->max_nq = idx->max_nq; out->max_k = idx->max_k; out->fast_path = idx->fast ? 1 : 0;
    out->rmax = idx->rmax;
    out->last_nq = idx->last_nq;
    // the last search's fallback count: every search copies its counters to pinned host memory behind itself; this call
    // waits for that copy's event - the last search of THIS handle - and for nothing else on the device
    int nf = 0;
    if (idx->h_nflag && idx->last_nq > 0) {
        HIP_TRY(hipSetDevice(idx->device));
        HIP_TRY(hipEventSynchronize(idx->ev_nflag));
        nf = idx->h_nflag[idx->fallback_word];
    }
    out->last_fallback = nf;
    out->last_second_pass = (idx->last_p2 > 0 && idx->h_nflag && idx->last_nq > 0) ? idx->h_nflag[idx->last_p2_word] : 0;
    out->last_second_pass_lists = idx->last_p2;
    out->wide_mode = idx->pol.wide_mode ? 1 : 0;
    out->second_pass_armed = (idx->pass2_enabled && idx->pol.pass2_armed()) ? 1 : 0;
    out->sparse_fallback_armed = idx->pol.sparse_disarmed ? 0 : 1;
    out->centered = idx->cmean ? 1 : 0; out->mean_share = idx->mean_share;
    out->last_chunks = idx->last_chunks; out->last_mode = idx->last_mode;
    return ICD_OK;
}

int icd_index_cert_terms(icd_index *idx, float *cmax, float *dcmax, int32_t *cexp, float *qnorm, float *qres, int64_t count) {
    if (!valid(idx)) return fail(ICD_ERR_STATE, "invalid handle");
    std::lock_guard<std::mutex> guard(idx->mu);
    if (!idx->fast) return fail(ICD_ERR_INVALID, "the index has no fp16 image");
    if (count < 0 || count > idx->max_nq_pad || ((qnorm || qres) && count > idx->last_nq))
        return fail(ICD_ERR_INVALID, "count=%lld exceeds the last search's batch", (long long)count);
    if (cmax) *cmax = idx->rmax_scaled;
    if (dcmax) *dcmax = idx->dcmax_scaled;
    if (cexp) *cexp = idx->cexp;
    if (count > 0 && (qnorm || qres)) {
        HIP_TRY(hipSetDevice(idx->device));
        HIP_TRY(hipDeviceSynchronize());
        if (qnorm) HIP_TRY(hipMemcpy(qnorm, idx->qnorm, (size_t)count * sizeof(float), hipMemcpyDeviceToHost));
        if (qres) HIP_TRY(hipMemcpy(qres, idx->qres, (size_t)count * sizeof(float), hipMemcpyDeviceToHost));
    }
    return ICD_OK;
}

int icd_index_set_option(icd_index *idx, int32_t option, int32_t value) {
    if (!valid(idx)) return fail(ICD_ERR_STATE, "invalid handle");
    std::lock_guard<std::mutex> guard(idx->mu);
    icd_index *x = idx;
    switch (option) {
    case ICD_OPT_FAMILY_ORDER: x->opt_family_order = (value & 1) != 0; break;
    case ICD_OPT_STREAM_ONE:   x->opt_stream_one = value != 0; break;
    case ICD_OPT_HOST_ONE:     x->opt_host_one = value & 3; break;
    case ICD_OPT_PACING_SHIFT: x->opt_pace_shift = value > 12 ? 12 : value; break;
    case ICD_OPT_PACING_LEAD:  x->opt_pace_lead = value < 1 ? 1 : value; break;
    case ICD_OPT_EXACT_NARROW: x->opt_exact_narrow = value != 0; break;
    case ICD_OPT_WIDE_FROM:    x->opt_wide_from = value < 0 ? 0 : value; break;
    default: return fail(ICD_ERR_INVALID, "option %d: not one of ICD_OPT_*", option);
    }
    return ICD_OK;
}

int icd_index_set_second_pass(icd_index *idx, int32_t enabled) {
    if (!valid(idx)) return fail(ICD_ERR_STATE, "invalid handle");
    std::lock_guard<std::mutex> guard(idx->mu);
    idx->pass2_enabled = enabled != 0;
    idx->adapt_enabled = enabled == 1;
    idx->pol.rearm(idx->pass2_enabled && idx->adapt_enabled);
    if (idx->nflag) { HIP_TRY(hipSetDevice(idx->device)); HIP_TRY(hipDeviceSynchronize()); HIP_TRY(hipMemset(idx->nflag + 4, 0, sizeof(int))); idx->h_nflag[4] = 0; }
    return ICD_OK;
}

int icd_index_set_chunks(icd_index *idx, int32_t chunks) {
    if (!valid(idx)) return fail(ICD_ERR_STATE, "invalid handle");
    std::lock_guard<std::mutex> guard(idx->mu);
    if (chunks < 0 || chunks > COARSE_MAX_P) return fail(ICD_ERR_INVALID, "chunks=%d (0..%d)", chunks, COARSE_MAX_P);
    idx->chunks_override = chunks;
    return ICD_OK;
}

int icd_index_debug_counters(icd_index *idx, unsigned long long *out, int32_t count) {
    if (!valid(idx)) return fail(ICD_ERR_STATE, "invalid handle");
    std::lock_guard<std::mutex> guard(idx->mu);
    if (!out || count <= 0 || count > 8192 * 16) return fail(ICD_ERR_INVALID, "bad arguments");
    HIP_TRY(hipSetDevice(idx->device));
    HIP_TRY(hipMemcpy(out, idx->dbg, (size_t)count * 8, hipMemcpyDeviceToHost));
    return ICD_OK;
}

int icd_index_set_profiling(icd_index *idx, int32_t enabled) {
    if (!valid(idx)) return fail(ICD_ERR_STATE, "invalid handle");
    std::lock_guard<std::mutex> guard(idx->mu);
    if (enabled < 0) return fail(ICD_ERR_INVALID, "enabled=%d", enabled);
    idx->profiling = enabled != 0;
    idx->prof_every = enabled > 1 ? enabled : 1;
    idx->prof_tick = 0;
    return ICD_OK;
}

int icd_index_profile_summary(icd_index *idx, icd_profile *out_mean, int32_t *out_count) {
    if (!valid(idx)) return fail(ICD_ERR_STATE, "invalid handle");
    std::lock_guard<std::mutex> guard(idx->mu);
    if (!out_mean || !out_count) return fail(ICD_ERR_INVALID, "out is NULL");
    memset(out_mean, 0, sizeof *out_mean);
    HIP_TRY(hipSetDevice(idx->device));
    const long total = idx->prof_count;
    const int n = (int)std::min<long>(total, EV_RING);
    int used = 0;
    double acc[6] = {0, 0, 0, 0, 0, 0};
    for (int j = 0; j < n; ++j) {
        const int slot = (int)((total - 1 - j) % EV_RING);
        hipEvent_t *ev = idx->evring[slot];
        const bool *ok = idx->evring_valid[slot];
        if (!ok[0] || !ok[NUM_EV]) continue;
        HIP_TRY(hipEventSynchronize(ev[NUM_EV]));
        auto span = [&](int a, int b) -> double {
            float ms = 0.f;
            if (ok[a] && ok[b]) hipEventElapsedTime(&ms, ev[a], ev[b]);
            return ms;
        };
        acc[0] += span(0, 1); acc[1] += span(1, 2); acc[2] += span(2, 3); acc[3] += span(3, 4);
        acc[4] += span(4, 5); acc[5] += span(0, NUM_EV);
        ++used;
    }
    if (used) {
        out_mean->ms_prep = (float)(acc[0] / used); out_mean->ms_coarse = (float)(acc[1] / used);
        out_mean->ms_finalize = (float)(acc[2] / used); out_mean->ms_exact = (float)(acc[3] / used);
        out_mean->ms_exact_finalize = (float)(acc[4] / used); out_mean->ms_total = (float)(acc[5] / used);
    }
    *out_count = used;
    idx->prof_count = 0;
    for (int r = 0; r < EV_RING; ++r)
        for (int i = 0; i <= NUM_EV; ++i) idx->evring_valid[r][i] = false;
    return ICD_OK;
}

int icd_index_last_profile(icd_index *idx, icd_profile *out) {
    if (!valid(idx)) return fail(ICD_ERR_STATE, "invalid handle");
    std::lock_guard<std::mutex> guard(idx->mu);
    if (!out) return fail(ICD_ERR_INVALID, "out is NULL");
    memset(out, 0, sizeof *out);
    if (!idx->ev_valid[0] || !idx->ev_valid[NUM_EV]) return fail(ICD_ERR_STATE, "no profiled search recorded");
    HIP_TRY(hipSetDevice(idx->device));
    HIP_TRY(hipEventSynchronize(idx->ev[NUM_EV]));
    auto span = [&](int a, int b) -> float {
        float ms = 0.f;
        if (idx->ev_valid[a] && idx->ev_valid[b]) hipEventElapsedTime(&ms, idx->ev[a], idx->ev[b]);
        return ms;
    };
    out->ms_prep = span(0, 1);
    out->ms_coarse = span(1, 2);
    out->ms_finalize = span(2, 3);
    out->ms_exact = span(3, 4);
    out->ms_exact_finalize = span(4, 5);
    out->ms_total = span(0, NUM_EV);
    return ICD_OK;
}

}  // extern "C"

// the other entry families, each its own file in this translation unit (launch_lds's per-kernel state and the kernel templates exist once)
#include "icd_utility.hpp"   // the stateless utility entry points
#include "icd_grouped.hpp"   // the grouping search
#include "icd_maxsim.hpp"    // the embedding-list search: MAX_SIM over a list of vectors per query
#include "icd_hybrid.hpp"    // the hybrid search, the fuse of caller-provided lists
#include "icd_sparse.hpp"    // the sparse-vector search
#include "icd_text_match.hpp" // keyword match filters: row masks from the sparse index's postings
#include "icd_filter.hpp"     // filter programs: row masks from int32 columns and the postings, any boolean shape
#include "icd_facet.hpp"      // facet counts: rows per group of a grouping under a batch of row masks
#include "icd_mmr.hpp"        // MMR search: a diverse top-k out of the exact candidate list
#include "icd_byrows.hpp"     // search by stored rows: gather, the masked search at k + 1, drop the row's own hit
#include "icd_rankof.hpp"     // rank-of search: the targets' scores, then a counting sweep
#include "icd_wide.hpp"       // wide search: ordered scores, radix threshold, ordered collect, sort and emit
#include "icd_recommend.hpp"  // recommend search: example vectors, the wide sweep over them, the fold, the wide select
// the small-input sentence encoder (icd_encoder_*): its own file, this translation unit (fail(), HIP_TRY, packed_attention_kernel)
#include "icd_encoder.hpp"
